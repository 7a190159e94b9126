"""The texts of the BGZF output tests (test_bgzf_write_cpu.py, test_bgzf_write_gpu.py) and what is asked of every file the
encoder writes.  zlib is the judge: gzip.decompress of the file is the text."""
import gzip
import random
import struct
import zlib

import bgzf_ref as R
import seqgen

BT = 65280   # bgzip's block text


def acgt(n, seed):
    r = random.Random(seed)
    return bytes(r.choice(b"ACGT") for _ in range(n))


def _far(dist):
    """300 bytes that come again exactly `dist` later, with nothing but noise between them"""
    head = random.Random(7).randbytes(300)
    return head + random.Random(8).randbytes(dist - 300) + head


def _sized(n, seed):
    """FASTQ-like text of exactly n bytes"""
    return R.fastq_text(n, seed)[:n]


def build():
    """name -> (text, kind); kind "ratio": held against zlib level 1, "stored": incompressible, "": only exactness"""
    rng = random.Random(21)
    T = {
        "empty": (b"", ""),
        "one_byte": (b"x", ""),
        "n65279": (_sized(BT - 1, 3), "ratio"),
        "n65280": (_sized(BT, 4), "ratio"),
        "n65281": (_sized(BT + 1, 5), "ratio"),
        "two_blocks": (_sized(2 * BT, 6), "ratio"),
        "three_blocks_17": (_sized(3 * BT + 17, 7), "ratio"),
        "constant": (b"A" * BT, "ratio"),
        "period2": ((b"AC" * BT)[:BT], "ratio"),
        "period63": ((bytes(range(33, 96)) * 1100)[:BT], "ratio"),
        "period64": ((bytes(range(33, 97)) * 1100)[:BT], "ratio"),
        "period65": ((bytes(range(33, 98)) * 1100)[:BT], "ratio"),
        "far32768": (_far(32768), ""),
        "far32769": (_far(32769), ""),
        "run258": (acgt(100, 1) + b"G" * 700 + acgt(100, 2), ""),
        "acgt": (acgt(BT, 9), "ratio"),
        "random": (random.Random(3).randbytes(BT), "stored"),
        "fasta": (seqgen.random_fasta(rng, 300), "ratio"),
        "fastq": (seqgen.random_fastq(rng, 400), "ratio"),
        "all256": (bytes(range(256)) * 3, ""),
    }
    return T


def fastq_500k():
    return R.fastq_text(500000, 11)


def level1_blocks(text, bt=BT, level=1):
    """what `bgzip -l 1` makes of the text: raw deflate of every block + 26 bytes of frame"""
    total = 0
    for off in range(0, len(text), bt):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        total += len(c.compress(text[off:off + bt]) + c.flush()) + 26
    return total


def check_file(out, text, bt, eof):
    """everything that holds for a file of the encoder whatever wrote it"""
    assert gzip.decompress(out) == text if out else text == b""
    body = out
    if eof:
        assert out[-28:] == R.EOF_BLOCK
        body = out[:-28]
    assert body[-28:] != R.EOF_BLOCK
    nblocks = (len(text) + bt - 1) // bt
    ix = R.index(body) if body else []
    assert len(ix) == nblocks
    at = 0
    for k, (off, bsize, isize, xlen) in enumerate(ix):
        piece = text[at:at + isize]
        assert xlen == 6 and body[off:off + 16] == R.HEADER_SIGNATURE
        assert isize == min(bt, len(text) - at) and isize <= bt
        assert bsize <= isize + 31 and bsize <= 65536
        crc, isz = struct.unpack_from("<II", body, off + bsize - 8)
        assert isz == isize and crc == zlib.crc32(piece) & 0xffffffff
        assert zlib.decompress(body[off + 18:off + bsize - 8], -15) == piece
        at += isize
    assert at == len(text)
