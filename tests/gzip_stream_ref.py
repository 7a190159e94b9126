"""The piece rule of the gzip reader restated for the tests (PARITY.md GZIP "segments"), and the settings the tests read the
corpus of gzip_ref at.  Nothing here is a test; tests/test_gzip_stream_cpu.py and tests/test_gzip_stream_gpu.py share it.  The
model takes the text from zlib (gzip.decompress) and asks bsk_find_record_start for the cut: it knows nothing of segments,
chunks, resume points, buffers or devices."""
import ctypes as C
import functools
import gzip

import gzip_ref as G
import bigseqkit_amd as bsk
from bigseqkit_amd._lib import lib, check

FA, FQ = bsk.FORMAT_FASTA, bsk.FORMAT_FASTQ


def find_record_start(window, frm, fmt):
    out = C.c_size_t()
    check(lib.bsk_find_record_start(window, len(window), frm, fmt, C.byref(out)))
    return out.value


def model(text, fmt, piece, look):
    """[(text_lo, text_hi)] by the rule: from s the window is text[s, min(s + piece + look, end)); it reaches the end: the piece
    is the rest; else the piece ends at the record start from `piece`; none in the window: look doubles"""
    out, s, n = [], 0, len(text)
    while True:
        grow = look
        while True:
            if s + piece + grow >= n:
                c = n - s
                break
            c = find_record_start(text[s:s + piece + grow], piece, fmt)
            if c < piece + grow:
                break
            grow *= 2
        out.append((s, s + c))
        s += c
        if s == n:
            return out


def fmt_of(name):
    return FA if name == "stored_false" else FQ


def sizes_of(text):
    """(piece, lookahead) for a text: five pieces or so, a lookahead that holds some records"""
    return max(1000, len(text) // 5), 2000


def settings(data, chunk):
    """the three (segment, chunk) every file is read at: 4 and 16 chunks per segment, and one segment that holds the file"""
    return [(4 * chunk, chunk), (16 * chunk, chunk), (len(data) + 4096, chunk)]


def _bytes(p):
    return bytes(p.cpu().numpy().tobytes()) if hasattr(p, "cpu") else p


def read_all(path, fmt, device, piece, look, segment, chunk, again=True):
    """([(bytes, text_lo, text_hi)], info) from GzipReader; with `again` every piece once more through .piece(), last to first,
    then the first three in order (read on without re-entry), then the sequential pass once more behind them"""
    with bsk.GzipReader(path, fmt, device=device, piece_text_bytes=piece, lookahead_bytes=look, segment_bytes=segment, chunk_bytes=chunk) as r:
        got, held = [], []
        for p, lo, hi in r:
            held.append(p)
            if len(held) >= 2:          # a piece stays readable after the next call
                assert _bytes(held[-2]) == got[-1][0], lo
            got.append((_bytes(p), lo, hi))
        info = r.info()
        if again:
            for b, lo, hi in reversed(got):
                assert _bytes(r.piece(lo, hi)) == b, (lo, hi)
            for b, lo, hi in got[:3]:
                assert _bytes(r.piece(lo, hi)) == b, (lo, hi)
    return got, info


def refusal(path, fmt, device, piece, look, segment, chunk):
    """(code, message) of the sequential pass over a file that must be refused"""
    try:
        read_all(path, fmt, device, piece, look, segment, chunk, again=False)
    except bsk.BskError as e:
        return e.code, str(e)
    return 0, ""


@functools.lru_cache(maxsize=None)
def long_member():
    """a member of three segments and more at (segment 8192, chunk 1024), then a short one: (good file, the same with the long
    member's CRC32 flipped, offset of that trailer)"""
    a, c = G.gz(G.fastq(400_000, 41), 6), G.gz(G.fastq(20_000, 42), 6)
    assert len(a) > 4 * 8192
    return a + c, a[:-8] + bytes([a[-8] ^ 1]) + a[-7:] + c, len(a) - 8


@functools.lru_cache(maxsize=None)
def far_across_segments():
    """far_32768 has no dynamic block, so no segment can end inside it.  This member has: 40 000 bytes written by zlib with a
    full flush every 3 000 -- a dynamic block starts behind every flush --, then the fixed block of far_32768 by hand: one match
    of length 258 at distance 32 768.  At a segment of two 1 KiB chunks the match reaches across a dozen segment ends, through
    a window that every one of them has carried on.  (file, text)"""
    import random
    import struct
    import zlib
    import bgzf_ref as B
    r = random.Random(9)
    head = bytes(r.choice(b"ACGTN\n") for _ in range(40_000))
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = b"".join(c.compress(head[i:i + 3000]) + c.flush(zlib.Z_FULL_FLUSH) for i in range(0, len(head), 3000))
    w = B.BitWriter()
    w.bits(1, 1); w.bits(1, 2)
    w.fixed_lit(285)
    w.code(29, 5); w.bits(8191, 13)
    w.fixed_lit(256)
    text = head + head[-32768:][:258]
    data = G.member(raw + w.done(), text)
    assert gzip.decompress(data) == text
    return data, text


SMALL = (2048, 1024)     # a segment of two 1 KiB chunks


def member_end_settings(ends):
    """(segment, chunk) that put the end of a member where the reader must get it right.  A first segment of exactly the first
    member (or the first two): its buffer ends behind the trailer while the file goes on, so the segment ends in front of the
    chain chunk that walked there, and that chunk is chunk 0 of the next segment: the member ends inside it.  Five bytes more:
    the buffer ends inside the next member's header, with the same consequence"""
    return [(ends[0], 1024), (ends[0] + 5, 1024), (ends[0], 8192), (ends[1], 1024), (ends[1] + 5, 2048)]


def member_ends(data):
    """the file offsets behind the members of a file, by zlib"""
    import zlib
    out, at = [], 0
    while at < len(data):
        d = zlib.decompressobj(31)
        d.decompress(data[at:])
        at = len(data) - len(d.unused_data)
        out.append(at)
    return out


def expected(data):
    return gzip.decompress(data) if data else b""
