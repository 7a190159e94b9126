"""The piece rule of the BGZF reader restated for the tests (PARITY.md BGZF "pieces"), the texts and the files the tests read.
Nothing here is a test; tests/test_bgzf_stream_cpu.py and tests/test_bgzf_stream_gpu.py share it.  The model walks the block
index of bgzf_ref and asks bsk_find_record_start for the cut: it knows nothing of chunks, buffers or devices."""
import ctypes as C
import gzip
import random
import struct
import zlib

import bgzf_ref as R
import bigseqkit_amd as bsk
from bigseqkit_amd._lib import lib, check

FA, FQ = bsk.FORMAT_FASTA, bsk.FORMAT_FASTQ
DECLINED = 2 ** 64 - 1


# ---- texts: (bytes, format); every FASTQ line is 7 bytes or longer, where find_fastq_cut is exact ---------------------------
def fastq4(seed, nrec, lo=8, hi=70):
    """four lines per record; qualities begin with '@' and '+' now and then"""
    r, out = random.Random(seed), []
    for i in range(nrec):
        L = r.randint(lo, hi)
        q = [chr(r.randint(35, 126)) for _ in range(L)]
        if r.random() < 0.35:
            q[0] = r.choice("@+")
        out.append("@read%d/%d x=%d\n%s\n+%s\n%s\n" % (i, 1 + i % 2, r.randrange(10 ** r.randint(1, 6)), "".join(r.choice("ACGTN") for _ in range(L)),
                                                     "read%d" % i if r.random() < 0.2 else "", "".join(q)))
    return "".join(out).encode()


def fastq_wrapped(seed, nrec, width=11):
    """bases and qualities wrapped at `width`: the strict rule does not read it, the cut comes from the host"""
    r, out = random.Random(seed), []
    for i in range(nrec):
        L = r.randint(width, 6 * width)
        if L % width < 7:
            L -= L % width          # (no last line shorter than 7 bytes)
        s = "".join(r.choice("ACGT") for _ in range(L))
        q = "".join(chr(r.randint(48, 90)) for _ in range(L))
        out.append("@wrapped%d\n%s\n+\n%s\n" % (i, "\n".join(s[k:k + width] for k in range(0, L, width)), "\n".join(q[k:k + width] for k in range(0, L, width))))
    return "".join(out).encode()


def fasta(seed, nrec, long_at=None, long_len=0):
    r, out = random.Random(seed), []
    for i in range(nrec):
        L = long_len if i == long_at else r.randint(1, 400)
        s = "".join(r.choice("ACGTN>") if k % 60 else r.choice("ACGT") for k in range(L))   # ('>' inside a line is no record start)
        out.append(">seq%d desc > %d\n" % (i, L) + "".join(s[k:k + 60] + "\n" for k in range(0, L, 60)))
    return "".join(out).encode()


def record_starts(text, fmt):
    """the record starts a sequential parse of the whole text names, and len(text)"""
    starts, at, n = [], 0, len(text)
    if fmt == FA:
        while at < n:
            if text[at:at + 1] == b">":
                starts.append(at)
            nl = text.find(b"\n", at)
            at = n if nl < 0 else nl + 1
        return set(starts) | {n}
    lines = text.split(b"\n")
    i, pos = 0, 0
    while i < len(lines) and pos < n:
        assert lines[i][:1] == b"@", (i, lines[i])
        starts.append(pos)
        pos += len(lines[i]) + 1
        i += 1
        S = 0
        while lines[i][:1] != b"+":
            S += len(lines[i]); pos += len(lines[i]) + 1; i += 1
        pos += len(lines[i]) + 1
        i += 1
        Q = 0
        while Q < S:
            Q += len(lines[i]); pos += len(lines[i]) + 1; i += 1
        assert Q == S
    return set(starts) | {n}


# ---- files ----------------------------------------------------------------------------------------------------------------------
def write_mixed(text, seed, lo=200, hi=700):
    """blocks of lo .. hi text bytes -- stored, fixed and dynamic by turns -- with an empty block now and then"""
    r, out, at, k = random.Random(seed), [], 0, 0
    kinds = (dict(level=0), dict(strategy=zlib.Z_FIXED), dict(level=6), dict(level=9))
    while at < len(text):
        t = text[at:at + r.randint(lo, hi)]
        out.append(R.member(R.deflate(t, **kinds[k % 4]), t))
        if r.random() < 0.15:
            out.append(R.member(R.deflate(b""), b""))
        at += len(t)
        k += 1
    return b"".join(out)


def block_types(data):
    """the DEFLATE block types of the file's members"""
    rep = R.inflate(data)[1]
    return rep.types


def cases():
    """name -> (file, format, piece_text_bytes, lookahead_bytes)"""
    fq, fa = fastq4(1, 260), fasta(2, 60)
    C_ = {}
    C_["fq_mixed"] = (write_mixed(fq, 11) + R.EOF_BLOCK, FQ, 1500, 700)
    C_["fa_mixed"] = (write_mixed(fa, 12) + R.EOF_BLOCK, FA, 2000, 600)
    C_["fq_small_pieces"] = (R.write(fq, block=333), FQ, 1000, 600)
    C_["fa_long_record"] = (R.write(fasta(3, 70, long_at=9, long_len=9000), block=500), FA, 1000, 500)
    half = len(fq) // 2
    half = fq.rfind(b"\n@read", 0, half) + 1
    C_["fq_cat_two_files"] = (write_mixed(fq[:half], 13) + R.EOF_BLOCK + R.member(R.deflate(b""), b"") + write_mixed(fq[half:], 14) + R.EOF_BLOCK, FQ, 1200, 600)
    C_["fa_no_eof"] = (R.write(fa, block=450, eof=False), FA, 1500, 400)
    C_["fq_no_last_newline"] = (R.write(fq[:-1], block=300), FQ, 2000, 700)
    C_["fq_wrapped"] = (R.write(fastq_wrapped(4, 120), block=400), FQ, 1500, 1200)
    C_["fa_tiny_lookahead"] = (R.write(fa, block=97), FA, 700, 1)      # (short carried heads: the cut lies just in front of E)
    C_["fq_tiny_lookahead"] = (R.write(fastq4(5, 70), block=61), FQ, 500, 1)
    C_["fq_one_piece"] = (R.write(fastq4(6, 9), block=250), FQ, 4000, 600)
    C_["empty_file"] = (b"", FQ, 1000, 500)
    C_["eof_alone"] = (R.EOF_BLOCK, FA, 1000, 500)
    C_["empty_blocks_only"] = (R.member(R.deflate(b""), b"") * 3 + R.EOF_BLOCK, FA, 1000, 500)
    return C_


def chunk_sizes(data):
    """from "one block" to "whole file" """
    return sorted({256, 1000, 4097, max(len(data), 1), len(data) + 5000})


# ---- the model ----------------------------------------------------------------------------------------------------------------
def find_record_start(window, frm, fmt):
    out = C.c_size_t()
    check(lib.bsk_find_record_start(window, len(window), frm, fmt, C.byref(out)))
    return out.value


def model(data, fmt, piece, look):
    """[(text_lo, text_hi, voff_lo, voff_hi, carry)] by the rule, and the text"""
    text = gzip.decompress(data) if data else b""
    blocks, at = [], 0                      # (file offset, text start, text end) of the blocks with text
    for off, bsize, isize, _ in R.index(data):
        if isize:
            blocks.append((off, at, at + isize))
        at += isize
    assert at == len(text)

    def voff(t):
        for off, a, b in blocks:
            if a <= t < b:
                return off << 16 | (t - a)
        assert t == len(text)
        return len(data) << 16

    out, s = [], 0
    while True:
        grow = look
        while True:
            E = next((b for _, _, b in blocks if b - s >= piece + grow), len(text))
            if E == len(text):
                c = E - s
                break
            c = find_record_start(text[s:E], piece, fmt)
            if c < E - s:
                break
            grow *= 2
        out.append((s, s + c, voff(s), voff(s + c), E - s - c))
        s += c
        if s == len(text):
            return out, text


def read_all(path, fmt, device, piece, look, chunk):
    """[(bytes, voff_lo, voff_hi)] from BgzfReader, and every piece once more through .piece(), last to first"""
    with bsk.BgzfReader(path, fmt, device=device, piece_text_bytes=piece, lookahead_bytes=look, comp_chunk_bytes=chunk) as r:
        got = [(bytes(p.cpu().numpy().tobytes()) if hasattr(p, "cpu") else p, lo, hi) for p, lo, hi in r]
        for b, lo, hi in reversed(got):
            again = r.piece(lo, hi)
            assert (bytes(again.cpu().numpy().tobytes()) if hasattr(again, "cpu") else again) == b, (lo, hi)
        for b, lo, hi in got[:3]:          # ... and in order: read on without a seek
            again = r.piece(lo, hi)
            assert (bytes(again.cpu().numpy().tobytes()) if hasattr(again, "cpu") else again) == b, (lo, hi)
    return got


def check_case(tmp_path, name, case, device):
    """the reader on one file, at every chunk size, against zlib and the model; returns the carries of its pieces"""
    data, fmt, piece, look = case
    want, text = model(data, fmt, piece, look)
    starts = record_starts(text, fmt)
    path = tmp_path / (name + ".gz")
    path.write_bytes(data)
    for chunk in chunk_sizes(data):
        got = read_all(path, fmt, device, piece, look, chunk)
        assert b"".join(b for b, _, _ in got) == text, (name, chunk)
        assert [(lo, hi) for _, lo, hi in got] == [(w[2], w[3]) for w in want], (name, chunk)
        assert [len(b) for b, _, _ in got] == [w[1] - w[0] for w in want], (name, chunk)
        at = 0
        for b, _, _ in got:
            assert at in starts, (name, chunk, at)
            at += len(b)
    return [w[4] for w in want[:-1]]


def fuzz_windows(seed, count):
    """(window, from, format): FASTA and four-line FASTQ text cut at any byte, and a few wrapped and damaged ones"""
    r = random.Random(seed)
    for k in range(count):
        kind = k % 5
        if kind == 0:
            text, fmt = fasta(r.randrange(10 ** 6), 8), FA
        elif kind == 4:
            text, fmt = fastq_wrapped(r.randrange(10 ** 6), 12, r.choice((7, 11, 30))), FQ
        else:
            text, fmt = fastq4(r.randrange(10 ** 6), 14, 1 if kind == 3 else 8, 40), FQ
        a = 0 if r.random() < 0.5 else r.randrange(len(text) // 3)
        b = len(text) if r.random() < 0.3 else r.randrange(2 * len(text) // 3, len(text))
        w = bytearray(text[a:b])
        if kind == 3 and r.random() < 0.5:     # damage: a byte changed, a line feed doubled
            at = r.randrange(len(w))
            w[at:at + 1] = r.choice((b"\n\n", b"@", b"+", b"\n@"))
        yield bytes(w), r.randrange(1, len(w)), fmt


def stream_cut(window, frm, fmt, device):
    out = C.c_uint64()
    check(lib.bsk_selftest_bgzf_stream_cut(window, len(window), frm, fmt, device, C.byref(out)))
    return out.value


def malformed_in_second_chunk():
    """name -> (file, chunk, code, block, offset, word): 24 good blocks with one thing wrong in block 17, and a chunk size that
    puts block 17 into the second chunk"""
    fq = fastq4(21, 200)
    texts = [fq[k:k + 400] for k in range(0, 24 * 400, 400)]
    members = [R.member(R.deflate(t), t) for t in texts]
    offs = [sum(map(len, members[:k])) for k in range(25)]
    k = 17
    chunk = offs[12] + 7            # (block 12 straddles the end of the first chunk; block 17 lies in the second)
    assert offs[k] > chunk and offs[k + 1] < 2 * chunk

    def with_block(m):
        return b"".join(members[:k]) + m + b"".join(members[k + 1:]) + R.EOF_BLOCK

    M = {}
    bad_crc = bytearray(members[k]); bad_crc[-8] ^= 4
    M["bad_crc"] = (with_block(bytes(bad_crc)), chunk, 3, k, offs[k], "CRC")
    M["btype3"] = (with_block(R.member(b"\x07" + bytes(8), texts[k])), chunk, 3, k, offs[k], "block type")
    whole = b"".join(members)
    M["truncated_last"] = (whole[:offs[23] + len(members[23]) // 2], chunk, 3, 23, offs[23], "truncated")
    M["plain_gzip"] = (gzip.compress(fq), chunk, 4, None, None, "bgzip")
    return M
