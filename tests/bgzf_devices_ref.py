"""Where `world` workers cut a BGZF file, restated for the tests (PARITY.md BGZF "workers"), and the files these tests read.
Nothing here is a test; tests/test_bgzf_devices_cpu.py and tests/test_bgzf_devices_gpu.py share it.  The model walks the whole
block chain (bgzf_ref.index) and parses the whole text (bgzf_stream_ref.record_starts): it knows nothing of candidates, windows
or devices, and it never asks the library for a cut."""
import gzip
import random

import bgzf_ref as R
import bgzf_stream_ref as S

FA, FQ = S.FA, S.FQ
WORLDS = (1, 2, 3, 7)


def layout(data):
    """(blocks, text): blocks = [(file offset, text start, ISIZE)] of the chain from 0"""
    text = gzip.decompress(data) if data else b""
    blocks, at = [], 0
    for off, bsize, isize, _ in R.index(data):
        blocks.append((off, at, isize))
        at += isize
    assert at == len(text)
    return blocks, text


def voff_of(blocks, size, t):
    """the normalised virtual offset of text position t: in the block that holds the byte, never at a block's end"""
    for off, a, isize in blocks:
        if a <= t < a + isize:
            return off << 16 | (t - a)
    return size << 16


def text_of(blocks, size, n_text, v):
    """the text position of a virtual offset"""
    if v == size << 16:
        return n_text
    for off, a, isize in blocks:
        if off == v >> 16:
            assert (v & 0xFFFF) < isize, v
            return a + (v & 0xFFFF)
    raise AssertionError("%d is not on the block chain" % (v >> 16))


def model(data, fmt, world):
    """(block cuts B_0 .. B_world-1, record cuts V_0 .. V_world, their text positions T) by the definitions"""
    blocks, text = layout(data)
    size = len(data)
    starts = sorted(S.record_starts(text, fmt))
    B, T = [0], [0]
    for k in range(1, world):
        lo = max(size * k // world, B[-1])
        b = next(((off, a) for off, a, _ in blocks if off >= lo), (size, len(text)))
        B.append(b[0])
        T.append(next(s for s in starts if s >= b[1]))
    T.append(len(text))
    return B, [voff_of(blocks, size, t) for t in T[:-1]] + [size << 16], T


def cases():
    """the files of bgzf_stream_ref, without the wrapped FASTQ (its widths are chosen where it is used)"""
    return {k: (v[0], v[1]) for k, v in S.cases().items() if k != "fq_wrapped"}


def worlds_of(data):
    return WORLDS + (len(R.index(data)) + 2,)


# ---- a block whose data holds a whole BGZF block ---------------------------------------------------------------------------------
def nested_member():
    """(file, format, offset of the inner member in the file, the true block start behind it).  FASTA: one header line holds the
    bytes of a complete small BGZF member that has no line feed in it; the record lies in a stored block, and the records behind
    it are chosen so that floor(size / 2) falls between that block's start and the inner member"""
    inner = None
    for seed in range(200):
        r = random.Random(seed)
        t = b">x0\n" + bytes(r.choice(b"ACGT") for _ in range(40)) + b"\n"
        m = R.member(R.deflate(t, level=6), t)
        if b"\n" not in m and b"\r" not in m:
            inner = m
            break
    assert inner is not None and gzip.decompress(inner) == t
    head = S.fasta(31, 6)
    carrier = b">carrier " + inner + b" end\nACGTACGTAC\n"
    pre = [R.member(R.deflate(head[i:i + 300]), head[i:i + 300]) for i in range(0, len(head), 300)]
    # the stored block: some records, the carrier in its second half
    lead = S.fasta(32, 1)
    stored_text = lead + carrier + S.fasta(33, 1)
    stored = R.member(R.deflate(stored_text, level=0), stored_text)
    front = b"".join(pre)
    at_stored = len(front)
    at_inner = at_stored + stored.index(inner)
    # the tail is grown until size // 2 falls into (at_stored, at_inner]
    for nrec in range(1, 400):
        tail_text = S.fasta(34, nrec)
        tail = b"".join(R.member(R.deflate(tail_text[i:i + 350]), tail_text[i:i + 350]) for i in range(0, len(tail_text), 350)) + R.EOF_BLOCK
        data = front + stored + tail
        if at_stored < len(data) // 2 <= at_inner:
            assert gzip.decompress(data[at_inner:at_inner + len(inner)]) == t
            return data, FA, at_inner, at_stored + len(stored)
    raise AssertionError("no tail puts the nominal cut in front of the inner member")


def with_duplicates(seed=41, nrec=120):
    """four-line FASTQ whose sequences repeat across the whole file: every cut has copies of a sequence on both sides"""
    r, out = random.Random(seed), []
    pool = ["".join(r.choice("ACGT") for _ in range(r.randint(20, 50))) for _ in range(25)]
    for i in range(nrec):
        s = pool[r.randrange(len(pool))] if r.random() < 0.7 else "".join(r.choice("ACGT") for _ in range(r.randint(20, 50)))
        out.append("@dup%d\n%s\n+\n%s\n" % (i, s, "".join(chr(r.randint(48, 90)) for _ in s)))
    return "".join(out).encode()
