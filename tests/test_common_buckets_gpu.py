"""`common` in buckets of the key on the GPU (PARITY.md COMB; include/bsk.h bsk_common_hist_run .. bsk_common_emit_run): the bytes
are those of the one-call bsk.Common and of the oracle whatever the budget, the number of files and the cut of the files into
shards; the histogram and the keep bits against the restatement in common_buckets_ref.py; the smallest shapes, the lanes of the
comparison, 64 files, a launch of many blocks, distinct subjects under one key, global indices past 2^32; misuse; the command
line."""
import ctypes as C
import functools
import json
import os
import subprocess

import pytest

import bigseqkit_amd as bsk
from bigseqkit_amd import _lib
from bigseqkit_amd._lib import lib, check
import oracle
import common_buckets_ref as M
import rmdup_buckets_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")
BINS = R.BINS
IDS = lambda o: "+".join(k if v is True else "w%d" % v["LineWidth"] for k, v in o.items()) or "id"


class Opts:
    def __init__(self, d):
        self.d = dict(d)

    def to_json(self):
        return json.dumps(self.d)


def frame(data, fastq, parts=1):
    """`data` as 1, 3 or 7 shards that begin on record starts (7: a one-record shard and an empty one among them)"""
    fmt = bsk.FORMAT_FASTQ if fastq else bsk.FORMAT_FASTA
    cuts = R.cuts_of(data, fastq, parts)
    return bsk.SeqFrame(fmt, [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])])


def frames(texts, fastq, parts=1):
    return [frame(t, fastq, parts) for t in texts]


def dev(data):
    import torch
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8) if len(data) else torch.empty(0, dtype=torch.uint8)
    return t.cuda()


def one_call_of(texts, fastq, o):
    fmt = bsk.FORMAT_FASTQ if fastq else bsk.FORMAT_FASTA
    fs = [bsk.SeqFrame(fmt, [dev(t)]) for t in texts]
    return bsk.Common(fs[0], fs[1], Opts(o), *fs[2:])


def buckets_of(fs, o, budget):
    return bsk.CommonBuckets(fs[0], fs[1], Opts(o), *fs[2:], budget_bytes=budget)


def run(fs, o, budget):
    """the passes of bsk.CommonBuckets, step by step: (bytes, buckets, kept, flagged, keep bits of file 1, (hist bytes, hist records))"""
    with bsk.Operator("Common", json.dumps(o), 0) as op:
        bsk.CommonHistReset(op)
        counts = bsk.CommonHistRun(op, fs)
        hist = bsk.CommonHistGet(op)
        bounds = bsk.ShufflePlan(hist[0], budget)
        file_records = [sum(c) for c in counts]
        bsk.CommonVerdictBegin(op, file_records)
        kept = flagged = 0
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            k, fl = bsk.CommonBucket(op, fs, counts, lo, hi)
            kept, flagged = kept + k, flagged + fl
        bits = bsk.CommonVerdictGet(op, 0, file_records[0])
        return bsk.CommonEmit(op, fs[0], counts[0]), len(bounds) - 1, kept, flagged, bits, hist


@functools.lru_cache(maxsize=None)
def one_call(name, nfiles, oj):
    texts, fastq = M.files_text(name, nfiles)
    return one_call_of(texts, fastq, json.loads(oj))


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", R.SHAPES)
@pytest.mark.parametrize("o", M.OPTION_SETS, ids=IDS)
def test_buckets_equal_the_one_call_and_the_oracle(name, o):
    oj = json.dumps(o)
    for nfiles, all_parts, budgets in ((2, (1, 3, 7), slice(0, 3)), (3, (3,), slice(1, 2))):   # (three files: the 8-bucket budget)
        texts, fastq = M.files_text(name, nfiles)
        want = M.want_of(name, nfiles, oj)
        assert one_call(name, nfiles, oj) == want
        recs, subs, hb, hr, bits, file_records = M.restated(name, nfiles, oj)
        for budget, least in list(zip(R.budgets_of(hb), (1, 8, 8)))[budgets]:
            for parts in all_parts:
                got, nb, kept, flagged, got_bits, hist = run(frames(texts, fastq, parts), o, budget)
                assert got == want, (nfiles, budget, parts, nb)
                assert nb >= least and (least > 1 or nb == 1)
                assert got_bits == bits and kept == sum(bits) and flagged == 0
                assert hist == (hb, hr)
        assert buckets_of(frames(texts, fastq, 3), o, R.budgets_of(hb)[1]) == want
        if o == {"BySeq": True}:                                                     # -s -P is accepted and means -s
            assert buckets_of(frames(texts, fastq, 3), dict(o, OnlyPositiveStrand=True), R.budgets_of(hb)[1]) == want


# ------------------------------------------------------------------ the smallest shapes
def pattern_files(n, pattern):
    """the IDs of two files of n records (the second may hold fewer)"""
    if pattern == "file 2 equals file 1":
        return list(range(n)), list(range(n))
    if pattern == "file 2 holds every other ID":
        return list(range(n)), list(range(0, n, 2))
    return [0] * n, [0] * n                                                        # one ID everywhere: the result is one record


@pytest.mark.parametrize("n", (1, 31, 32, 33, 2047, 2048, 2049, 4097))
def test_smallest_shapes(n):
    """the records of a block of the 8-lane kernel (32), the bits of a word of the verdict (32) and the tile of the scans (2048)"""
    for pattern in ("file 2 equals file 1", "file 2 holds every other ID", "one ID everywhere"):
        files = [[(b"r%d" % i, b"ACGT") for i in ids] for ids in pattern_files(n, pattern)]
        subs = [h for f in files for h, _ in f]
        want_bits = M.py_bits(subs, [len(f) for f in files])
        hb = R.py_hist(subs)[0]
        for fastq, parts, budget in ((True, 1, 1 << 30), (False, 3, max(max(hb), sum(hb) // 4))):
            texts = [M.tiny_text(f, fastq) for f in files]
            got, nb, kept, flagged, bits, hist = run(frames(texts, fastq, parts), {}, budget)
            assert bits == want_bits, (pattern, fastq)
            assert kept == sum(want_bits) and flagged == 0
            assert got == M.tiny_text(M.py_common(files, {}), fastq) == oracle.common(texts, fastq), (pattern, fastq)
            if pattern == "file 2 equals file 1":
                assert got == texts[0]
            if pattern == "one ID everywhere":
                assert kept == 1 and got == M.tiny_text(files[0][:1], fastq)


# ------------------------------------------------------------------ the lanes of the comparison
def test_comparison_lanes(monkeypatch):
    """sequences of 0 .. 257 bytes under BySeq: 16 bytes per lane and step, 8 lanes, the bytes behind the last whole 16"""
    o = {"BySeq": True}
    lengths = M.LANE_LENGTHS
    a = [(b"a%d" % L, M.lane_sequence(L, L, b"A")) for L in lengths]
    same = [(b"b%d" % L, s) for (h, s), L in zip(a, lengths)]
    last = [(b"b%d" % L, M.lane_sequence(L, L, b"C")) for L in lengths]             # (the empty sequence has no last byte: equal)
    for other, want_bits in ((same, [1] * len(lengths)), (last, [1] + [0] * (len(lengths) - 1))):
        texts = [R.fasta_text(a, 1000), R.fasta_text(other, 1000)]
        got, nb, kept, flagged, bits, hist = run(frames(texts, False), o, 1 << 30)
        assert list(bits) == want_bits and kept == sum(want_bits) and flagged == 0   # a last byte that differs is another key
        assert got == oracle.common(texts, False, json.dumps(o)) == one_call_of(texts, False, o)
    # under 16 bits of the key a pair that differs in its last byte only shares a key group: the comparison tells it apart
    pairs = [M.last_byte_collision(L) for L in lengths if L >= 2]
    a = [(b"a0", b""), (b"a1", b"G")] + [(b"a%d" % len(s), s) for s, t in pairs]
    b = [(b"b0", b""), (b"b1", b"G")] + [(b"b%d" % len(t), t) for s, t in pairs]
    texts = [R.fasta_text(a, 1000), R.fasta_text(b, 1000)]
    want = oracle.common(texts, False, json.dumps(o))
    assert R.parse(want, False) == a[:2]
    monkeypatch.setenv("BSK_RMDUP_K1_BITS", "16")
    got, nb, kept, flagged, bits, hist = run(frames(texts, False), o, 1 << 30)
    assert nb == 1 and flagged == len(pairs) == 9                                    # every t differs from the s in front of it
    assert list(bits) == [1, 1] + [0] * len(pairs) and kept == 2 and got == want


# ------------------------------------------------------------------ the number of files
def test_number_of_files():
    one = lambda h: M.tiny_text([(h, b"ACGT")], True)
    files = [one(b"same desc %d" % f) for f in range(64)]
    fs = frames(files, True)
    assert buckets_of(fs, {}, 1 << 20) == files[0] == oracle.common(files, True)
    got, nb, kept, flagged, bits, hist = run(fs, {}, 1 << 20)
    assert (got, kept, bits) == (files[0], 1, b"\x01")
    for changed in (63, 1):                                                         # (63: the highest bit of the mask)
        other = list(files)
        other[changed] = one(b"other")
        assert oracle.common(other, True) == b""
        got, nb, kept, flagged, bits, hist = run(frames(other, True), {}, 1 << 20)
        assert (got, kept, bits) == (b"", 0, b"\x00")
    INV = _lib.BSK_ERR_INVALID_ARG
    with pytest.raises(bsk.BskError) as e:
        buckets_of(frames(files + [files[0]], True), {}, 1 << 20)                   # 65 files
    assert e.value.code == INV and "65 files" in str(e.value)
    with bsk.Operator("Common", "{}", 0) as op:
        arr = (C.c_uint64 * 65)(*([1] * 65))
        for n_files in (0, 1, 65):
            assert lib.bsk_common_verdict_begin(op.ctx, arr, n_files) == INV and "2 .. 64 files" in lib.bsk_last_error(op.ctx).decode()
        assert lib.bsk_common_verdict_begin(op.ctx, None, 2) == INV and "null argument" in lib.bsk_last_error(op.ctx).decode()
    # an empty file: an empty result and no error
    a, b, c = (M.tiny_text([(b"r%d" % i, b"ACGT") for i in range(40)], True) for _ in range(3))
    for texts in ([a, b"", c], [b"", b, c], [a, b, b""]):
        assert buckets_of(frames(texts, True), {}, 1 << 20) == b""
        assert run(frames(texts, True), {}, 1 << 20)[:4] == (b"", 1, 0, 0)
    fmt = bsk.FORMAT_FASTQ
    assert bsk.CommonBuckets(bsk.SeqFrame(fmt, []), bsk.SeqFrame(fmt, [b])) == b""  # (a frame without a shard)
    with pytest.raises(ValueError):
        bsk.CommonBuckets(bsk.SeqFrame(fmt, [a]), bsk.SeqFrame(bsk.FORMAT_FASTA, [b">x\nA\n"]))


# ------------------------------------------------------------------ past one launch of many blocks
def test_many_blocks():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 3 * cus * 256 + 1234
    a = b"".join(b">%x\nA\n" % i for i in range(n))
    b = b"".join(b">%x\nA\n" % i for i in range(0, n, 3))
    subs = [b"%x" % i for i in range(n)] + [b"%x" % i for i in range(0, n, 3)]
    hb, hr = R.py_hist(subs)
    got, nb, kept, flagged, bits, hist = run(frames([a, b], False), {}, sum(hb) // 4 + 1)
    assert hist == (hb, hr) and nb >= 4 and flagged == 0
    assert kept == (n + 2) // 3 and bits == bytes(1 if i % 3 == 0 else 0 for i in range(n))
    assert got == oracle.common([a, b], False)


# ------------------------------------------------------------------ distinct subjects under one key
def test_distinct_subjects_under_one_key_are_kept_apart(monkeypatch):
    files = M.masked_key_files()
    texts = [M.tiny_text(f, True) for f in files]
    want = oracle.common(texts, True)
    subs = [h for f in files for h, _ in f]
    want_bits = M.py_bits(subs, [3000, 3000])
    hb, hr = R.py_hist(subs)
    plain = run(frames(texts, True, 3), {}, sum(hb) // 3 + 1)
    assert plain[0] == want and plain[3] == 0 and plain[4] == want_bits and plain[2] == 1500
    monkeypatch.setenv("BSK_RMDUP_K1_BITS", "16")                                  # 4500 subjects under 65 536 keys: some pairs collide
    got, nb, kept, flagged, bits, hist = run(frames(texts, True, 3), {}, sum(hb) // 3 + 1)
    assert got == want and bits == want_bits == plain[4]
    assert flagged > 0 and kept == 1500
    assert hist == (hb, hr) == plain[5] and nb == plain[1]                         # the bins come from the whole k1


# ------------------------------------------------------------------ global indices past 2^32
def test_indices_past_2_to_32():
    """the verdict of 2^32 + 8 records of file 1 takes 512 MB"""
    ids_a, ids_b = [1, 2, 3, 1, 4, 5, 2, 6], [7, 1, 8, 6, 6, 9, 3, 10]
    recs_a, recs_b = ([(b"r%d" % i, b"ACGT") for i in ids] for ids in (ids_a, ids_b))
    a, b = M.tiny_text(recs_a, True), M.tiny_text(recs_b, True)
    first_a, first_b = (1 << 32) - 3, (1 << 32) + 8
    want_bits = [1, 0, 1, 0, 0, 0, 0, 1]
    assert list(M.py_bits(ids_a + ids_b, [8, 8])) == want_bits
    with bsk.Operator("Common", "{}", 0) as op:
        bsk.CommonVerdictBegin(op, [(1 << 32) + 8, 8])
        check(lib.bsk_common_bucket_begin(op.ctx, 0, BINS), op.ctx)
        for text, first in ((a, first_a), (b, first_b)):
            check(lib.bsk_common_bucket_add(op.ctx, text, len(text), 0, bsk.FORMAT_FASTQ, 0, first, None), op.ctx)
        kept, flagged = C.c_uint64(), C.c_uint64()
        check(lib.bsk_common_bucket_finish(op.ctx, None, C.byref(kept), C.byref(flagged)), op.ctx)
        assert (kept.value, flagged.value) == (3, 0)
        assert list(bsk.CommonVerdictGet(op, first_a - 5, 5 + 8 + 3)) == [0] * 5 + want_bits + [0] * 3
        assert bsk.CommonVerdictGet(op, 0, 40) == bytes(40)                        # nothing wrapped round to the low indices
        out = _lib.Out()
        check(lib.bsk_common_emit_run(op.ctx, a, len(a), 0, bsk.FORMAT_FASTQ, 0, first_a, None, C.byref(out)), op.ctx)
        buf = C.create_string_buffer(max(1, out.len))
        check(lib.bsk_out_to_host(op.ctx, C.byref(out), buf, out.len), op.ctx)
        assert buf.raw[:out.len] == oracle.common([a, b], True) == M.tiny_text([recs_a[0], recs_a[2], recs_a[7]], True)


# ------------------------------------------------------------------ misuse and refusals
def test_refusals_and_misuse():
    texts, fastq = M.files_text("fastq", 2)
    fs = frames(texts, fastq)
    (pid, ptr, n, on_dev, keep), = fs[0].partitions()
    (pid2, ptr2, n2, on_dev2, keep2), = fs[1].partitions()
    fmt = fs[0].format
    err = lambda op: lib.bsk_last_error(op.ctx).decode()
    INV, UNS = _lib.BSK_ERR_INVALID_ARG, _lib.BSK_ERR_UNSUPPORTED
    k, r, fl = C.c_uint64(), C.c_uint64(), C.c_uint64()
    want = M.want_of("fastq", 2, "{}")

    def emit_bytes(op, out):
        buf = C.create_string_buffer(max(1, out.len))
        check(lib.bsk_out_to_host(op.ctx, C.byref(out), buf, out.len), op.ctx)
        return buf.raw[:out.len]

    with bsk.Operator("Common", "{}", 0) as op:
        out = _lib.Out()
        assert lib.bsk_common_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 0, None) == INV and "bsk_common_bucket_add: no bucket is open" in err(op)
        assert lib.bsk_common_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)) == INV and "no bucket is open" in err(op)
        assert lib.bsk_common_bucket_begin(op.ctx, 0, BINS) == INV and "bsk_common_verdict_begin first" in err(op)
        assert lib.bsk_common_emit_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(out)) == INV and "bsk_common_verdict_begin" in err(op)
        assert lib.bsk_common_verdict_get(op.ctx, 0, 1, (C.c_uint8 * 1)()) == INV and "no verdict" in err(op)
        assert lib.bsk_common_bucket_begin(op.ctx, 5, 5) == INV and lib.bsk_common_bucket_begin(op.ctx, 0, BINS + 1) == INV
        check(lib.bsk_common_hist_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(k)), op.ctx)
        n_a = k.value
        check(lib.bsk_common_hist_run(op.ctx, ptr2, n2, 0, fmt, 1, n_a, None, C.byref(k)), op.ctx)
        n_b = k.value
        assert (n_a, n_b) == (500, 500)
        bsk.CommonVerdictBegin(op, [n_a, n_b])
        check(lib.bsk_common_bucket_begin(op.ctx, 0, 2048), op.ctx)
        assert lib.bsk_common_bucket_begin(op.ctx, 2048, BINS) == INV and "a bucket is open" in err(op)
        assert lib.bsk_common_verdict_begin(op.ctx, (C.c_uint64 * 2)(n_a, n_b), 2) == INV and "a bucket is open" in err(op)
        # an add that is refused before it runs leaves the bucket usable
        assert lib.bsk_common_bucket_add(op.ctx, ptr, n, 0, 99, 0, 0, None) == INV and "format" in err(op)
        assert lib.bsk_common_bucket_add(op.ctx, None, n, 0, fmt, 0, 0, None) == INV and "null shard" in err(op)
        check(lib.bsk_common_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 0, None), op.ctx)
        check(lib.bsk_common_bucket_add(op.ctx, ptr2, n2, 0, fmt, 1, n_a, None), op.ctx)
        check(lib.bsk_common_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)), op.ctx)
        # half of the bins are decided: the emit names the first one that is not
        assert lib.bsk_common_emit_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(out)) == INV and "fine bin 2048 has not been decided" in err(op)
        # the shards of a bucket arrive in input order: a first_record that goes backwards closes the bucket
        check(lib.bsk_common_bucket_begin(op.ctx, 2048, BINS), op.ctx)
        half = R.cuts_of(texts[0], fastq, 3)[1]
        check(lib.bsk_common_bucket_add(op.ctx, texts[0][:half], half, 0, fmt, 0, 100, None), op.ctx)
        assert lib.bsk_common_bucket_add(op.ctx, texts[0][:half], half, 0, fmt, 0, 99, None) == INV and "goes backwards" in err(op)
        assert lib.bsk_common_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)) == INV and "no bucket is open" in err(op)
        # a shard that reaches past the sum of file_records
        check(lib.bsk_common_bucket_begin(op.ctx, 2048, BINS), op.ctx)
        assert lib.bsk_common_bucket_add(op.ctx, ptr2, n2, 0, fmt, 0, n_a + 1, None) == INV
        assert "bsk_common_bucket_add" in err(op) and "reach past the total_records = %d of bsk_common_verdict_begin" % (n_a + n_b) in err(op)
        assert lib.bsk_common_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)) == INV                       # ... has closed the bucket
        check(lib.bsk_common_bucket_begin(op.ctx, 2048, BINS), op.ctx)                                          # (a bucket that was never finished wrote nothing)
        check(lib.bsk_common_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 0, None), op.ctx)
        check(lib.bsk_common_bucket_add(op.ctx, ptr2, n2, 0, fmt, 1, n_a, None), op.ctx)
        check(lib.bsk_common_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)), op.ctx)
        # the emit runs over the first file: a shard that reaches past file_records[0]
        assert lib.bsk_common_emit_run(op.ctx, ptr, n, 0, fmt, 0, 1, None, C.byref(out)) == INV and "reach past the file_records[0] = 500" in err(op)
        assert lib.bsk_common_emit_run(op.ctx, ptr2, n2, 0, fmt, 0, n_a, None, C.byref(out)) == INV and "reach past" in err(op)
        check(lib.bsk_common_emit_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(out)), op.ctx)
        assert emit_bytes(op, out) == want                                                                       # the context is whole after all that
        assert bsk.CommonVerdictGet(op, 0, n_a) == M.restated("fastq", 2, "{}")[4]
        assert lib.bsk_common_verdict_get(op.ctx, n_a, 1, (C.c_uint8 * 1)()) == INV and "reach past" in err(op)
        assert lib.bsk_common_verdict_get(op.ctx, 0, 1, None) == INV and "null argument" in err(op)
        bsk.CommonVerdictBegin(op, [n_a, n_b])                                                                  # a new verdict forgets the decided bins
        assert lib.bsk_common_emit_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(out)) == INV and "fine bin 0 has not been decided" in err(op)
        # the one call still runs on a context that has been through the buckets
        both = texts[0] + texts[1]
        ends = (C.c_uint64 * 2)(len(texts[0]), len(both))
        check(lib.bsk_common_run(op.ctx, both, len(both), ends, 2, 0, fmt, None, C.byref(out)), op.ctx)
        assert emit_bytes(op, out) == want
    # a single bin above the budget: the plan's refusal
    hb = M.restated("fastq", 2, "{}")[2]
    with pytest.raises(bsk.BskError) as e:
        buckets_of(fs, {}, max(hb) - 1)
    assert e.value.code == UNS and "holds %d bytes" % next(v for v in hb if v > max(hb) - 1) in str(e.value) and "budget of %d bytes" % (max(hb) - 1) in str(e.value)
    # out=slices on the emit is refused; the one call is what it was
    os.environ["BSK_OUT"] = "slices"
    try:
        assert one_call_of(texts, fastq, {}) == want
        with pytest.raises(bsk.BskError) as e:
            buckets_of(fs, {}, R.budgets_of(hb)[1])
        assert e.value.code == UNS and "bsk_common_emit_run: out=slices" in str(e.value)
    finally:
        del os.environ["BSK_OUT"]
    # every entry point on a context of another operator -- and rmdup's and rename's on a Common context
    arr = (C.c_uint64 * 2)(10, 10)
    for other in ("Shuffle", "RmDup", "Rename"):
        with bsk.Operator(other, "{}", 0) as op:
            out = _lib.Out()
            for rc in (lib.bsk_common_hist_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(k)),
                       lib.bsk_common_hist_get(op.ctx, None, None),
                       lib.bsk_common_hist_reset(op.ctx),
                       lib.bsk_common_verdict_begin(op.ctx, arr, 2),
                       lib.bsk_common_verdict_get(op.ctx, 0, 1, (C.c_uint8 * 1)()),
                       lib.bsk_common_bucket_begin(op.ctx, 0, BINS),
                       lib.bsk_common_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 0, None),
                       lib.bsk_common_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)),
                       lib.bsk_common_emit_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(out))):
                assert rc == INV and "not a Common context" in err(op)
    with bsk.Operator("Common", "{}", 0) as op:
        out = _lib.Out()
        for prefix, message, word in (("bsk_rmdup", "not an RmDup context", C.c_uint8), ("bsk_rename", "not a Rename context", C.c_uint32)):
            fn = lambda name: getattr(lib, prefix + "_" + name)
            for rc in (fn("hist_run")(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(k)),
                       fn("hist_get")(op.ctx, None, None),
                       fn("hist_reset")(op.ctx),
                       fn("verdict_begin")(op.ctx, 10),
                       fn("verdict_get")(op.ctx, 0, 1, (word * 1)()),
                       fn("bucket_begin")(op.ctx, 0, BINS),
                       fn("bucket_add")(op.ctx, ptr, n, 0, fmt, 0, 0, None),
                       fn("bucket_finish")(op.ctx, None, C.byref(r), C.byref(fl)),
                       fn("emit_run")(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(out))):
                assert rc == INV and message in err(op)


# ------------------------------------------------------------------ the command line
def test_cli_common_in_buckets(tmp_path):
    """three FASTA files, the second one without its final newline"""
    texts, fastq = M.files_text("fasta 60", 3)
    paths = [str(tmp_path / x) for x in ("a.fa", "b.fa", "c.fa")]
    for path, text in zip(paths, (texts[0], texts[1][:-1], texts[2])):
        open(path, "wb").write(text)
    for flags, o in (([], {}), (["-s", "-i"], {"BySeq": True, "IgnoreCase": True})):
        want = oracle.common(list(texts), fastq, json.dumps(o))
        recs, subs, hb, hr, bits, file_records = M.restated("fasta 60", 3, json.dumps(o))
        args = [CLI, "common", *paths, "-o", "-", *flags]
        p = subprocess.run(args, capture_output=True, timeout=900, env=dict(os.environ, BSK_CLI_TIMING="1"))
        assert p.returncode == 0, p.stderr.decode()
        assert p.stdout == want and "k_rdb_hist" not in p.stderr.decode()            # the whole-file run, as before
        env = dict(os.environ, BSK_CLI_TIMING="1", BSK_STREAM_PIECE_BYTES="4096", BSK_COMMON_BUDGET_BYTES=str(max(max(hb), sum(hb) // 6)))
        p = subprocess.run(args, capture_output=True, timeout=900, env=env)
        assert p.returncode == 0, p.stderr.decode()
        assert p.stdout == want, flags
        err = p.stderr.decode()
        assert all(s in err for s in ("k_rdb_hist", "k_rdb_pick", "k_rdb_pack", "k_comb_verify", "k_comb_decide", "k_comb_apply")), err[-800:]
        assert int(err.split("common in ")[1].split(" bucket")[0]) >= 4 and int(err.split(" bytes, ")[1].split(" piece")[0]) >= 9
        assert "common: %d record(s) kept, 0 flagged" % sum(bits) in err
    # a single bin above the budget ends with the plan's message
    p = subprocess.run([CLI, "common", *paths, "-o", "-"], capture_output=True, timeout=900, env=dict(os.environ, BSK_COMMON_BUDGET_BYTES="20"))
    assert p.returncode != 0 and "more than the budget of 20 bytes" in p.stderr.decode() and "common: a fine bin" in p.stderr.decode()
    # two formats, and one file, are refused as on the whole-file path
    fq = str(tmp_path / "r.fq")
    open(fq, "wb").write(M.files_text("fastq", 2)[0][0])
    for env in ({}, {"BSK_COMMON_BUDGET_BYTES": "20000"}):
        p = subprocess.run([CLI, "common", paths[0], fq, "-o", "-"], capture_output=True, timeout=900, env=dict(os.environ, **env))
        assert p.returncode != 0 and "common: inputs of different formats" in p.stderr.decode()
        p = subprocess.run([CLI, "common", paths[0], "-o", "-"], capture_output=True, timeout=900, env=dict(os.environ, **env))
        assert p.returncode != 0 and "at least 2 files needed" in p.stderr.decode()
