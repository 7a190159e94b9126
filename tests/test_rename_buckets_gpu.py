"""`rename` in buckets of the key on the GPU (PARITY.md RENB; include/bsk.h bsk_rename_hist_run .. bsk_rename_emit_run): the bytes
are those of the one-call bsk.Rename and of the oracle whatever the budget and the cut of the input into shards; the histogram
and the ordinals against the restatement in rename_buckets_ref.py; the smallest shapes, a launch of many blocks, distinct
subjects under one key, global indices past 2^32, the forms of a header; misuse; the command line."""
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
import rename_buckets_ref as N
import rmdup_buckets_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")
BINS = R.BINS


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


def run(f, o, budget):
    """the passes of bsk.RenameBuckets, step by step: (bytes, buckets, renamed, flagged, ordinals, (hist bytes, hist records))"""
    with bsk.Operator("Rename", json.dumps(o), 0) as op:
        bsk.RenameHistReset(op)
        counts = bsk.RenameHistRun(op, f)
        hist = bsk.RenameHistGet(op)
        bounds = bsk.ShufflePlan(hist[0], budget)
        total = sum(counts)
        bsk.RenameVerdictBegin(op, total)
        renamed = flagged = 0
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            r, fl = bsk.RenameBucket(op, f, counts, lo, hi)
            renamed, flagged = renamed + r, flagged + fl
        ords = bsk.RenameVerdictGet(op, 0, total)
        return bsk.RenameEmit(op, f, counts), len(bounds) - 1, renamed, flagged, ords, hist


@functools.lru_cache(maxsize=None)
def one_call(name, oj):
    data, fastq = R.shape(name)
    return bsk.Rename(frame(data, fastq), Opts(json.loads(oj)))


# ------------------------------------------------------------------ parity
CASES = [(n, o) for n in R.SHAPES for o in N.OPTION_SETS]
CASES += [(n, dict(o, LineWidth=w)) for n in ("fasta 7", "fasta 60") for w in (0, 60) for o in N.OPTION_SETS]


@pytest.mark.parametrize("name,o", CASES, ids=lambda v: v if isinstance(v, str) else ("+".join("%s" % k if x is True else "%s%s" % (k, x) for k, x in v.items()) or "id"))
def test_buckets_equal_the_one_call_and_the_oracle(name, o):
    oj = json.dumps(o)
    data, fastq = R.shape(name)
    want = N.want_of(name, oj)
    assert one_call(name, oj) == want
    recs, subs, hb, hr, ords = N.restated(name, oj)
    for budget, least in zip(R.budgets_of(hb), (1, 8, 8)):
        for parts in (1, 3, 7):
            got, nb, renamed, flagged, got_ords, hist = run(frame(data, fastq, parts), o, budget)
            assert got == want, (budget, parts, nb)
            assert nb >= least and (least > 1 or nb == 1)
            assert got_ords == ords and renamed == sum(1 for k in ords if k) and flagged == 0
            assert hist == (hb, hr)
    assert bsk.RenameBuckets(frame(data, fastq, 3), Opts(o), R.budgets_of(hb)[1]) == want


# ------------------------------------------------------------------ the smallest shapes
def pattern_ids(n, pattern):
    if pattern == "all repeat record 0":
        return [0] * n                                                             # ordinals 0 .. n - 1: suffixes of 1 to 4 digits
    if pattern == "alternating":
        return [i if i % 2 == 0 else i - 1 for i in range(n)]                    # every odd record repeats the one before it
    return list(range(n))                                                          # no repeat


@pytest.mark.parametrize("n", (1, 31, 32, 33, 2047, 2048, 2049, 4097))
def test_smallest_shapes(n):
    """the records of a block of the 8-lane kernels (32) and the tile of the scans (2048)"""
    for pattern in ("all repeat record 0", "alternating", "no repeat"):
        ids = pattern_ids(n, pattern)
        recs = [(b"r%d" % i, b"ACGT") for i in ids]
        want_ords = N.py_ordinals(ids)
        hb = R.py_hist([h for h, _ in recs])[0]
        for fastq, parts, budget in ((True, 1, 1 << 30), (False, 3, max(max(hb), sum(hb) // 4))):
            data = N.tiny_text(recs, fastq)
            got, nb, renamed, flagged, ords, hist = run(frame(data, fastq, parts), {}, budget)
            assert ords == want_ords, (pattern, fastq)
            assert renamed == sum(1 for k in want_ords if k) and flagged == 0
            if pattern == "no repeat":
                assert renamed == 0 and got == data
            assert got == N.tiny_text(N.py_rename(recs, {}), fastq), (pattern, fastq)


# ------------------------------------------------------------------ past one launch of many blocks
def test_many_blocks():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 3 * cus * 256 + 1234
    ids = [i % (n // 3) for i in range(n)]                                         # every ID three times, some four: ordinals 0 .. 3
    data = b"".join(b">%x\nA\n" % i for i in ids)
    subs = [b"%x" % i for i in ids]
    hb, hr = R.py_hist(subs)
    got, nb, renamed, flagged, ords, hist = run(frame(data, False, 1), {}, sum(hb) // 4 + 1)
    want_ords = N.py_ordinals(subs)
    assert max(want_ords) == 3 and hist == (hb, hr)
    assert nb >= 4 and ords == want_ords and flagged == 0 and renamed == n - n // 3
    assert got == oracle.rename(data, False)


# ------------------------------------------------------------------ distinct subjects under one key
def test_distinct_subjects_under_one_key_keep_their_own_ordinals(monkeypatch):
    data = N.masked_key_input()
    want = oracle.rename(data, True)
    subs = [R.subject(r, {}) for r in R.parse(data, True)]
    want_ords = N.py_ordinals(subs)
    hb, hr = R.py_hist(subs)
    plain = run(frame(data, True, 3), {}, sum(hb) // 3 + 1)
    assert plain[0] == want and plain[3] == 0 and plain[4] == want_ords
    monkeypatch.setenv("BSK_RMDUP_K1_BITS", "16")                                  # 3000 subjects under 65 536 keys: some pairs collide
    got, nb, renamed, flagged, ords, hist = run(frame(data, True, 3), {}, sum(hb) // 3 + 1)
    assert got == want and ords == want_ords == plain[4]
    assert flagged > 0 and renamed == sum(1 for k in want_ords if k)
    assert hist == (hb, hr) == plain[5] and nb == plain[1]                         # the bins come from the whole k1


# ------------------------------------------------------------------ global indices past 2^32
def test_indices_past_2_to_32():
    import torch
    free = torch.cuda.mem_get_info(0)[0]
    if free < 24 << 30:
        pytest.skip("the verdict of 2^32 + 16 records takes 17.2 GB; %d bytes are free" % free)
    ids_a, ids_b = [1, 2, 3, 1, 4, 5, 2, 6], [7, 1, 8, 6, 6, 9, 3, 10]
    recs_a, recs_b = ([(b"r%d" % i, b"ACGT") for i in ids] for ids in (ids_a, ids_b))
    a, b = N.tiny_text(recs_a, True), N.tiny_text(recs_b, True)
    first_a, first_b = (1 << 32) - 3, (1 << 32) + 5
    want_ords = N.py_ordinals(ids_a + ids_b)
    with bsk.Operator("Rename", "{}", 0) as op:
        bsk.RenameVerdictBegin(op, (1 << 32) + 16)
        check(lib.bsk_rename_bucket_begin(op.ctx, 0, BINS), op.ctx)
        for text, first in ((a, first_a), (b, first_b)):
            check(lib.bsk_rename_bucket_add(op.ctx, text, len(text), 0, bsk.FORMAT_FASTQ, 0, first, None), op.ctx)
        renamed, flagged = C.c_uint64(), C.c_uint64()
        check(lib.bsk_rename_bucket_finish(op.ctx, None, C.byref(renamed), C.byref(flagged)), op.ctx)
        assert (renamed.value, flagged.value) == (sum(1 for k in want_ords if k), 0)
        assert bsk.RenameVerdictGet(op, first_a - 5, 5 + 16 + 3) == [0] * 5 + want_ords + [0] * 3
        assert bsk.RenameVerdictGet(op, 0, 40) == [0] * 40                         # nothing wrapped round to the low indices
        outs = []
        for text, first in ((a, first_a), (b, first_b)):
            out = _lib.Out()
            check(lib.bsk_rename_emit_run(op.ctx, text, len(text), 0, bsk.FORMAT_FASTQ, 0, first, None, C.byref(out)), op.ctx)
            buf = C.create_string_buffer(max(1, out.len))
            check(lib.bsk_out_to_host(op.ctx, C.byref(out), buf, out.len), op.ctx)
            outs.append(buf.raw[:out.len])
        assert b"".join(outs) == oracle.rename(a + b, True) == N.tiny_text(N.py_rename(recs_a + recs_b, {}), True)


# ------------------------------------------------------------------ the forms of a header
def test_header_forms():
    heads = [b"id first stays", b"id\ttabbed", b"id", b"other", b"id second", b"id_1 is taken", b"id", b"other\tx", b"id_1 again"]
    recs = [(h, b"ACGTACGT") for h in heads]
    for fastq in (True, False):
        data = N.tiny_text(recs, fastq)
        want = oracle.rename(data, fastq)
        lines = want.split(b"\n")
        step = 4 if fastq else 2
        got_heads = [ln[1:] for ln in lines[0:len(lines) - 1:step]]
        assert got_heads == [b"id first stays", b"id_1 tabbed", b"id_2 ", b"other", b"id_3 second", b"id_1 is taken", b"id_4 ", b"other_1 x",
                             b"id_1_1 again"]
        assert want == N.tiny_text(N.py_rename(recs, {}), fastq)
        assert bsk.Rename(frame(data, fastq), Opts({})) == want
        hb = R.py_hist([R.subject(r, {}) for r in recs])[0]
        for budget, parts in ((sum(hb), 1), (max(hb), 3)):
            got, nb, renamed, flagged, ords, hist = run(frame(data, fastq, parts), {}, budget)
            assert got == want and ords == [0, 1, 2, 0, 3, 0, 4, 1, 1] and flagged == 0
    by_name = oracle.rename(N.tiny_text(recs, True), True, json.dumps({"ByName": True}))
    got, nb, renamed, flagged, ords, hist = run(frame(N.tiny_text(recs, True), True, 3), {"ByName": True}, 1 << 20)
    assert got == by_name and ords == [0, 0, 0, 0, 0, 0, 1, 0, 0] and b"@id_1 \n" in got


# ------------------------------------------------------------------ misuse and refusals
def test_refusals_and_misuse():
    data, fastq = R.shape("fastq")
    f = frame(data, fastq)
    (pid, ptr, n, on_dev, keep), = f.partitions()
    fmt = f.format
    err = lambda op: lib.bsk_last_error(op.ctx).decode()
    INV, UNS = _lib.BSK_ERR_INVALID_ARG, _lib.BSK_ERR_UNSUPPORTED
    k, r, fl = C.c_uint64(), C.c_uint64(), C.c_uint64()
    want = N.want_of("fastq", "{}")
    with bsk.Operator("Rename", "{}", 0) as op:
        out = _lib.Out()
        assert lib.bsk_rename_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 0, None) == INV and "bsk_rename_bucket_add: no bucket is open" in err(op)
        assert lib.bsk_rename_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)) == INV and "no bucket is open" in err(op)
        assert lib.bsk_rename_bucket_begin(op.ctx, 0, BINS) == INV and "bsk_rename_verdict_begin first" in err(op)
        assert lib.bsk_rename_emit_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(out)) == INV and "bsk_rename_verdict_begin" in err(op)
        assert lib.bsk_rename_verdict_get(op.ctx, 0, 1, (C.c_uint32 * 1)()) == INV and "no verdict" in err(op)
        assert lib.bsk_rename_bucket_begin(op.ctx, 5, 5) == INV and lib.bsk_rename_bucket_begin(op.ctx, 0, BINS + 1) == INV
        check(lib.bsk_rename_hist_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(k)), op.ctx)
        total = k.value
        bsk.RenameVerdictBegin(op, total)
        check(lib.bsk_rename_bucket_begin(op.ctx, 0, 2048), op.ctx)
        assert lib.bsk_rename_bucket_begin(op.ctx, 2048, BINS) == INV and "a bucket is open" in err(op)
        assert lib.bsk_rename_verdict_begin(op.ctx, total) == INV and "a bucket is open" in err(op)
        # an add that is refused before it runs leaves the bucket usable
        assert lib.bsk_rename_bucket_add(op.ctx, ptr, n, 0, 99, 0, 0, None) == INV and "format" in err(op)
        assert lib.bsk_rename_bucket_add(op.ctx, None, n, 0, fmt, 0, 0, None) == INV and "null shard" in err(op)
        check(lib.bsk_rename_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 0, None), op.ctx)
        check(lib.bsk_rename_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)), op.ctx)
        # half of the bins are decided: the emit names the first one that is not
        assert lib.bsk_rename_emit_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(out)) == INV and "fine bin 2048 has not been decided" in err(op)
        # the shards of a bucket arrive in input order: a first_record that goes backwards closes the bucket
        check(lib.bsk_rename_bucket_begin(op.ctx, 2048, BINS), op.ctx)
        half = R.cuts_of(data, fastq, 3)[1]
        check(lib.bsk_rename_bucket_add(op.ctx, data[:half], half, 0, fmt, 0, 100, None), op.ctx)
        assert lib.bsk_rename_bucket_add(op.ctx, data[:half], half, 0, fmt, 0, 99, None) == INV and "goes backwards" in err(op)
        assert lib.bsk_rename_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)) == INV and "no bucket is open" in err(op)
        # a shard that reaches past total_records
        check(lib.bsk_rename_bucket_begin(op.ctx, 2048, BINS), op.ctx)
        assert lib.bsk_rename_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 1, None) == INV
        assert "bsk_rename_bucket_add" in err(op) and "reach past the total_records = %d of bsk_rename_verdict_begin" % total in err(op)
        assert lib.bsk_rename_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)) == INV                       # ... has closed the bucket
        check(lib.bsk_rename_bucket_begin(op.ctx, 2048, BINS), op.ctx)                                          # (a bucket that was never finished wrote nothing)
        check(lib.bsk_rename_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 0, None), op.ctx)
        check(lib.bsk_rename_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)), op.ctx)
        assert lib.bsk_rename_emit_run(op.ctx, ptr, n, 0, fmt, 0, 1, None, C.byref(out)) == INV and "reach past" in err(op)
        check(lib.bsk_rename_emit_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(out)), op.ctx)
        buf = C.create_string_buffer(max(1, out.len))
        check(lib.bsk_out_to_host(op.ctx, C.byref(out), buf, out.len), op.ctx)
        assert buf.raw[:out.len] == want                                                                         # the context is whole after all that
        assert lib.bsk_rename_verdict_get(op.ctx, total, 1, (C.c_uint32 * 1)()) == INV and "reach past" in err(op)
        assert lib.bsk_rename_verdict_get(op.ctx, 0, 1, None) == INV and "null argument" in err(op)
        bsk.RenameVerdictBegin(op, total)                                                                       # a new verdict forgets the decided bins
        assert lib.bsk_rename_emit_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(out)) == INV and "fine bin 0 has not been decided" in err(op)
        # the one call still runs on a context that has been through the buckets
        check(lib.bsk_rename_run(op.ctx, ptr, n, 0, fmt, 0, None, C.byref(out)), op.ctx)
        buf = C.create_string_buffer(max(1, out.len))
        check(lib.bsk_out_to_host(op.ctx, C.byref(out), buf, out.len), op.ctx)
        assert buf.raw[:out.len] == want
    # a single bin above the budget: the plan's refusal
    hb = N.restated("fastq", "{}")[2]
    with pytest.raises(bsk.BskError) as e:
        bsk.RenameBuckets(f, Opts({}), max(hb) - 1)
    assert e.value.code == UNS and "holds %d bytes" % next(v for v in hb if v > max(hb) - 1) in str(e.value) and "budget of %d bytes" % (max(hb) - 1) in str(e.value)
    # out=slices on the emit is what it is on the one call: the bytes all the same
    os.environ["BSK_OUT"] = "slices"
    try:
        assert bsk.Rename(f, Opts({})) == want
        assert bsk.RenameBuckets(f, Opts({}), R.budgets_of(hb)[1]) == want
    finally:
        del os.environ["BSK_OUT"]
    # every entry point on a context of another operator, an RmDup context among them -- and rmdup's on a Rename context
    for other in ("Shuffle", "RmDup"):
        with bsk.Operator(other, "{}", 0) as op:
            out = _lib.Out()
            for rc in (lib.bsk_rename_hist_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(k)),
                       lib.bsk_rename_hist_get(op.ctx, None, None),
                       lib.bsk_rename_hist_reset(op.ctx),
                       lib.bsk_rename_verdict_begin(op.ctx, 10),
                       lib.bsk_rename_verdict_get(op.ctx, 0, 1, (C.c_uint32 * 1)()),
                       lib.bsk_rename_bucket_begin(op.ctx, 0, BINS),
                       lib.bsk_rename_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 0, None),
                       lib.bsk_rename_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)),
                       lib.bsk_rename_emit_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(out))):
                assert rc == INV and "not a Rename context" in err(op)
    with bsk.Operator("Rename", "{}", 0) as op:
        out = _lib.Out()
        for rc in (lib.bsk_rmdup_hist_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(k)),
                   lib.bsk_rmdup_hist_get(op.ctx, None, None),
                   lib.bsk_rmdup_hist_reset(op.ctx),
                   lib.bsk_rmdup_verdict_begin(op.ctx, 10),
                   lib.bsk_rmdup_verdict_get(op.ctx, 0, 1, (C.c_uint8 * 1)()),
                   lib.bsk_rmdup_bucket_begin(op.ctx, 0, BINS),
                   lib.bsk_rmdup_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 0, None),
                   lib.bsk_rmdup_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)),
                   lib.bsk_rmdup_emit_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(out))):
            assert rc == INV and "not an RmDup context" in err(op)


# ------------------------------------------------------------------ the command line
def cli(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([CLI, *args], capture_output=True, timeout=900, env=e)
    assert p.returncode == 0, p.stderr.decode()
    return p


def test_cli_rename_in_buckets(tmp_path):
    """two FASTA files, the first one without its final newline, unioned in order; a FASTQ file"""
    fq = R.shape("fastq")[0]
    a, b = R.shape("fasta 60")[0][:-1], R.shape("fasta 7")[0]
    ffq, fa, fb = (str(tmp_path / x) for x in ("r.fq", "a.fa", "b.fa"))
    for path, text in ((ffq, fq), (fa, a), (fb, b)):
        open(path, "wb").write(text)
    out = str(tmp_path / "o")
    streamed = {"BSK_STREAM_PIECE_BYTES": "9000", "BSK_STAGE_BYTES": "4096"}
    for files, union, fastq in (([fa, fb], a + b"\n" + b, False), ([ffq], fq, True)):
        for flags in ([], ["-n"]):
            o = {"ByName": "-n" in flags}
            args = ["rename", *files, "-o", out, "--merge", *flags]
            want = oracle.rename(union, fastq, json.dumps(o))
            subs = [R.subject(r, o) for r in R.parse(union, fastq)]
            hb = R.py_hist(subs)[0]
            streamed["BSK_RENAME_BUDGET_BYTES"] = str(max(max(hb), sum(hb) // 6))             # six buckets or so, and the fullest bin fits
            p = cli(args, {"BSK_CLI_TIMING": "1"})
            assert open(out, "rb").read() == want and "k_rdb_hist" not in p.stderr.decode()      # the whole-file run, as before
            os.remove(out)
            p = cli(args, dict(streamed, BSK_CLI_TIMING="1"))
            assert open(out, "rb").read() == want, (files, flags)
            err = p.stderr.decode()
            assert all(s in err for s in ("k_rdb_hist", "k_rdb_pick", "k_rdb_pack", "k_renb_verify", "k_renb_scatter")), err[-800:]
            assert int(err.split("rename in ")[1].split(" bucket")[0]) >= 3 and int(err.split(" bytes, ")[1].split(" piece")[0]) >= 3
            assert "rename: %d record(s) renamed, 0 flagged" % sum(1 for k in N.py_ordinals(subs) if k) in err
            os.remove(out)
    # a single bin above the budget ends with the plan's message
    p = subprocess.run([CLI, "rename", ffq, "-o", out], capture_output=True, timeout=900, env=dict(os.environ, BSK_RENAME_BUDGET_BYTES="20"))
    assert p.returncode != 0 and "more than the budget of 20 bytes" in p.stderr.decode() and "rename: a fine bin" in p.stderr.decode()
    # an input that cannot be loaded whole is told about the switch, not about --devices, and with it goes through the buckets
    p = subprocess.run([CLI, "rename", ffq, "-o", out], capture_output=True, timeout=900, env=dict(os.environ, BSK_SHARD_FAIL_ALLOC="1"))
    assert p.returncode != 0 and "BSK_RENAME_BUDGET_BYTES" in p.stderr.decode() and "--devices" not in p.stderr.decode()
    p = cli(["rename", ffq, "-o", out, "--merge"], {"BSK_RENAME_BUDGET_BYTES": str(1 << 30), "BSK_SHARD_FAIL_ALLOC": "1", "BSK_CLI_TIMING": "1"})
    assert open(out, "rb").read() == N.want_of("fastq", "{}") and "rename in 1 bucket(s)" in p.stderr.decode()
