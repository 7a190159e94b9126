"""`rmdup` in buckets of the key on the GPU (PARITY.md RMDUPB; include/bsk.h bsk_rmdup_hist_run .. bsk_rmdup_emit_run): the
bytes are those of the one-call bsk.RmDup and of the oracle whatever the budget and the cut of the input into shards; the
histogram and the verdict bits against the restatement in rmdup_buckets_ref.py; the smallest shapes, counts past the grid of the
histogram, distinct subjects under one key, global indices past 2^32, a subject of several MiB; misuse; the command line."""
import ctypes as C
import functools
import json
import os
import random
import subprocess

import pytest

import bigseqkit_amd as bsk
from bigseqkit_amd import _lib
from bigseqkit_amd._lib import lib, check
import oracle
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
    """the passes of bsk.RmDupBuckets, step by step: (bytes, buckets, removed, flagged, verdict, (hist bytes, hist records))"""
    with bsk.Operator("RmDup", json.dumps(o), 0) as op:
        bsk.RmDupHistReset(op)
        counts = bsk.RmDupHistRun(op, f)
        hist = bsk.RmDupHistGet(op)
        bounds = bsk.ShufflePlan(hist[0], budget)
        total = sum(counts)
        bsk.RmDupVerdictBegin(op, total)
        removed = flagged = 0
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            r, fl = bsk.RmDupBucket(op, f, counts, lo, hi)
            removed, flagged = removed + r, flagged + fl
        verdict = bsk.RmDupVerdictGet(op, 0, total)
        return bsk.RmDupEmit(op, f, counts), len(bounds) - 1, removed, flagged, verdict, hist


@functools.lru_cache(maxsize=None)
def one_call(name, oj):
    data, fastq = R.shape(name)
    return bsk.RmDup(frame(data, fastq), Opts(json.loads(oj)))


# ------------------------------------------------------------------ parity
CASES = [(n, o) for n in R.SHAPES for o in R.OPTION_SETS]
CASES += [(n, dict(o, LineWidth=w)) for n in ("fasta 7", "fasta 60") for w in (0, 60) for o in ({}, {"BySeq": True})]


@pytest.mark.parametrize("name,o", CASES, ids=lambda v: v if isinstance(v, str) else ("+".join("%s" % k if x is True else "%s%s" % (k, x) for k, x in v.items()) or "id"))
def test_buckets_equal_the_one_call_and_the_oracle(name, o):
    oj = json.dumps(o)
    data, fastq = R.shape(name)
    want = R.want_of(name, oj)
    assert one_call(name, oj) == want
    recs, subs, hb, hr = R.restated(name, json.dumps({k: v for k, v in o.items() if k != "LineWidth"}))
    verdict = R.py_verdict(subs)
    for budget, least in zip(R.budgets_of(hb), (1, 8, 8)):
        for parts in (1, 3, 7):
            got, nb, removed, flagged, bits, hist = run(frame(data, fastq, parts), o, budget)
            assert got == want, (budget, parts, nb)
            assert nb >= least and (least > 1 or nb == 1)
            assert bits == verdict and removed == sum(verdict) and flagged == 0
            assert hist == (hb, hr)
    assert bsk.RmDupBuckets(frame(data, fastq, 3), Opts(o), R.budgets_of(hb)[1]) == want


# ------------------------------------------------------------------ the histogram
@pytest.mark.parametrize("name", R.SHAPES)
def test_histogram_is_the_restated_one(name):
    data, fastq = R.shape(name)
    for o in R.OPTION_SETS + ({"IgnoreCase": True}, {"ByName": True, "IgnoreCase": True}):
        recs, subs, hb, hr = R.restated(name, json.dumps(o))
        with bsk.Operator("RmDup", json.dumps(o), 0) as op:
            counts = bsk.RmDupHistRun(op, frame(data, fastq, 7))
            assert sum(counts) == len(recs)
            assert bsk.RmDupHistGet(op) == (hb, hr), o
            bsk.RmDupHistRun(op, frame(data, fastq, 1))                          # the counters accumulate ...
            assert bsk.RmDupHistGet(op) == ([2 * v for v in hb], [2 * v for v in hr])
            bsk.RmDupHistReset(op)                                                  # ... until they are reset
            assert bsk.RmDupHistGet(op) == ([0] * BINS, [0] * BINS)


# ------------------------------------------------------------------ the verdict bits at the smallest shapes
def pattern_ids(n, pattern):
    if pattern == "all repeat record 0":
        return [0] * n
    if pattern == "alternating":
        return [i if i % 2 == 0 else i - 1 for i in range(n)]                    # every odd record repeats the one before it
    return list(range(n))                                                          # no duplicate


def tiny(ids, fastq):
    if fastq:
        return b"".join(b"@r%d\nACGT\n+\nIIII\n" % i for i in ids)
    return b"".join(b">r%d\nACGT\n" % i for i in ids)


@pytest.mark.parametrize("n", (1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4097))
def test_verdict_bits(n):
    """the words of the bitmap (32 records) and the tile of the scans (2048 records)"""
    for pattern in ("all repeat record 0", "alternating", "no duplicate"):
        ids = pattern_ids(n, pattern)
        want_bits = R.py_verdict(ids)
        hb = R.py_hist([b"r%d" % i for i in ids])[0]
        for fastq, parts, budget in ((True, 1, 1 << 30), (False, 3, max(max(hb), sum(hb) // 4))):
            data = tiny(ids, fastq)
            got, nb, removed, flagged, bits, hist = run(frame(data, fastq, parts), {}, budget)
            assert bits == want_bits, (pattern, fastq)
            assert removed == sum(want_bits) and flagged == 0
            if pattern == "no duplicate":
                assert removed == 0 and got == data
            assert got == tiny([i for i, v in zip(ids, want_bits) if not v], fastq)


# ------------------------------------------------------------------ more records than the grid stride of the histogram
@pytest.mark.parametrize("parts", [1, 3])
def test_counts_past_the_grid_of_the_histogram(parts):
    """one shard: a launch with more records than the lanes of the histogram's grid, so its loop takes a second stride; three
    shards: every launch stays below the grid, the counters add up over the launches"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 3 * cus * 256 + 1234
    ids = [i % (n - 5000) for i in range(n)]                                       # IDs of a few bytes, 5000 of them twice
    data = b"".join(b">%x\nA\n" % i for i in ids)
    subs = [b"%x" % i for i in ids]
    hb, hr = R.py_hist(subs)
    got, nb, removed, flagged, bits, hist = run(frame(data, False, parts), {}, sum(hb) // 4 + 1)
    assert hist == (hb, hr) and sum(hist[1]) == n
    assert nb >= 4 and removed == 5000 and flagged == 0
    assert bits == R.py_verdict(subs)
    assert got == oracle.rmdup(data, False)


# ------------------------------------------------------------------ distinct subjects under one key
@pytest.mark.parametrize("o", ({}, {"BySeq": True, "IgnoreCase": True}), ids=("id", "seq-i"))
def test_distinct_subjects_under_one_key_are_kept_apart(o, monkeypatch):
    rng = random.Random(16)
    recs = []
    for i in range(3000):
        seq = "".join(rng.choice("ACGTacgt") for _ in range(rng.randint(20, 40)))
        recs.append(("q%d" % i, seq))
    recs += [rng.choice(recs[:3000]) for _ in range(600)]                          # duplicates of both kinds of subject
    rng.shuffle(recs)
    data = "".join("@%s\n%s\n+\n%s\n" % (h, s, "I" * len(s)) for h, s in recs).encode()
    want = oracle.rmdup(data, True, json.dumps(o))
    subs = [R.subject(r, o) for r in R.parse(data, True)]
    hb, hr = R.py_hist(subs)
    plain = run(frame(data, True, 3), o, sum(hb) // 3 + 1)
    assert plain[0] == want and plain[3] == 0
    monkeypatch.setenv("BSK_RMDUP_K1_BITS", "16")                                  # 3000 subjects under 65 536 keys: some pairs collide
    got, nb, removed, flagged, bits, hist = run(frame(data, True, 3), o, sum(hb) // 3 + 1)
    assert got == want and bits == R.py_verdict(subs) == plain[4]
    assert flagged > 0 and removed == sum(bits)
    assert hist == (hb, hr) == plain[5] and nb == plain[1]                         # the bins come from the whole k1


# ------------------------------------------------------------------ global indices past 2^32
def test_indices_past_2_to_32():
    ids_a, ids_b = [1, 2, 3, 1, 4, 5, 2, 6], [7, 1, 8, 6, 6, 9, 3, 10]
    a, b = tiny(ids_a, True), tiny(ids_b, True)
    first_a, first_b = (1 << 32) - 3, (1 << 32) + 5
    want_bits = R.py_verdict(ids_a + ids_b)
    with bsk.Operator("RmDup", "{}", 0) as op:
        bsk.RmDupVerdictBegin(op, (1 << 32) + 16)
        check(lib.bsk_rmdup_bucket_begin(op.ctx, 0, BINS), op.ctx)
        for text, first in ((a, first_a), (b, first_b)):
            check(lib.bsk_rmdup_bucket_add(op.ctx, text, len(text), 0, bsk.FORMAT_FASTQ, 0, first, None), op.ctx)
        removed, flagged = C.c_uint64(), C.c_uint64()
        check(lib.bsk_rmdup_bucket_finish(op.ctx, None, C.byref(removed), C.byref(flagged)), op.ctx)
        assert (removed.value, flagged.value) == (sum(want_bits), 0)
        assert bsk.RmDupVerdictGet(op, first_a - 5, 5 + 16 + 3) == bytes(5) + want_bits + bytes(3)
        assert bsk.RmDupVerdictGet(op, 0, 40) == bytes(40)                         # nothing wrapped round to the low indices
        outs = []
        for text, first in ((a, first_a), (b, first_b)):
            out = _lib.Out()
            check(lib.bsk_rmdup_emit_run(op.ctx, text, len(text), 0, bsk.FORMAT_FASTQ, 0, first, None, C.byref(out)), op.ctx)
            buf = C.create_string_buffer(max(1, out.len))
            check(lib.bsk_out_to_host(op.ctx, C.byref(out), buf, out.len), op.ctx)
            outs.append(buf.raw[:out.len])
        assert outs[0] == tiny([1, 2, 3, 4, 5, 6], True) and outs[1] == tiny([7, 8, 9, 10], True)
        assert b"".join(outs) == oracle.rmdup(a + b, True)


# ------------------------------------------------------------------ a subject of several MiB
def test_long_subject():
    rng = random.Random(3)
    block = "".join(rng.choice("ACGT") for _ in range(4099))
    big = (block * ((3 << 20) // len(block)) + "ACGTTGCA").encode()
    small = R.parse(R.shape("fasta 60")[0], False)[:20]
    recs = small[:10] + [(b"chrA first", big)] + small[10:] + [(b"chrB copy", big), (b"chrC lower", big.lower()), (b"chrD other", big[:-1] + b"C")]
    data = R.fasta_text(recs, 60)
    for o, gone in (({"BySeq": True}, {b"chrB copy"}), ({"BySeq": True, "IgnoreCase": True}, {b"chrB copy", b"chrC lower"})):
        want = oracle.rmdup(data, False, json.dumps(o))
        subs = [R.subject(r, o) for r in recs]
        hb, hr = R.py_hist(subs)
        for budget in (sum(hb), max(hb)):
            got, nb, removed, flagged, bits, hist = run(frame(data, False, 3), o, budget)
            assert got == want and hist == (hb, hr), (o, budget)
            assert bits == R.py_verdict(subs) and flagged == 0
            assert {r[0] for r, v in zip(recs, bits) if v and r[0].startswith(b"chr")} == gone


# ------------------------------------------------------------------ misuse and refusals
def test_refusals_and_misuse(tmp_path):
    data, fastq = R.shape("fastq")
    f = frame(data, fastq)
    (pid, ptr, n, on_dev, keep), = f.partitions()
    fmt = f.format
    err = lambda op: lib.bsk_last_error(op.ctx).decode()
    INV, UNS = _lib.BSK_ERR_INVALID_ARG, _lib.BSK_ERR_UNSUPPORTED
    k, r, fl = C.c_uint64(), C.c_uint64(), C.c_uint64()
    with bsk.Operator("RmDup", "{}", 0) as op:
        out = _lib.Out()
        assert lib.bsk_rmdup_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 0, None) == INV and "no bucket is open" in err(op)
        assert lib.bsk_rmdup_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)) == INV and "no bucket is open" in err(op)
        assert lib.bsk_rmdup_bucket_begin(op.ctx, 0, BINS) == INV and "bsk_rmdup_verdict_begin first" in err(op)
        assert lib.bsk_rmdup_emit_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(out)) == INV and "bsk_rmdup_verdict_begin" in err(op)
        assert lib.bsk_rmdup_bucket_begin(op.ctx, 5, 5) == INV and lib.bsk_rmdup_bucket_begin(op.ctx, 0, BINS + 1) == INV
        check(lib.bsk_rmdup_hist_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(k)), op.ctx)
        total = k.value
        bsk.RmDupVerdictBegin(op, total)
        check(lib.bsk_rmdup_bucket_begin(op.ctx, 0, 2048), op.ctx)
        assert lib.bsk_rmdup_bucket_begin(op.ctx, 2048, BINS) == INV and "a bucket is open" in err(op)
        # an add that is refused before it runs leaves the bucket usable
        assert lib.bsk_rmdup_bucket_add(op.ctx, ptr, n, 0, 99, 0, 0, None) == INV and "format" in err(op)
        assert lib.bsk_rmdup_bucket_add(op.ctx, None, n, 0, fmt, 0, 0, None) == INV and "null shard" in err(op)
        check(lib.bsk_rmdup_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 0, None), op.ctx)
        check(lib.bsk_rmdup_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)), op.ctx)
        # half of the bins are decided: the emit names the first one that is not
        assert lib.bsk_rmdup_emit_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(out)) == INV and "fine bin 2048 has not been decided" in err(op)
        # the shards of a bucket arrive in input order: a first_record that goes backwards closes the bucket
        check(lib.bsk_rmdup_bucket_begin(op.ctx, 2048, BINS), op.ctx)
        half = R.cuts_of(data, fastq, 3)[1]
        check(lib.bsk_rmdup_bucket_add(op.ctx, data[:half], half, 0, fmt, 0, 100, None), op.ctx)
        assert lib.bsk_rmdup_bucket_add(op.ctx, data[:half], half, 0, fmt, 0, 99, None) == INV and "goes backwards" in err(op)
        assert lib.bsk_rmdup_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)) == INV and "no bucket is open" in err(op)
        # a shard that reaches past total_records
        check(lib.bsk_rmdup_bucket_begin(op.ctx, 2048, BINS), op.ctx)
        assert lib.bsk_rmdup_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 1, None) == INV and "reach past the total_records = %d" % total in err(op)
        assert lib.bsk_rmdup_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)) == INV                       # ... has closed the bucket
        check(lib.bsk_rmdup_bucket_begin(op.ctx, 2048, BINS), op.ctx)
        check(lib.bsk_rmdup_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 0, None), op.ctx)
        check(lib.bsk_rmdup_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)), op.ctx)
        assert lib.bsk_rmdup_emit_run(op.ctx, ptr, n, 0, fmt, 0, 1, None, C.byref(out)) == INV and "reach past" in err(op)
        check(lib.bsk_rmdup_emit_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(out)), op.ctx)
        buf = C.create_string_buffer(max(1, out.len))
        check(lib.bsk_out_to_host(op.ctx, C.byref(out), buf, out.len), op.ctx)
        assert buf.raw[:out.len] == R.want_of("fastq", "{}")                                                     # the context is whole after all that
        assert lib.bsk_rmdup_verdict_get(op.ctx, total, 1, (C.c_uint8 * 1)()) == INV and "reach past" in err(op)
        bsk.RmDupVerdictBegin(op, total)                                                                        # a new verdict forgets the decided bins
        assert lib.bsk_rmdup_emit_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(out)) == INV and "fine bin 0 has not been decided" in err(op)
    # a single bin above the budget: the plan's refusal
    hb = R.restated("fastq", "{}")[2]
    with pytest.raises(bsk.BskError) as e:
        bsk.RmDupBuckets(f, Opts({}), max(hb) - 1)
    assert e.value.code == UNS and "holds %d bytes" % next(v for v in hb if v > max(hb) - 1) in str(e.value) and "budget of %d bytes" % (max(hb) - 1) in str(e.value)
    # -d / -D side files
    for side in ("DupSeqsFile", "DupNumFile"):
        with bsk.Operator("RmDup", json.dumps({side: str(tmp_path / "side")}), 0) as op:
            assert lib.bsk_rmdup_hist_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(k)) == UNS
            assert "-d / -D side files are not available" in err(op)
    # out=slices on the emit
    os.environ["BSK_OUT"] = "slices"
    try:
        with bsk.Operator("RmDup", "{}", 0) as op:
            counts = bsk.RmDupHistRun(op, f)
            bsk.RmDupVerdictBegin(op, sum(counts))
            bsk.RmDupBucket(op, f, counts, 0, BINS)
            out = _lib.Out()
            assert lib.bsk_rmdup_emit_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(out)) == UNS and "out=slices" in err(op)
    finally:
        del os.environ["BSK_OUT"]
    # every entry point on a context of another operator
    with bsk.Operator("Shuffle", "{}", 0) as op:
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


def test_cli_rmdup_in_buckets(tmp_path):
    """a FASTQ file; two FASTA files, the first one without its final newline, unioned in order"""
    fq = R.shape("fastq")[0]
    a, b = R.shape("fasta 60")[0][:-1], R.shape("fasta 7")[0]
    ffq, fa, fb = (str(tmp_path / x) for x in ("r.fq", "a.fa", "b.fa"))
    for path, text in ((ffq, fq), (fa, a), (fb, b)):
        open(path, "wb").write(text)
    out = str(tmp_path / "o")
    streamed = {"BSK_STREAM_PIECE_BYTES": "9000", "BSK_STAGE_BYTES": "4096"}
    for files, union, fastq in (([ffq], fq, True), ([fa, fb], a + b"\n" + b, False)):
        for flags in ([], ["-s", "-i"], ["-n"]):
            o = {"BySeq": "-s" in flags, "IgnoreCase": "-i" in flags, "ByName": "-n" in flags}
            args = ["rmdup", *files, "-o", out, "--merge", *flags]
            want = oracle.rmdup(union, fastq, json.dumps(o))
            hb = R.py_hist([R.subject(r, o) for r in R.parse(union, fastq)])[0]
            streamed["BSK_RMDUP_BUDGET_BYTES"] = str(max(max(hb), sum(hb) // 6))              # six buckets or so, and the fullest bin fits
            p = cli(args, {"BSK_CLI_TIMING": "1"})
            assert open(out, "rb").read() == want and "k_rdb_hist" not in p.stderr.decode()      # one call, as before
            os.remove(out)
            p = cli(args, dict(streamed, BSK_CLI_TIMING="1"))
            assert open(out, "rb").read() == want, (files, flags)
            err = p.stderr.decode()
            assert all(s in err for s in ("k_rdb_hist", "k_rdb_pick", "k_rdb_pack", "k_rdb_verify", "k_rdb_apply")), err[-800:]
            assert int(err.split("rmdup in ")[1].split(" bucket")[0]) >= 3 and int(err.split(" bytes, ")[1].split(" piece")[0]) >= 3
            nrec = len(R.parse(union, fastq))
            assert "rmdup: %d record(s) removed, 0 flagged" % (nrec - len(R.parse(want, fastq))) in err
            os.remove(out)
    # a single bin above the budget ends with the plan's message
    p = subprocess.run([CLI, "rmdup", ffq, "-o", out], capture_output=True, timeout=900, env=dict(os.environ, BSK_RMDUP_BUDGET_BYTES="20"))
    assert p.returncode != 0 and "more than the budget of 20 bytes" in p.stderr.decode() and "rmdup: a fine bin" in p.stderr.decode()
    # -d is refused on this path
    p = subprocess.run([CLI, "rmdup", ffq, "-o", out, "-d", str(tmp_path / "dups")], capture_output=True, timeout=900, env=dict(os.environ, **streamed))
    assert p.returncode != 0 and "-d / -D side files are not available" in p.stderr.decode()
    # an input that cannot be loaded whole is told about the switch, and with it goes through the buckets
    p = subprocess.run([CLI, "rmdup", ffq, "-o", out], capture_output=True, timeout=900, env=dict(os.environ, BSK_SHARD_FAIL_ALLOC="1"))
    assert p.returncode != 0 and "BSK_RMDUP_BUDGET_BYTES" in p.stderr.decode()
    p = cli(["rmdup", ffq, "-o", out, "--merge"], {"BSK_RMDUP_BUDGET_BYTES": str(1 << 30), "BSK_SHARD_FAIL_ALLOC": "1", "BSK_CLI_TIMING": "1"})
    assert open(out, "rb").read() == R.want_of("fastq", "{}") and "rmdup in 1 bucket(s)" in p.stderr.decode()
