"""`shuffle` in buckets of the draw on the GPU (PARITY.md SHUF; include/bsk.h bsk_shuffle_hist_run .. bsk_shuffle_bucket_finish):
the bytes are those of tests/sample_ref.py -- and of the one-shard bsk.Shuffle -- whatever the number of buckets and however the
input is cut into shards; the histogram against its restatement; the smallest shapes; misuse; the command line."""
import ctypes as C
import functools
import os
import random
import subprocess

import pytest

import bigseqkit_amd as bsk
from bigseqkit_amd import _lib
from bigseqkit_amd._lib import lib, check
import oracle
import sample_ref as R
import seqgen
from test_sample_gpu import INPUTS, frame, wrapped_fastq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")
BINS = 4096
SEEDS = (23, 0, -1, (1 << 63) - 1)

BY_NAME = {name: (data, fastq) for name, data, fastq in INPUTS}
SHAPES = {
    "fasta wrapped, blank lines": BY_NAME["fasta blank lines, > in headers"],
    "fastq": BY_NAME["fastq"],
    "fastq wrapped at 7": (wrapped_fastq(random.Random(71), 250, 7), True),
}


@functools.lru_cache(maxsize=None)
def want_of(name, seed):
    data, fastq = SHAPES[name]
    return R.shuffle(data, fastq, seed)


@functools.lru_cache(maxsize=None)
def hist_of(name, seed):
    """the histogram restated: bytes (text + newline) and records per fine bin = draw >> 52"""
    data, fastq = SHAPES[name]
    return py_hist(R.records(data, fastq), seed)


def py_hist(recs, seed, first=0):
    hb, hr = [0] * BINS, [0] * BINS
    for i, r in enumerate(recs):
        b = R.draw(seed, first + i) >> 52
        hb[b] += len(r) + 1
        hr[b] += 1
    return hb, hr


def py_plan(hb, budget):
    """the greedy plan restated (the library's is checked against its properties in tests/test_shuffle_plan_cpu.py)"""
    bounds, s = [0], 0
    for b, v in enumerate(hb):
        if s + v > budget:
            bounds.append(b)
            s = 0
        s += v
    return bounds + [BINS]


def budgets_of(hb):
    """budgets that give 1, 2, about 5 and more than 20 buckets: T; T/2 + m (the first bucket passes T/2, the rest fits one);
    T/5 + m (every bucket but the last passes T/5: 4 or 5); max(m, T/25) (no bucket above T/25 where m is below it: 25 or more)"""
    T, m = sum(hb), max(hb)
    out = [T, T // 2 + m, T // 5 + m, max(m, T // 25)]
    counts = [len(py_plan(hb, b)) - 1 for b in out]
    assert counts[0] == 1 and counts[1] == 2 and 4 <= counts[2] <= 5 and counts[3] > 20, counts
    return out


def opts(seed):
    return bsk.SeqKitShuffleOptions().Seed(seed)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_bucketed_equals_the_restatement(name, device):
    data, fastq = SHAPES[name]
    for seed in SEEDS:
        want = want_of(name, seed)
        assert bsk.Shuffle(frame(data, fastq), opts(seed)) == want, (name, seed)
        for parts in (1, 3, 7):
            f = frame(data, fastq, parts, device)
            for budget in budgets_of(hist_of(name, seed)[0]):
                assert bsk.ShuffleBuckets(f, opts(seed), budget) == want, (name, seed, parts, budget)


def test_empty_buckets_and_any_bounds():
    """buckets need not come from the plan: 64 equal intervals over 30 records leave most of them empty"""
    data = seqgen.random_fastq(random.Random(3), 30, 1, 40)
    f = frame(data, True, 3)
    with bsk.Operator("Shuffle", opts(5).to_json(), 0) as op:
        counts = bsk.ShuffleHistRun(op, f)
        assert sum(counts) == 30
        got = [bsk.ShuffleBucket(op, f, counts, lo, lo + 64) for lo in range(0, BINS, 64)]
    assert sum(1 for g in got if not g) >= 34 and b"".join(got) == R.shuffle(data, True, 5)


@pytest.mark.parametrize("segcopy", ["off", "force"])
def test_copy_paths(segcopy, monkeypatch):
    """the byte-wise copies that stand in for the segmented copy (switch segcopy), a last record without its newline included"""
    monkeypatch.setenv("BSK_SEGCOPY", segcopy)
    for name in ("fastq no final newline", "fasta no final newline", "fastq wrapped"):
        data, fastq = BY_NAME[name]
        hb, _ = py_hist(R.records(data, fastq), 24)
        for budget in budgets_of(hb)[1:3]:
            assert bsk.ShuffleBuckets(frame(data, fastq, 3), opts(24), budget) == R.shuffle(data, fastq, 24), (name, budget)


def test_a_context_without_the_histogram_and_a_second_input():
    """the accumulation grows shard by shard when the context never saw the histogram (what it holds moves along), and
    bsk_shuffle_hist_reset makes the context ready for another input"""
    data, fastq = BY_NAME["fastq tiny records"]
    n = len(R.records(data, fastq))
    f = frame(data, fastq, 7)
    starts = [s for s, _ in oracle.record_spans(data, fastq)]
    cuts, at = [], 0
    for sh in f.shards:
        cuts.append((at, at + len(sh)))
        at += len(sh)
    counts = [sum(1 for s in starts if a <= s < b) for a, b in cuts]
    assert sum(counts) == n == 900
    with bsk.Operator("Shuffle", opts(3).to_json(), 0) as op:
        got = bsk.ShuffleBucket(op, f, counts, 0, 2048) + bsk.ShuffleBucket(op, f, counts, 2048, BINS)
        assert got == R.shuffle(data, fastq, 3)
        assert bsk.ShuffleHistRun(op, f) == counts and bsk.ShuffleHistRun(op, f) == counts
        assert sum(bsk.ShuffleHistGet(op)[1]) == 2 * n          # the counters accumulate ...
        bsk.ShuffleHistReset(op)
        assert sum(bsk.ShuffleHistGet(op)[1]) == 0              # ... until they are put back
        assert bsk.ShuffleHistRun(op, f) == counts
        assert bsk.ShuffleHistGet(op) == py_hist(R.records(data, fastq), 3)


@pytest.mark.parametrize("fastq", [True, False])
def test_smallest_shapes(fastq):
    one = b"@r\nACGT\n+\nIIII\n" if fastq else b">r d\nACGT\nAC\n"
    two = one + (b"@s x\nAC\n+\nII\n" if fastq else b">s x\nAC\n")
    for data in (b"", one, one[:-1]):
        for budget in (1 << 30, len(one)):
            assert bsk.ShuffleBuckets(frame(data, fastq), opts(23), budget) == (one if data else b"")
    # two records in two buckets: the budget holds the larger one alone
    for seed in SEEDS:
        hb, _ = py_hist(R.records(two, fastq), seed)
        assert len(py_plan(hb, len(one))) - 1 == 2
        for parts in (1, 2):
            assert bsk.ShuffleBuckets(frame(two, fastq, parts), opts(seed), len(one)) == R.shuffle(two, fastq, seed), (seed, parts)


@pytest.mark.parametrize("fastq", [True, False])
def test_a_last_record_without_newline_lands_inside(fastq):
    rng = random.Random(31)
    data = seqgen.random_fastq(rng, 150, 1, 100, final_newline=False) if fastq else seqgen.random_fasta(rng, 120, 1, 200, final_newline=False)
    assert not data.endswith(b"\n")
    n = len(R.records(data, fastq))
    seed = next(s for s in range(1000) if R.shuffle_order(s, n).index(n - 1) not in (0, n - 1))   # searched on the CPU
    want = R.shuffle(data, fastq, seed)
    hb, _ = py_hist(R.records(data, fastq), seed)
    for parts in (1, 3):
        for device in (False, True):
            for budget in budgets_of(hb):
                got = bsk.ShuffleBuckets(frame(data, fastq, parts, device), opts(seed), budget)
                assert got == want, (parts, device, budget)
    assert want.endswith(b"\n") and not want.endswith(b"\n\n") and len(R.records(want, fastq)) == n


def test_a_shard_of_one_record_between_two_larger_ones():
    data = seqgen.random_fastq(random.Random(32), 201, 1, 80)
    starts = [s for s, _ in oracle.record_spans(data, True)]
    cuts = [0, starts[100], starts[101], len(data)]
    f = bsk.SeqFrame(bsk.FORMAT_FASTQ, [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])])
    hb, _ = py_hist(R.records(data, True), 23)
    for budget in budgets_of(hb):
        assert bsk.ShuffleBuckets(f, opts(23), budget) == R.shuffle(data, True, 23), budget


@pytest.mark.parametrize("name", list(SHAPES))
def test_histogram_equals_its_restatement(name):
    data, fastq = SHAPES[name]
    recs = R.records(data, fastq)
    for seed in SEEDS:
        hb, hr = hist_of(name, seed)
        assert sum(hb) == sum(len(r) + 1 for r in recs) and sum(hr) == len(recs)
        for parts, device in ((1, False), (3, False), (3, True)):
            with bsk.Operator("Shuffle", opts(seed).to_json(), 0) as op:
                counts = bsk.ShuffleHistRun(op, frame(data, fastq, parts, device))
                gb, gr = bsk.ShuffleHistGet(op)
            assert sum(counts) == len(recs) and len(counts) == parts
            assert gb == hb and gr == hr, (name, seed, parts, device)


def test_stage_names_of_the_bucket_path():
    data, fastq = SHAPES["fastq"]
    f = frame(data, fastq, 3)
    with bsk.Operator("Shuffle", "{}", 0) as op:
        check(lib.bsk_profile_enable(op.ctx, 1), op.ctx)
        counts = bsk.ShuffleHistRun(op, f)
        got = bsk.ShuffleBucket(op, f, counts, 0, BINS)
        buf = C.create_string_buffer(1 << 16)
        check(lib.bsk_profile_dump(op.ctx, buf, len(buf)), op.ctx)
    stages = dict(x.split("=") for x in buf.value.decode().split(";") if x)
    for s in ("k_shuffle_hist", "k_shuffle_pick", "shuffle_bucket_sort", "shuffle_bucket_copy"):
        assert s in stages, stages
    assert stages["k_shuffle_hist"].endswith("/3") and stages["k_shuffle_pick"].endswith("/3") and "k_shuffle_keys" not in stages
    assert got == want_of("fastq", 23)


def test_refusals_and_misuse():
    data, fastq = SHAPES["fastq"]
    f = frame(data, fastq)
    with pytest.raises(bsk.BskError) as e:
        bsk.ShuffleBuckets(f, opts(23), 1)
    assert e.value.code == _lib.BSK_ERR_UNSUPPORTED and "budget of 1 bytes" in str(e.value)
    (pid, ptr, n, on_dev, keep), = f.partitions()
    with bsk.Operator("Shuffle", "{}", 0) as op:
        out = _lib.Out()
        assert lib.bsk_shuffle_bucket_add(op.ctx, ptr, n, 0, f.format, 0, 0, None) == _lib.BSK_ERR_INVALID_ARG
        assert "bsk_shuffle_bucket_add" in lib.bsk_last_error(op.ctx).decode()
        assert lib.bsk_shuffle_bucket_finish(op.ctx, None, C.byref(out)) == _lib.BSK_ERR_INVALID_ARG
        assert "bsk_shuffle_bucket_finish" in lib.bsk_last_error(op.ctx).decode()
        check(lib.bsk_shuffle_bucket_begin(op.ctx, 0, BINS), op.ctx)
        assert lib.bsk_shuffle_bucket_begin(op.ctx, 0, BINS) == _lib.BSK_ERR_INVALID_ARG
        assert "bsk_shuffle_bucket_begin" in lib.bsk_last_error(op.ctx).decode()
        assert lib.bsk_shuffle_bucket_begin(op.ctx, 7, 7) == _lib.BSK_ERR_INVALID_ARG
        # the open bucket is still good: the whole range is the one-pass shuffle
        check(lib.bsk_shuffle_bucket_add(op.ctx, ptr, n, 0, f.format, 0, 0, None), op.ctx)
        check(lib.bsk_shuffle_bucket_finish(op.ctx, None, C.byref(out)), op.ctx)
        buf = C.create_string_buffer(out.len)
        check(lib.bsk_out_to_host(op.ctx, C.byref(out), buf, out.len), op.ctx)
        assert buf.raw[:out.len] == want_of("fastq", 23) and out.records == len(R.records(data, fastq))
        assert lib.bsk_shuffle_bucket_finish(op.ctx, None, C.byref(out)) == _lib.BSK_ERR_INVALID_ARG   # finished: closed again
    with bsk.Operator("Sample", '{"Proportion": 0.5}', 0) as op:
        k = C.c_uint64()
        for rc in (lib.bsk_shuffle_hist_run(op.ctx, ptr, n, 0, f.format, 0, 0, None, C.byref(k)),
                   lib.bsk_shuffle_bucket_begin(op.ctx, 0, BINS),
                   lib.bsk_shuffle_bucket_add(op.ctx, ptr, n, 0, f.format, 0, 0, None),
                   lib.bsk_shuffle_bucket_finish(op.ctx, None, C.byref(_lib.Out()))):
            assert rc == _lib.BSK_ERR_INVALID_ARG and "not a Shuffle context" in lib.bsk_last_error(op.ctx).decode()


# ------------------------------------------------------------------ the command line
def cli(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([CLI, *args], capture_output=True, timeout=900, env=e)
    assert p.returncode == 0, p.stderr.decode()
    return p


def test_cli_shuffle_in_buckets(tmp_path):
    """the inputs of test_cli_shuffle_and_refusals: two files, the first one without its final newline, unioned in order"""
    rng = random.Random(50)
    a, b = seqgen.random_fastq(rng, 800, 1, 150), seqgen.random_fastq(rng, 300, 1, 90, final_newline=False)
    fa, fb = str(tmp_path / "a.fq"), str(tmp_path / "b.fq")
    open(fa, "wb").write(a)
    open(fb, "wb").write(b)
    want = R.shuffle(b + b"\n" + a, True, 24)
    out = str(tmp_path / "o")
    args = ["shuffle", "-s", "24", fb, fa, "-o", out, "--merge"]
    p = cli(args, {"BSK_CLI_TIMING": "1"})
    assert open(out, "rb").read() == want and "k_shuffle_pick" not in p.stderr.decode()          # one pass, as before
    os.remove(out)
    streamed = {"BSK_SHUFFLE_BUDGET_BYTES": "20000", "BSK_STREAM_PIECE_BYTES": "30000", "BSK_STAGE_BYTES": "4096"}
    p = cli(args, dict(streamed, BSK_CLI_TIMING="1"))
    assert open(out, "rb").read() == want
    assert "k_shuffle_pick" in p.stderr.decode() and "k_shuffle_hist" in p.stderr.decode(), p.stderr.decode()[-800:]
    os.remove(out)
    cli(args, streamed)
    assert open(out, "rb").read() == want
    os.remove(out)
    # an input that fits the budget but cannot be loaded whole goes through the buckets too
    p = cli(args, {"BSK_SHUFFLE_BUDGET_BYTES": str(1 << 30), "BSK_SHARD_FAIL_ALLOC": "1", "BSK_CLI_TIMING": "1"})
    assert open(out, "rb").read() == want and "shuffle in 1 bucket(s)" in p.stderr.decode()
