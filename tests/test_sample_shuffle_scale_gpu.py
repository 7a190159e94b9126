"""`sample` / `shuffle` at the record counts where their table passes change shape (PARITY.md SAMPLE, SHUF), byte for byte against
tests/sample_ref.py.  The other sample, shuffle and bucket tests stay below 1 000 records: one tile of the scan, one block of
the sort, no grid stride in the histogram, record indices of a few hundred.  Here:

  * the tile of launch_scan_u32 (stream_index.hip SCAN_BLOCK = 2048): 2047, 2048, 2049 and 4097 records;
  * a bucket that accumulates more records than any shard's table held (shuffle_order_emit sizes its scan for the bucket);
  * 3 * CUs * 256 + 257 records: k_shuffle_hist launches at most 3 * CUs blocks of 256 lanes and walks the rest with a grid
    stride.  The sort (rocprim::radix_sort_pairs, 64-bit keys, 32-bit counting-iterator values) runs in ONE block up to
    1 024 items with the installed rocprim (rocprim/device/device_radix_sort.hpp: min(256, block_size) x min(4, items_per_thread)
    of radix_sort_block_sort_config_base, device_config_helper.hpp: 256 x 4 for items of 8 bytes), as a merge sort of several
    blocks up to merge_sort_limit = 1 048 576 items and as onesweep above (tests/test_fuzz_late_commands_cpu.py reads these
    figures from the installed headers); every N of the tile, accumulated and grid tests is above the first limit;
  * first_record at and beyond 2^32 and 2^63: the index of a record in the whole input is a 64-bit number on its whole way.

Inputs are records of a few bytes, the largest input is under 3 MB; the restatement of the largest one is computed once."""
import ctypes as C
import functools

import pytest

import bigseqkit_amd as bsk
from bigseqkit_amd._lib import Out, lib, check
import sample_ref as R
from test_sample_gpu import frame
from test_shuffle_buckets_gpu import BINS, budgets_of, py_hist, py_plan

pytestmark = pytest.mark.gpu

FORMATS = ("fasta", "fastq", "fasta no final newline")
ONE_BLOCK_SORT = 1024   # (the docstring above)


@functools.lru_cache(maxsize=None)
def data_of(fmt, n):
    if fmt == "fastq":
        return b"".join(b"@%d\nA\n+\nI\n" % i for i in range(n))
    data = b"".join(b">%d\nA\n" % i for i in range(n))
    return data[:-1] if fmt == "fasta no final newline" else data


@functools.lru_cache(maxsize=None)
def recs_of(fmt, n):
    recs = R.records(data_of(fmt, n), fmt == "fastq")
    assert len(recs) == n
    return recs


@functools.lru_cache(maxsize=None)
def shuffle_of(fmt, n, seed):
    return R.shuffle(data_of(fmt, n), fmt == "fastq", seed)


@functools.lru_cache(maxsize=None)
def hist_of(fmt, n, seed):
    return py_hist(recs_of(fmt, n), seed)


@functools.lru_cache(maxsize=None)
def sample_of(fmt, n, seed, number, proportion):
    return R.sample(data_of(fmt, n), fmt == "fastq", seed, number, proportion)


def shuffle_opts(seed):
    return bsk.SeqKitShuffleOptions(seed=seed)


def shard_counts(f, fastq):
    return [len(R.records(bytes(s), fastq)) for s in f.shards]


# ---- the tile of the scan
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("n", [2047, 2048, 2049, 4097])
def test_scan_tile_edges(n, fmt):
    data, fastq = data_of(fmt, n), fmt == "fastq"
    assert len(recs_of(fmt, n)) == n
    for o in ({"proportion": 0.5}, {"number": n // 3}):
        want = sample_of(fmt, n, 11, o.get("number", 0), o.get("proportion", 0.0))
        assert want and len(want) < len(data)
        for parts in (1, 3):
            assert bsk.Sample(frame(data, fastq, parts), bsk.SeqKitSampleOptions(**o)) == want, (o, parts)
    for seed in (23, -1):
        want = shuffle_of(fmt, n, seed)
        assert bsk.Shuffle(frame(data, fastq), shuffle_opts(seed)) == want, seed
        hb, _ = hist_of(fmt, n, seed)
        budgets = budgets_of(hb)[:3]
        assert [len(py_plan(hb, b)) - 1 for b in budgets][:2] == [1, 2]
        for parts in (1, 3):
            for budget in budgets:   # 1, 2 and 4 - 5 buckets
                assert bsk.ShuffleBuckets(frame(data, fastq, parts), shuffle_opts(seed), budget) == want, (seed, parts, budget)


# ---- a bucket of more records than any table had
@pytest.mark.parametrize("mode", ["fresh context", "histogram first", "segcopy off"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_accumulated_count_above_the_tables(fmt, mode, monkeypatch):
    """7 shards of fewer than 2048 records (one tile each) make one bucket of 3 * 2048 + 1: the scan over the accumulated
    lengths needs four tiles of scratch in a context whose tables never asked for more than one"""
    if mode == "segcopy off":
        monkeypatch.setenv("BSK_SEGCOPY", "off")
    n, fastq = 3 * 2048 + 1, fmt == "fastq"
    data = data_of(fmt, n)
    f = frame(data, fastq, 7)
    counts = shard_counts(f, fastq)
    assert len(counts) == 7 and max(counts) < 2048 and sum(counts) == n
    with bsk.Operator("Shuffle", shuffle_opts(5).to_json(), 0) as op:
        if mode == "histogram first":
            assert bsk.ShuffleHistRun(op, f) == counts
            assert bsk.ShuffleHistGet(op) == hist_of(fmt, n, 5)
        got = bsk.ShuffleBucket(op, f, counts, 0, BINS)
    assert got == shuffle_of(fmt, n, 5)


# ---- past the grid of the histogram and the one-block sort
def grid_n():
    import torch
    return 3 * torch.cuda.get_device_properties(0).multi_processor_count * 256 + 257


@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("fmt", FORMATS[:2])
def test_histogram_past_its_grid(fmt, parts):
    n, fastq = grid_n(), fmt == "fastq"
    data = data_of(fmt, n)
    assert n > ONE_BLOCK_SORT and len(data) < 3_000_000
    for seed in (23, -(1 << 63)):
        hb, hr = hist_of(fmt, n, seed)
        assert sum(hr) == n and sum(hb) == len(data)
        with bsk.Operator("Shuffle", shuffle_opts(seed).to_json(), 0) as op:
            counts = bsk.ShuffleHistRun(op, frame(data, fastq, parts))
            gb, gr = bsk.ShuffleHistGet(op)
        assert sum(counts) == n and len(counts) == parts
        assert gr == hr and gb == hb, (seed, [(b, x, y) for b, (x, y) in enumerate(zip(gr, hr)) if x != y][:5])


@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("fmt", FORMATS[:2])
def test_shuffle_and_sample_past_the_grid(fmt, parts):
    n, fastq = grid_n(), fmt == "fastq"
    data = data_of(fmt, n)
    f = frame(data, fastq, parts)
    want = shuffle_of(fmt, n, 23)
    assert bsk.Shuffle(f, shuffle_opts(23)) == want
    hb, _ = hist_of(fmt, n, 23)
    budget = sum(hb) // 2 + max(hb)
    assert len(py_plan(hb, budget)) - 1 == 2
    assert bsk.ShuffleBuckets(f, shuffle_opts(23), budget) == want
    assert bsk.Sample(f, bsk.SeqKitSampleOptions(proportion=0.5)) == sample_of(fmt, n, 11, 0, 0.5)


# ---- first_record beyond 32 bits
N_FIRST = 300
FIRSTS = [(1 << 32) - 5, 1 << 32, (1 << 40) + 3, (1 << 63) + 1]
T_HALF = R.threshold(0.5)


def wrong_sets(seed, first):
    """the kept sets that a narrowing to 32 bits would give: of the record index first + i, and of first_record alone.  Below
    2^32 the second one is no mistake (first_record fits; the edge lies inside the shard), so only the first is listed"""
    index32 = [i for i in range(N_FIRST) if R.keeps(seed, (first + i) & 0xFFFFFFFF, T_HALF)]
    if first < (1 << 32):
        return [index32]
    return [index32, R.kept_indices(seed, N_FIRST, T_HALF, first & 0xFFFFFFFF)]


@functools.lru_cache(maxsize=None)
def seed_first():
    """searched on the CPU: a seed for which no narrowing keeps the same records, at any of FIRSTS"""
    return next(s for s in range(1, 1000) if all(R.kept_indices(s, N_FIRST, T_HALF, F) not in wrong_sets(s, F) for F in FIRSTS))


def to_host(ctx, out):
    buf = C.create_string_buffer(max(1, out.len))
    check(lib.bsk_out_to_host(ctx, C.byref(out), buf, out.len), ctx)
    return buf.raw[:out.len]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("first", FIRSTS, ids=["2^32-5", "2^32", "2^40+3", "2^63+1"])
def test_large_first_record(first, fmt, tmp_path):
    seed, fastq = seed_first(), fmt == "fastq"
    data, recs = data_of(fmt, N_FIRST), recs_of(fmt, N_FIRST)
    code = bsk.FORMAT_FASTQ if fastq else bsk.FORMAT_FASTA
    kept = R.kept_indices(seed, N_FIRST, T_HALF, first)
    want = R.sample(data, fastq, seed, 0, 0.5, first=first)
    assert want == b"".join(recs[i] + b"\n" for i in kept) and 0 < len(kept) < N_FIRST
    assert kept not in wrong_sets(seed, first)
    opts = '{"Proportion": 0.5, "Seed": %d}' % seed
    path = str(tmp_path / "o")
    with bsk.Operator("Sample", opts, 0) as op:
        store = C.c_void_p()
        assert lib.bsk_store_open(path.encode(), 1, C.byref(store)) == 0
        check(lib.bsk_sample_set_first_record(op.ctx, first), op.ctx)
        check(lib.bsk_run_to_store(op.ctx, data, len(data), code, 0, store, 0, None, None), op.ctx)
        assert lib.bsk_store_close(store, None) == 0
    assert open(path, "rb").read() == want
    with bsk.Operator("Sample", opts, 0) as op:
        out = Out()
        check(lib.bsk_sample_run(op.ctx, data, len(data), 0, code, 0, first, None, C.byref(out)), op.ctx)
        assert to_host(op.ctx, out) == want and out.records == len(kept)
    order = sorted(range(N_FIRST), key=lambda i: R.draw(seed, first + i))
    assert order != sorted(range(N_FIRST), key=lambda i: R.draw(seed, (first + i) & 0xFFFFFFFF))
    with bsk.Operator("Shuffle", shuffle_opts(seed).to_json(), 0) as op:
        k = C.c_uint64()
        check(lib.bsk_shuffle_hist_run(op.ctx, data, len(data), 0, code, 0, first, None, C.byref(k)), op.ctx)
        assert k.value == N_FIRST
        assert bsk.ShuffleHistGet(op) == py_hist(recs, seed, first=first)
        out = Out()
        check(lib.bsk_shuffle_bucket_begin(op.ctx, 0, BINS), op.ctx)
        check(lib.bsk_shuffle_bucket_add(op.ctx, data, len(data), 0, code, 0, first, None), op.ctx)
        check(lib.bsk_shuffle_bucket_finish(op.ctx, None, C.byref(out)), op.ctx)
        assert to_host(op.ctx, out) == b"".join(recs[i] + b"\n" for i in order) and out.records == N_FIRST
