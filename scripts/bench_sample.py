#!/usr/bin/env python3
"""`sample` and `shuffle` on HBM-resident synthetic shards (1 GPU): a FASTQ-150 shard and a FASTA-1k shard from
bsk_synth_device.  Every output is compared byte for byte (`exact`) with a torch restatement of the draw
(csrc/sample_dev.hpp) applied to the fixed record layout.  Legs: sample -p 0.1, -p 0.5, -p 1, shuffle.  Each leg is timed
next to a yardstick on the same shard in the same run: for `sample -p f`, `range 1:ceil(f N)` (the same number of bytes
through the same index pass and segment copy, as ONE contiguous run); for `shuffle`, `sort -l` (index, radix sort,
permuted emit).  With --buckets N the shuffle is also run in N buckets of the draw (histogram pass, then N collect passes over
the same HBM-resident shard, bounds from bsk_shuffle_plan with a budget of 1/N of the output plus the largest fine bin) and
reported next to the one-pass shuffle as `ratio_to_one_pass`; the shard is read 1 + N times there.  Per leg: median ms over the repetitions, the spread (max - min) / median, the ratio to the yardstick
and the per-stage device times of bsk_profile_dump (one extra profiled call).  Prints one JSON object.  Not the driver's
bench (that is bench.py).
  python scripts/bench_sample.py [GB per shard, default 2] [reps, default 5] [--buckets N]"""
import ctypes as C
import json
import math
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bigseqkit_amd as bsk
from bigseqkit_amd import _lib
from bigseqkit_amd._lib import lib, check

argv = sys.argv[1:]
n_buckets = 0
if "--buckets" in argv:
    at = argv.index("--buckets")
    n_buckets = int(argv[at + 1])
    del argv[at:at + 2]
gb = float(argv[0]) if len(argv) > 0 else 2.0
reps = int(argv[1]) if len(argv) > 1 else 5


def s64(x):  # a 64-bit constant as the int64 torch computes in (products wrap, as the unsigned ones do)
    return x - (1 << 64) if x >= 1 << 63 else x


def lsr(x, k):  # logical shift right of int64 words
    return (x >> k) & ((1 << (64 - k)) - 1)


def splitmix64(x):
    x = x + s64(0x9E3779B97F4A7C15)
    x = (x ^ lsr(x, 30)) * s64(0xBF58476D1CE4E5B9)
    x = (x ^ lsr(x, 27)) * s64(0x94D049BB133111EB)
    return x ^ lsr(x, 31)


def draws(seed, n):
    key = splitmix64(torch.tensor([seed], dtype=torch.int64, device="cuda"))
    return splitmix64(key ^ torch.arange(n, dtype=torch.int64, device="cuda"))


def synth(kind, nbytes):
    rb = lib.bsk_synth_record_bytes(kind)
    n = int(nbytes) // rb * rb
    t = torch.empty(n, dtype=torch.uint8, device="cuda")
    check(lib.bsk_synth_device(kind, 42, 0, 0, C.c_void_p(t.data_ptr()), n, 0, None))
    torch.cuda.synchronize()
    return t, n // rb, rb


def timed(op_name, fn, opts, t, fmt):
    out = _lib.Out()
    with bsk.Operator(op_name, json.dumps(opts), 0) as op:
        call = lambda: check(fn(op.ctx, C.c_void_p(t.data_ptr()), t.numel(), 1, fmt, 0, None, C.byref(out)), op.ctx)
        call()  # (sizes the buffers)
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        lib.bsk_profile_reset(op.ctx)
        lib.bsk_profile_enable(op.ctx, 1)
        call()
        torch.cuda.synchronize()
        pb = C.create_string_buffer(1 << 16)
        check(lib.bsk_profile_dump(op.ctx, pb, len(pb)), op.ctx)
        stages = {}
        for item in pb.value.decode().split(";"):
            if "=" in item:
                k, v = item.rsplit("=", 1)
                stages[k] = round(float(v.split("/")[0]), 3)
        got = torch.empty(out.len, dtype=torch.uint8, device="cuda")
        if out.len:
            check(lib.bsk_device_copy(C.c_void_p(got.data_ptr()), out.d_data, out.len, 3))
    ms.sort()
    med = ms[len(ms) // 2]
    return {"ms": round(med, 3), "spread": round((ms[-1] - ms[0]) / med, 3), "stages_ms": stages, "out_GB": round(out.len / 1e9, 3)}, got


def timed_buckets(t, fmt, nb):
    """the shuffle of shard `t` in about `nb` buckets through one context: histogram, plan, begin / add / finish per bucket"""
    ptr, n = C.c_void_p(t.data_ptr()), t.numel()
    out = _lib.Out()
    got = None
    with bsk.Operator("Shuffle", "{}", 0) as op:
        def run(keep):
            check(lib.bsk_shuffle_hist_reset(op.ctx), op.ctx)
            k = C.c_uint64()
            check(lib.bsk_shuffle_hist_run(op.ctx, ptr, n, 1, fmt, 0, 0, None, C.byref(k)), op.ctx)
            hb, _ = bsk.ShuffleHistGet(op)
            bounds = bsk.ShufflePlan(hb, sum(hb) // nb + max(hb))
            parts = []
            for lo, hi in zip(bounds[:-1], bounds[1:]):
                check(lib.bsk_shuffle_bucket_begin(op.ctx, lo, hi), op.ctx)
                check(lib.bsk_shuffle_bucket_add(op.ctx, ptr, n, 1, fmt, 0, 0, None), op.ctx)
                check(lib.bsk_shuffle_bucket_finish(op.ctx, None, C.byref(out)), op.ctx)
                if keep:
                    part = torch.empty(out.len, dtype=torch.uint8, device="cuda")
                    if out.len:
                        check(lib.bsk_device_copy(C.c_void_p(part.data_ptr()), out.d_data, out.len, 3))
                    parts.append(part)
            torch.cuda.synchronize()
            return len(bounds) - 1, parts
        run(False)  # (sizes the buffers)
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            nbk, _ = run(False)
            ms.append((time.perf_counter() - t0) * 1e3)
        lib.bsk_profile_reset(op.ctx)
        lib.bsk_profile_enable(op.ctx, 1)
        nbk, parts = run(True)
        pb = C.create_string_buffer(1 << 16)
        check(lib.bsk_profile_dump(op.ctx, pb, len(pb)), op.ctx)
        stages = {}
        for item in pb.value.decode().split(";"):
            if "=" in item:
                k, v = item.rsplit("=", 1)
                stages[k] = round(float(v.split("/")[0]), 3)
        got = torch.cat(parts) if parts else torch.empty(0, dtype=torch.uint8, device="cuda")
    ms.sort()
    med = ms[len(ms) // 2]
    return {"ms": round(med, 3), "spread": round((ms[-1] - ms[0]) / med, 3), "buckets": nbk, "stages_ms": stages}, got


sample_fn = lambda ctx, p, n, dev, fmt, pid, st, out: lib.bsk_sample_run(ctx, p, n, dev, fmt, pid, 0, st, out)
range_fn = lambda ctx, p, n, dev, fmt, pid, st, out: lib.bsk_range_run(ctx, p, n, dev, fmt, pid, 0, st, out)
res = {}
for label, kind, fmt in (("fastq150", 0, 1), ("fasta1k", 1, 0)):
    t, n, rb = synth(kind, gb * 1e9)
    rows = t.view(n, rb)
    for p in (0.1, 0.5, 1.0):
        f = struct.unpack("<f", struct.pack("<f", p))[0]
        T = (1 << 53) if f >= 1 else math.ceil(f * 2.0 ** 53)
        keep = lsr(draws(11, n), 11) < T
        want = rows[keep].reshape(-1)
        leg, got = timed("Sample", sample_fn, {"Proportion": p}, t, fmt)
        leg["exact"] = bool(got.numel() == want.numel() and torch.equal(got, want))
        leg["kept"] = int(keep.sum())
        k = max(1, math.ceil(f * n))
        yard, got = timed("Range", range_fn, {"Range": "1:%d" % k}, t, fmt)
        yard["exact"] = bool(torch.equal(got, rows[:k].reshape(-1)))
        leg["yardstick range 1:%d" % k] = yard
        leg["ratio_to_yardstick"] = round(leg["ms"] / yard["ms"], 3)
        res["%s sample -p %g" % (label, p)] = leg
        print(label, "sample -p", p, json.dumps(leg), file=sys.stderr, flush=True)
        del want, got, keep
    order = torch.argsort(draws(23, n) ^ s64(1 << 63))  # ascending as unsigned words; the draws are distinct
    want = rows[order].reshape(-1)
    leg, got = timed("Shuffle", lib.bsk_shuffle_run, {}, t, fmt)
    leg["exact"] = bool(got.numel() == want.numel() and torch.equal(got, want))
    if n_buckets > 0:
        bleg, bgot = timed_buckets(t, fmt, n_buckets)
        bleg["exact"] = bool(bgot.numel() == want.numel() and torch.equal(bgot, want))
        bleg["ratio_to_one_pass"] = round(bleg["ms"] / leg["ms"], 3)
        leg["in buckets"] = bleg
        del bgot
    del want, got, order
    yard, got = timed("Sort", lib.bsk_sort_run, {"ByLength": True, "Config": {"LineWidth": 60 if fmt == 0 else 0}}, t, fmt)
    leg["yardstick sort -l"] = yard
    leg["ratio_to_yardstick"] = round(leg["ms"] / yard["ms"], 3)
    res["%s shuffle" % label] = leg
    print(label, "shuffle", json.dumps(leg), file=sys.stderr, flush=True)
    del got, t, rows
print(json.dumps({"metric": "sample / shuffle on HBM-resident synthetic shards", "gb": gb, "reps": reps, "records_note": "FASTQ-150: 317 B, FASTA-1k: see bsk_synth_record_bytes(1)", "results": res}))
