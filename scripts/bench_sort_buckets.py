#!/usr/bin/env python3
"""`sort` in buckets of the key next to the one-pass `sort`, on HBM-resident synthetic shards (1 GPU): a FASTQ-150 shard and a
FASTA-1k shard from bsk_synth_device, by ID, by sequence (-s) and by length (-l).  The bucket path runs through one context:
the sample of the keys (about 32 samples per fine bin), the splitters, the histogram, bsk_shuffle_plan with a budget of 1/N of
the bytes plus the largest fine bin, then begin / add / finish per bucket -- the shard is read 2 + N times.  Every bucketed
output is compared byte for byte (`exact`) with the one-pass output of the same shard in the same run.  Per leg: median ms
over the repetitions, the spread (max - min) / median, `ratio_to_one_pass`, and the per-stage device times of
bsk_profile_dump (one extra profiled call).  Nothing about the speed of this path has been tuned: the piece size, the budget
and the 32 samples per bin are starting values.  Prints one JSON object.  Not the driver's bench (that is bench.py).
  python scripts/bench_sort_buckets.py [GB per shard, default 2] [reps, default 3] [--buckets N, default 4]"""
import ctypes as C
import json
import sys

from bucket_bench import synth, device_copy, measure, profiled
import torch
import bigseqkit_amd as bsk
from bigseqkit_amd import _lib
from bigseqkit_amd._lib import lib, check

argv = sys.argv[1:]
n_buckets = 4
if "--buckets" in argv:
    at = argv.index("--buckets")
    n_buckets = int(argv[at + 1])
    del argv[at:at + 2]
gb = float(argv[0]) if len(argv) > 0 else 2.0
reps = int(argv[1]) if len(argv) > 1 else 3


def one_pass(t, fmt, opts):
    out = _lib.Out()
    with bsk.Operator("Sort", json.dumps(opts), 0) as op:
        def run(keep):
            check(lib.bsk_sort_run(op.ctx, C.c_void_p(t.data_ptr()), t.numel(), 1, fmt, 0, None, C.byref(out)), op.ctx)
            torch.cuda.synchronize()
            return device_copy(out) if keep else None
        leg = measure(run, reps)
        got = profiled(op, run, leg)
    return leg, got


def in_buckets(t, fmt, opts, n_records, nb):
    ptr, n = C.c_void_p(t.data_ptr()), t.numel()
    out = _lib.Out()
    rate = min(1.0, bsk.api.SORT_SAMPLES_PER_BIN * bsk.api.SORT_BINS / max(1, n_records))
    info = {}
    with bsk.Operator("Sort", json.dumps(opts), 0) as op:
        def run(keep):
            k = C.c_uint64()
            check(lib.bsk_sort_sample_reset(op.ctx), op.ctx)
            check(lib.bsk_sort_sample_run(op.ctx, ptr, n, 1, fmt, 0, 0, rate, None, C.byref(k)), op.ctx)
            info["bins"] = bsk.SortSplittersBuild(op)
            check(lib.bsk_sort_hist_reset(op.ctx), op.ctx)
            check(lib.bsk_sort_hist_run(op.ctx, ptr, n, 1, fmt, 0, 0, None, C.byref(k)), op.ctx)
            hb, _ = bsk.SortHistGet(op)
            bounds = bsk.ShufflePlan(hb, sum(hb) // nb + max(hb))
            buckets = list(zip(bounds[:-1], bounds[1:]))
            if opts.get("Reverse"):
                buckets.reverse()
            parts = []
            for lo, hi in buckets:
                check(lib.bsk_sort_bucket_begin(op.ctx, lo, hi), op.ctx)
                check(lib.bsk_sort_bucket_add(op.ctx, ptr, n, 1, fmt, 0, 0, None), op.ctx)
                check(lib.bsk_sort_bucket_finish(op.ctx, None, C.byref(out)), op.ctx)
                if keep:
                    parts.append(device_copy(out))
            torch.cuda.synchronize()
            info["buckets"] = len(buckets)
            info["largest_bin_share"] = round(max(hb) / max(1, sum(hb)), 4)
            return torch.cat(parts) if parts else None
        leg = measure(run, reps)
        got = profiled(op, run, leg)
    leg.update(info)
    return leg, got


res = {}
for label, kind, fmt in (("fastq150", 0, 1), ("fasta1k", 1, 0)):
    t, n_records = synth(kind, gb * 1e9)
    cfg = {"LineWidth": 60 if fmt == 0 else 0}
    for name, o in (("by ID", {}), ("-s", {"BySeq": True}), ("-l", {"ByLength": True})):
        opts = dict(o, Config=cfg)
        one, want = one_pass(t, fmt, opts)
        leg, got = in_buckets(t, fmt, opts, n_records, n_buckets)
        leg["exact"] = bool(got is not None and got.numel() == want.numel() and torch.equal(got, want))
        leg["ratio_to_one_pass"] = round(leg["ms"] / one["ms"], 3)
        leg["one pass"] = one
        res["%s sort %s" % (label, name)] = leg
        print(label, "sort", name, json.dumps(leg), file=sys.stderr, flush=True)
        del want, got
    del t
print(json.dumps({"metric": "sort in buckets of the key next to the one-pass sort, HBM-resident synthetic shards", "gb": gb, "reps": reps,
                  "buckets_asked": n_buckets, "results": res}))
