#!/usr/bin/env python3
"""`rename` in buckets of the key next to the one-call `rename`, on HBM-resident synthetic shards (1 GPU): a FASTQ-150 shard and a
FASTA-1k shard from bsk_synth_device whose second half repeats the records of the first, so every ID comes twice and half of the
records are renamed; by ID and by name (-n).  The bucket path runs through one context: the histogram of the fine bins,
bsk_shuffle_plan with a budget of 1/N of the histogram's bytes plus the largest fine bin for N = 1, 4 and 16, the verdict, begin /
add / finish per bucket and one emit pass -- the shard is read 2 + N times.  Every bucketed output is compared byte for byte
(`exact`) with the one-call output of the same shard in the same run.  Per leg: median ms over the repetitions, the spread
(max - min) / median, `ratio_to_one_call`, the records renamed and flagged, and the per-stage device times of bsk_profile_dump (one
extra profiled call): k_rmdup_hash and k_rdb_hist are the histogram pass, k_rdb_pick and k_rdb_pack the collect passes,
rmdup_group(sort+dedupe), k_renb_verify, renb_ordinals(sort+rank) and k_renb_scatter the finish, k_sizes_scan and the emit kernel
the emit.  Nothing about the speed of this path has been tuned.  Prints one JSON object.  Not the driver's bench (that is bench.py).
  python scripts/bench_rename_buckets.py [GB per shard, default 1] [reps, default 3]"""
import ctypes as C
import json
import sys

from bucket_bench import synth_at, device_copy, measure, profiled
import torch
import bigseqkit_amd as bsk
from bigseqkit_amd import _lib
from bigseqkit_amd._lib import lib, check

argv = sys.argv[1:]
gb = float(argv[0]) if len(argv) > 0 else 1.0
reps = int(argv[1]) if len(argv) > 1 else 3


def synth(kind, nbytes):
    """two copies of the first nbytes / 2 of the synthetic file, back to back"""
    rb = lib.bsk_synth_record_bytes(kind)
    half = int(nbytes) // (2 * rb) * rb
    t = torch.empty(2 * half, dtype=torch.uint8, device="cuda")
    for at in (0, half):
        synth_at(kind, t, at, half)
    torch.cuda.synchronize()
    return t, 2 * half // rb


def one_call(t, fmt, opts):
    out = _lib.Out()
    with bsk.Operator("Rename", json.dumps(opts), 0) as op:
        def run(keep):
            check(lib.bsk_rename_run(op.ctx, C.c_void_p(t.data_ptr()), t.numel(), 1, fmt, 0, None, C.byref(out)), op.ctx)
            torch.cuda.synchronize()
            return device_copy(out) if keep else None
        leg = measure(run, reps)
        got = profiled(op, run, leg)
    return leg, got


def in_buckets(t, fmt, opts, nb):
    ptr, n = C.c_void_p(t.data_ptr()), t.numel()
    out = _lib.Out()
    info = {}
    with bsk.Operator("Rename", json.dumps(opts), 0) as op:
        def run(keep):
            k, r, f = C.c_uint64(), C.c_uint64(), C.c_uint64()
            check(lib.bsk_rename_hist_reset(op.ctx), op.ctx)
            check(lib.bsk_rename_hist_run(op.ctx, ptr, n, 1, fmt, 0, 0, None, C.byref(k)), op.ctx)
            hb, _ = bsk.RenameHistGet(op)
            bounds = bsk.ShufflePlan(hb, sum(hb) // nb + max(hb))
            check(lib.bsk_rename_verdict_begin(op.ctx, k.value), op.ctx)
            renamed = flagged = 0
            for lo, hi in zip(bounds[:-1], bounds[1:]):
                check(lib.bsk_rename_bucket_begin(op.ctx, lo, hi), op.ctx)
                check(lib.bsk_rename_bucket_add(op.ctx, ptr, n, 1, fmt, 0, 0, None), op.ctx)
                check(lib.bsk_rename_bucket_finish(op.ctx, None, C.byref(r), C.byref(f)), op.ctx)
                renamed, flagged = renamed + r.value, flagged + f.value
            check(lib.bsk_rename_emit_run(op.ctx, ptr, n, 1, fmt, 0, 0, None, C.byref(out)), op.ctx)
            torch.cuda.synchronize()
            info.update(buckets=len(bounds) - 1, renamed=renamed, flagged=flagged, subject_share=round(sum(hb) / max(1, n), 4),
                        largest_bin_share=round(max(hb) / max(1, sum(hb)), 4))
            return device_copy(out) if keep else None
        leg = measure(run, reps)
        got = profiled(op, run, leg)
    leg.update(info)
    return leg, got


res = {}
for label, kind, fmt in (("fastq150", 0, 1), ("fasta1k", 1, 0)):
    t, n_records = synth(kind, gb * 1e9)
    cfg = {"LineWidth": 60 if fmt == 0 else 0}
    for name, o in (("by ID", {}), ("-n", {"ByName": True})):
        opts = dict(o, Config=cfg)
        one, want = one_call(t, fmt, opts)
        for nb in (1, 4, 16):
            leg, got = in_buckets(t, fmt, opts, nb)
            leg["exact"] = bool(got is not None and got.numel() == want.numel() and torch.equal(got, want))
            leg["ratio_to_one_call"] = round(leg["ms"] / one["ms"], 3)
            leg["one call"] = one
            res["%s rename %s, %d bucket(s) asked" % (label, name, nb)] = leg
            print(label, "rename", name, nb, json.dumps(leg), file=sys.stderr, flush=True)
            del got
        del want
    del t
print(json.dumps({"metric": "rename in buckets of the key next to the one-call rename, HBM-resident synthetic shards (every ID twice)", "gb": gb, "reps": reps,
                  "results": res}))
