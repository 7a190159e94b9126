#!/usr/bin/env python3
"""`common` in buckets of the key next to the one-call `common`, on two HBM-resident synthetic files that fit the device (1 GPU):
file 1 is a FASTQ-150 or a FASTA-1k shard from bsk_synth_device and file 2 its first half, so half of the records of file 1 are
common to both; by ID and by sequence (-s).  The one call is bsk_common_run on the two files back to back.  The bucket path runs
through one context: the histogram of the fine bins over both files, bsk_shuffle_plan with a budget of 1/N of the histogram's
bytes plus the largest fine bin for N = 4 and 16, the verdict, begin / add of both files / finish per bucket and one emit pass over
file 1 -- both files are read 1 + N times, file 1 once more.  Every bucketed output is compared byte for byte (`exact`) with the
one-call output in the same run.  Per leg: median ms over the repetitions, the spread (max - min) / median, `ratio_to_one_call`,
the records kept and flagged, and the per-stage device times of bsk_profile_dump (one extra profiled call): k_rmdup_hash and
k_rdb_hist are the histogram pass, k_rdb_pick and k_rdb_pack the collect passes, rmdup_group(sort+dedupe), k_comb_verify and
k_comb_decide the finish, k_comb_apply, k_sizes_scan and the emit kernel the emit.  Nothing about the speed of this path has been
tuned.  Prints one JSON object.  Not the driver's bench (that is bench.py).
  python scripts/bench_common_buckets.py [GB of file 1, default 1] [reps, default 3]"""
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
    """file 1 and, behind it in one tensor, its first half as file 2: (tensor, bytes of file 1)"""
    rb = lib.bsk_synth_record_bytes(kind)
    half = int(nbytes) // (2 * rb) * rb
    t = torch.empty(3 * half, dtype=torch.uint8, device="cuda")
    synth_at(kind, t, 0, 2 * half)
    synth_at(kind, t, 2 * half, half)
    torch.cuda.synchronize()
    return t, 2 * half


def one_call(t, n_first, fmt, opts):
    out = _lib.Out()
    ends = (C.c_uint64 * 2)(n_first, t.numel())
    with bsk.Operator("Common", json.dumps(opts), 0) as op:
        def run(keep):
            check(lib.bsk_common_run(op.ctx, C.c_void_p(t.data_ptr()), t.numel(), ends, 2, 1, fmt, None, C.byref(out)), op.ctx)
            torch.cuda.synchronize()
            return device_copy(out) if keep else None
        leg = measure(run, reps)
        got = profiled(op, run, leg)
    return leg, got


def in_buckets(t, n_first, fmt, opts, nb):
    files = ((C.c_void_p(t.data_ptr()), n_first), (C.c_void_p(t.data_ptr() + n_first), t.numel() - n_first))
    out = _lib.Out()
    info = {}
    with bsk.Operator("Common", json.dumps(opts), 0) as op:
        def run(keep):
            k, r, f = C.c_uint64(), C.c_uint64(), C.c_uint64()
            check(lib.bsk_common_hist_reset(op.ctx), op.ctx)
            counts = []
            for pid, (ptr, n) in enumerate(files):
                check(lib.bsk_common_hist_run(op.ctx, ptr, n, 1, fmt, pid, sum(counts), None, C.byref(k)), op.ctx)
                counts.append(k.value)
            hb, _ = bsk.CommonHistGet(op)
            bounds = bsk.ShufflePlan(hb, sum(hb) // nb + max(hb))
            bsk.CommonVerdictBegin(op, counts)
            kept = flagged = 0
            for lo, hi in zip(bounds[:-1], bounds[1:]):
                check(lib.bsk_common_bucket_begin(op.ctx, lo, hi), op.ctx)
                for pid, (ptr, n) in enumerate(files):
                    check(lib.bsk_common_bucket_add(op.ctx, ptr, n, 1, fmt, pid, sum(counts[:pid]), None), op.ctx)
                check(lib.bsk_common_bucket_finish(op.ctx, None, C.byref(r), C.byref(f)), op.ctx)
                kept, flagged = kept + r.value, flagged + f.value
            check(lib.bsk_common_emit_run(op.ctx, files[0][0], files[0][1], 1, fmt, 0, 0, None, C.byref(out)), op.ctx)
            torch.cuda.synchronize()
            info.update(buckets=len(bounds) - 1, records=counts, kept=kept, flagged=flagged, subject_share=round(sum(hb) / max(1, t.numel()), 4),
                        largest_bin_share=round(max(hb) / max(1, sum(hb)), 4))
            return device_copy(out) if keep else None
        leg = measure(run, reps)
        got = profiled(op, run, leg)
    leg.update(info)
    return leg, got


res = {}
for label, kind, fmt in (("fastq150", 0, 1), ("fasta1k", 1, 0)):
    t, n_first = synth(kind, gb * 1e9)
    cfg = {"LineWidth": 60 if fmt == 0 else 0}
    for name, o in (("by ID", {}), ("-s", {"BySeq": True})):
        opts = dict(o, Config=cfg)
        one, want = one_call(t, n_first, fmt, opts)
        for nb in (4, 16):
            leg, got = in_buckets(t, n_first, fmt, opts, nb)
            leg["exact"] = bool(got is not None and got.numel() == want.numel() and torch.equal(got, want))
            leg["ratio_to_one_call"] = round(leg["ms"] / one["ms"], 3)
            leg["one call"] = one
            res["%s common %s, %d bucket(s) asked" % (label, name, nb)] = leg
            print(label, "common", name, nb, json.dumps(leg), file=sys.stderr, flush=True)
            del got
        del want
    del t
print(json.dumps({"metric": "common in buckets of the key next to the one-call common, two HBM-resident synthetic files (file 2 = the first half of file 1)",
                  "gb": gb, "reps": reps, "input_bytes": int(gb * 1e9) // 2 * 3, "results": res}))
