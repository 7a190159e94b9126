#!/usr/bin/env python3
"""`concat` in buckets of the key next to the one-call `concat`, on two HBM-resident synthetic FASTQ-150 files with unique IDs that
fit the device (1 GPU): file 1 is a shard from bsk_synth_device, file 2 the same records -- every record has one mate, the output is
linear -- as they stand ("in order") or shuffled by bsk_shuffle_run ("shuffled").  The one call is bsk_concat_run on the two files
back to back.  The bucket path runs through one context: the histogram of the fine bins over both files, bsk_shuffle_plan with a
budget of 1/N of the histogram's bytes plus the largest fine bin for N = 1, 4 and 16, the verdict, begin / add of both files / finish
per match bucket, the join step, the weights over file 2, the window histogram over file 1, its plan for the same N and begin / add of
both files / finish per window.  Either file is ONE shard here, so every window reads file 1 whole; a driver that cuts file 1 into
pieces skips those outside the window.  `reads` states how often either file was read.  The windows' shares, joined, are compared
byte for byte (`exact`) with the one-call output in the same run.  Per leg: median ms over the repetitions, the spread
(max - min) / median, `ratio_to_one_call`, the records with a head and the flagged records, and the per-stage device times of
bsk_profile_dump (one extra profiled call).  Nothing about the speed of this path has been tuned.  Prints one JSON object.  Not the
driver's bench (that is bench.py).
  python scripts/bench_concat_buckets.py [GB of either file, default 1] [reps, default 3]"""
import ctypes as C
import json
import sys

from bucket_bench import synth_two_files, device_copy, measure, profiled
import torch
import bigseqkit_amd as bsk
from bigseqkit_amd import _lib
from bigseqkit_amd._lib import lib, check

argv = sys.argv[1:]
gb = float(argv[0]) if len(argv) > 0 else 1.0
reps = int(argv[1]) if len(argv) > 1 else 3
FMT = 1  # FASTQ
OPTS = json.dumps({"Full": False})


def one_call(t, n1):
    out = _lib.Out()
    with bsk.Operator("Concat", OPTS, 0) as op:
        def run(keep):
            check(lib.bsk_concat_run(op.ctx, C.c_void_p(t.data_ptr()), t.numel(), n1, 1, FMT, None, C.byref(out)), op.ctx)
            torch.cuda.synchronize()
            return device_copy(out) if keep else None
        leg = measure(run, reps)
        got = profiled(op, run, leg)
    return leg, got


def in_buckets(t, n1, nb):
    files = ((C.c_void_p(t.data_ptr()), n1), (C.c_void_p(t.data_ptr() + n1), t.numel() - n1))
    info = {}
    with bsk.Operator("Concat", OPTS, 0) as op:
        def run(keep):
            k, r, f = C.c_uint64(), C.c_uint64(), C.c_uint64()
            reads = [0, 0]
            check(lib.bsk_concat_hist_reset(op.ctx), op.ctx)
            counts = []
            for pid, (ptr, n) in enumerate(files):
                check(lib.bsk_concat_hist_run(op.ctx, ptr, n, 1, FMT, pid, sum(counts), None, C.byref(k)), op.ctx)
                counts.append(k.value)
                reads[pid] += 1
            hb, _ = bsk.ConcatHistGet(op)
            bounds = bsk.ShufflePlan(hb, sum(hb) // nb + max(hb))
            bsk.ConcatVerdictBegin(op, counts)
            matched = flagged = 0
            for lo, hi in zip(bounds[:-1], bounds[1:]):
                check(lib.bsk_concat_bucket_begin(op.ctx, lo, hi), op.ctx)
                for pid, (ptr, n) in enumerate(files):
                    check(lib.bsk_concat_bucket_add(op.ctx, ptr, n, 1, FMT, pid, sum(counts[:pid]), None), op.ctx)
                    reads[pid] += 1
                check(lib.bsk_concat_bucket_finish(op.ctx, None, C.byref(r), C.byref(f)), op.ctx)
                matched += r.value
                flagged += f.value
            bsk.ConcatJoinBegin(op)
            check(lib.bsk_concat_weigh_run(op.ctx, files[1][0], files[1][1], 1, FMT, 1, counts[0], None, C.byref(k)), op.ctx)
            reads[1] += 1
            check(lib.bsk_concat_window_hist_run(op.ctx, files[0][0], files[0][1], 1, FMT, 0, 0, None, C.byref(k)), op.ctx)
            reads[0] += 1
            wb, _ = bsk.ConcatWindowHistGet(op)
            wbounds = bsk.ShufflePlan(wb, sum(wb) // nb + max(wb))
            shares = []
            out = _lib.Out()
            for lo, hi in zip(wbounds[:-1], wbounds[1:]):
                check(lib.bsk_concat_window_begin(op.ctx, lo, hi), op.ctx)
                for pid, (ptr, n) in enumerate(files):
                    check(lib.bsk_concat_window_add(op.ctx, ptr, n, 1, FMT, pid, sum(counts[:pid]), None), op.ctx)
                    reads[pid] += 1
                check(lib.bsk_concat_window_finish(op.ctx, None, C.byref(out)), op.ctx)
                if keep:
                    shares.append(device_copy(out))
            torch.cuda.synchronize()
            info.update(buckets=len(bounds) - 1, windows=len(wbounds) - 1, records=counts, with_head=matched, flagged=flagged,
                        reads={"file 1": reads[0], "file 2": reads[1]})
            return torch.cat(shares) if keep else None
        leg = measure(run, reps)
        got = profiled(op, run, leg)
    leg.update(info)
    return leg, got


res = {}
for label, shuffled in (("in order", False), ("shuffled", True)):
    t, n1 = synth_two_files(gb * 1e9, 4, shuffled)  # (file 2: as long as file 1)
    one, want = one_call(t, n1)
    for nb in (1, 4, 16):
        leg, got = in_buckets(t, n1, nb)
        leg["exact"] = got.numel() == want.numel() and bool(torch.equal(got, want))
        leg["ratio_to_one_call"] = round(leg["ms"] / one["ms"], 3)
        leg["one call"] = one
        res["fastq150 concat, file 2 %s, %d window(s) asked" % (label, nb)] = leg
        print(label, nb, json.dumps(leg), file=sys.stderr, flush=True)
        del got
    del want, t
print(json.dumps({"metric": "concat in buckets of the key next to the one-call concat, two HBM-resident synthetic FASTQ-150 files with unique IDs "
                            "(file 2 = the records of file 1, as they stand or shuffled)",
                  "gb": gb, "reps": reps, "input_bytes": int(gb * 1e9) * 2, "results": res}))
