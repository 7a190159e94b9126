#!/usr/bin/env python3
"""`pair` in buckets of the key next to the one-call `pair`, on two HBM-resident synthetic FASTQ-150 files that fit the device
(1 GPU): file 1 is a shard from bsk_synth_device, file 2 its first three quarters -- every record of file 2 has a mate, the last
quarter of file 1 has none -- as it stands ("in order": file 2 is in mate order and the emit pass prints paired.2) or shuffled by
bsk_shuffle_run ("shuffled": paired.2 comes from the order buckets).  The one call is bsk_pair_run on the two files back to back,
with SaveUnpaired.  The bucket path runs through one context: the histogram of the fine bins over both files, bsk_shuffle_plan with
a budget of 1/N of the histogram's bytes plus the largest fine bin for N = 1, 4 and 16, the verdict, begin / add of both files /
finish per match bucket, the rank step, the emit over both files and -- shuffled -- the order histogram over file 2, its plan for
the same N and begin / add of file 2 / finish per order bucket.  `reads` states how often either file was read.  Every one of
the four bucketed outputs is compared byte for byte (`exact`) with the one-call output in the same run.  Per leg: median ms over the
repetitions, the spread (max - min) / median, `ratio_to_one_call`, the pairs and the flagged records, and the per-stage device
times of bsk_profile_dump (one extra profiled call).  Nothing about the speed of this path has been tuned.  Prints one JSON
object.  Not the driver's bench (that is bench.py).
  python scripts/bench_pair_buckets.py [GB of file 1, default 1] [reps, default 3]"""
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
OPTS = json.dumps({"SaveUnpaired": True})


def one_call(t, n1):
    outs = (_lib.Out * 4)()
    with bsk.Operator("Pair", OPTS, 0) as op:
        def run(keep):
            check(lib.bsk_pair_run(op.ctx, C.c_void_p(t.data_ptr()), t.numel(), n1, 1, FMT, None, outs), op.ctx)
            torch.cuda.synchronize()
            return [device_copy(outs[k]) for k in range(4)] if keep else None
        leg = measure(run, reps)
        got = profiled(op, run, leg)
    return leg, got


def in_buckets(t, n1, nb):
    files = ((C.c_void_p(t.data_ptr()), n1), (C.c_void_p(t.data_ptr() + n1), t.numel() - n1))
    info = {}
    with bsk.Operator("Pair", OPTS, 0) as op:
        def run(keep):
            k, r, f, ordered = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
            reads = [0, 0]
            check(lib.bsk_pair_hist_reset(op.ctx), op.ctx)
            counts = []
            for pid, (ptr, n) in enumerate(files):
                check(lib.bsk_pair_hist_run(op.ctx, ptr, n, 1, FMT, pid, sum(counts), None, C.byref(k)), op.ctx)
                counts.append(k.value)
                reads[pid] += 1
            hb, _ = bsk.PairHistGet(op)
            bounds = bsk.ShufflePlan(hb, sum(hb) // nb + max(hb))
            bsk.PairVerdictBegin(op, counts)
            flagged = 0
            for lo, hi in zip(bounds[:-1], bounds[1:]):
                check(lib.bsk_pair_bucket_begin(op.ctx, lo, hi), op.ctx)
                for pid, (ptr, n) in enumerate(files):
                    check(lib.bsk_pair_bucket_add(op.ctx, ptr, n, 1, FMT, pid, sum(counts[:pid]), None), op.ctx)
                    reads[pid] += 1
                check(lib.bsk_pair_bucket_finish(op.ctx, None, C.byref(r), C.byref(f)), op.ctx)
                flagged += f.value
            check(lib.bsk_pair_order_begin(op.ctx, None, C.byref(r), C.byref(ordered)), op.ctx)
            got = [None] * 4
            outs = (_lib.Out * 3)()
            for pid, (ptr, n) in enumerate(files):
                check(lib.bsk_pair_emit_run(op.ctx, ptr, n, 1, FMT, pid, sum(counts[:pid]), None, outs), op.ctx)
                reads[pid] += 1
                if keep:
                    got[2 + pid] = device_copy(outs[1])
                    got[pid] = device_copy(outs[2 * pid])
            order_buckets = 0
            if r.value and not ordered.value:
                ptr, n = files[1]
                check(lib.bsk_pair_order_hist_run(op.ctx, ptr, n, 1, FMT, 1, counts[0], None, C.byref(k)), op.ctx)
                reads[1] += 1
                ob, _ = bsk.PairOrderHistGet(op)
                obounds = bsk.ShufflePlan(ob, sum(ob) // nb + max(ob))
                shares = []
                out = _lib.Out()
                for lo, hi in zip(obounds[:-1], obounds[1:]):
                    check(lib.bsk_pair_order_bucket_begin(op.ctx, lo, hi), op.ctx)
                    check(lib.bsk_pair_order_bucket_add(op.ctx, ptr, n, 1, FMT, 1, counts[0], None), op.ctx)
                    reads[1] += 1
                    check(lib.bsk_pair_order_bucket_finish(op.ctx, None, C.byref(out)), op.ctx)
                    if keep:
                        shares.append(device_copy(out))
                order_buckets = len(obounds) - 1
                if keep:
                    got[1] = torch.cat(shares)
            torch.cuda.synchronize()
            info.update(buckets=len(bounds) - 1, order_buckets=order_buckets, records=counts, pairs=r.value, flagged=flagged,
                        in_mate_order=bool(ordered.value), reads={"file 1": reads[0], "file 2": reads[1]})
            return got if keep else None
        leg = measure(run, reps)
        got = profiled(op, run, leg)
    leg.update(info)
    return leg, got


res = {}
for label, shuffled in (("in order", False), ("shuffled", True)):
    t, n1 = synth_two_files(gb * 1e9, 3, shuffled)  # (file 2: three quarters of file 1)
    one, want = one_call(t, n1)
    for nb in (1, 4, 16):
        leg, got = in_buckets(t, n1, nb)
        leg["exact"] = all(g is not None and g.numel() == w.numel() and torch.equal(g, w) for g, w in zip(got, want))
        leg["ratio_to_one_call"] = round(leg["ms"] / one["ms"], 3)
        leg["one call"] = one
        res["fastq150 pair, mates %s, %d bucket(s) asked" % (label, nb)] = leg
        print(label, nb, json.dumps(leg), file=sys.stderr, flush=True)
        del got
    del want, t
print(json.dumps({"metric": "pair in buckets of the key next to the one-call pair, two HBM-resident synthetic FASTQ-150 files (file 2 = the first three "
                            "quarters of file 1, as it stands or shuffled), SaveUnpaired",
                  "gb": gb, "reps": reps, "input_bytes": int(gb * 1e9) // 4 * 7, "results": res}))
