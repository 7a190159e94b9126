#!/usr/bin/env python3
"""Host time of the call sequence of `shuffle` in buckets (bsk_shuffle_hist_run, then bsk_shuffle_bucket_begin / _add / _finish
per bucket) on an HBM-resident synthetic shard: wall clock per call, each call followed by a device synchronisation, next to
the device time of its stages.  What bench_sample.py --buckets reports as one number is split here by entry point, so that a
change in the host side of one of them shows where it is.  Prints one JSON object: per shard the median over the repetitions
of the whole sequence and of every call kind (summed over the buckets), and the sum of the device stages of one profiled run.
  python scripts/bench_bucket_calls.py [GB per shard, default 2] [reps, default 9] [--buckets N, default 4]"""
import ctypes as C
import json
import sys
import time

from bucket_bench import synth
import torch
import bigseqkit_amd as bsk
from bigseqkit_amd import _lib
from bigseqkit_amd._lib import lib, check

argv = sys.argv[1:]
nb = 4
if "--buckets" in argv:
    at = argv.index("--buckets")
    nb = int(argv[at + 1])
    del argv[at:at + 2]
gb = float(argv[0]) if len(argv) > 0 else 2.0
reps = int(argv[1]) if len(argv) > 1 else 9


def med(v):
    v = sorted(v)
    return round(v[len(v) // 2], 4)


res = {}
for label, kind, fmt in (("fastq150", 0, 1), ("fasta1k", 1, 0)):
    t, _ = synth(kind, gb * 1e9)
    ptr, n = C.c_void_p(t.data_ptr()), t.numel()
    out = _lib.Out()
    with bsk.Operator("Shuffle", "{}", 0) as op:
        def run():
            w = {"hist_reset": 0.0, "hist_run": 0.0, "hist_get+plan": 0.0, "begin": 0.0, "add": 0.0, "finish": 0.0}

            def timed(name, f):
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                w[name] += (time.perf_counter() - t0) * 1e3
            k = C.c_uint64()
            t_all = time.perf_counter()
            timed("hist_reset", lambda: check(lib.bsk_shuffle_hist_reset(op.ctx), op.ctx))
            timed("hist_run", lambda: check(lib.bsk_shuffle_hist_run(op.ctx, ptr, n, 1, fmt, 0, 0, None, C.byref(k)), op.ctx))
            bounds = []

            def plan():
                hb, _ = bsk.ShuffleHistGet(op)
                bounds.extend(bsk.ShufflePlan(hb, sum(hb) // nb + max(hb)))
            timed("hist_get+plan", plan)
            for lo, hi in zip(bounds[:-1], bounds[1:]):
                timed("begin", lambda: check(lib.bsk_shuffle_bucket_begin(op.ctx, lo, hi), op.ctx))
                timed("add", lambda: check(lib.bsk_shuffle_bucket_add(op.ctx, ptr, n, 1, fmt, 0, 0, None), op.ctx))
                timed("finish", lambda: check(lib.bsk_shuffle_bucket_finish(op.ctx, None, C.byref(out)), op.ctx))
            w["all"] = (time.perf_counter() - t_all) * 1e3
            w["buckets"] = len(bounds) - 1
            return w
        run()  # (sizes the buffers)
        runs = [run() for _ in range(reps)]
        lib.bsk_profile_reset(op.ctx)
        lib.bsk_profile_enable(op.ctx, 1)
        run()
        pb = C.create_string_buffer(1 << 16)
        check(lib.bsk_profile_dump(op.ctx, pb, len(pb)), op.ctx)
        stages = sum(float(x.rsplit("=", 1)[1].split("/")[0]) for x in pb.value.decode().split(";") if "=" in x)
    row = {k: med([r[k] for r in runs]) for k in runs[0]}
    row["all_min"], row["all_max"] = round(min(r["all"] for r in runs), 4), round(max(r["all"] for r in runs), 4)
    row["device_stage_sum_ms"] = round(stages, 3)
    res[label] = row
    del t
print(json.dumps({"metric": "wall ms per entry point of shuffle in buckets (each call synchronised)", "gb": gb, "reps": reps, "results": res}))
