#!/usr/bin/env python3
"""`replace` on HBM-resident synthetic shards (1 GPU): ms per call, algorithmic GB/s (bytes in + bytes out), the
fraction of the 8 TB/s peak, and `exact` -- the output compared byte for byte with the answer built independently
(numpy, from the fixed record layout).  Prints one JSON object.  Not the driver's bench (that is bench.py).
  python scripts/bench_replace.py [GB per shard, default 4] [reps, default 3]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bigseqkit_amd as bsk
from bigseqkit_amd import _lib
from bigseqkit_amd._lib import lib, check

gb = float(sys.argv[1]) if len(sys.argv) > 1 else 4.0
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
rng = np.random.default_rng(1)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def digits(v, width):  # (N,) ints -> (N, width) ASCII, zero-padded
    out = np.empty((len(v), width), dtype=np.uint8)
    for k in range(width - 1, -1, -1):
        out[:, k] = 48 + v % 10
        v = v // 10
    return out


def records(parts):  # list of (N, w) arrays -> flat bytes of the concatenated rows
    return np.concatenate(parts, axis=1).reshape(-1)


def lit(s, n):
    return np.broadcast_to(np.frombuffer(s, dtype=np.uint8), (n, len(s)))


def run(opts, data, fmt, env=None):
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        t = torch.from_numpy(data).cuda()
        out = _lib.Out()
        with bsk.Operator("Replace", json.dumps(opts), 0) as op:
            check(lib.bsk_replace_run(op.ctx, C.c_void_p(t.data_ptr()), t.numel(), 1, fmt, 0, None, C.byref(out)), op.ctx)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                check(lib.bsk_replace_run(op.ctx, C.c_void_p(t.data_ptr()), t.numel(), 1, fmt, 0, None, C.byref(out)), op.ctx)
                torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / reps
            host = np.empty(max(1, out.len), dtype=np.uint8)
            check(lib.bsk_out_to_host(op.ctx, C.byref(out), host.ctypes.data_as(C.c_void_p), out.len), op.ctx)
        del t
        torch.cuda.empty_cache()
        return dt, host[:out.len], out.records
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


res = {}


def report(name, nrec, data, dt, got, expect):
    alg = data.size + got.size
    res[name] = {"records": nrec, "in_GB": round(data.size / 1e9, 2), "out_GB": round(got.size / 1e9, 3), "ms": round(dt * 1e3, 2),
                 "algorithmic_GBps": round(alg / dt / 1e9, 1), "frac_of_8TBps": round(alg / dt / 8e12, 4),
                 "exact": bool(got.size == expect.size and np.array_equal(got, expect))}
    print(name, json.dumps(res[name]), file=sys.stderr, flush=True)


# FASTQ-150, header @S%010d: 317 bytes per record
n = int(gb * 1e9) // 317
ids = np.arange(n, dtype=np.int64)
seq = ACGT[rng.integers(0, 4, size=(n, 150), dtype=np.uint8)]
qual = np.full((n, 150), ord("I"), dtype=np.uint8)
nl = lit(b"\n", n)
fq = records([lit(b"@S", n), digits(ids, 10), nl, seq, lit(b"\n+\n", n), qual, nl])
del seq
want = records([lit(b"@read_", n), digits(ids, 10), lit(b"_", n), digits(ids + 1, 9), nl,
                fq.reshape(n, 317)[:, 13:]])
opts = {"Pattern": "^S(\\d+)", "Replacement": "read_${1}_{nr}", "NrWidth": 9}
dt, got, k = run(opts, fq, 1)
report("fastq150_name_nr", n, fq, dt, got, want)
del want, got
dt, got, k = run({"Pattern": "^Z(\\d+)", "Replacement": "x"}, fq, 1)
report("fastq150_name_nomatch", n, fq, dt, got, fq)
del fq, got

# FASTA-5k CDS ">cds%08d len=5001", wrapped at 60
n = int(gb * 1e9) // 5104
L = 5001
body = ACGT[rng.integers(0, 4, size=(n, L), dtype=np.uint8)]
lines = [body[:, k:k + 60] for k in range(0, L, 60)]
wrapped = np.concatenate([np.concatenate([x, lit(b"\n", n)], axis=1) for x in lines], axis=1)
del body, lines
ids = np.arange(n, dtype=np.int64)
fa = records([lit(b">cds", n), digits(ids, 8), lit(b" len=5001\n", n), wrapped])
want = records([lit(b">cds", n), digits(ids, 8), lit(b"\n", n), wrapped])
del wrapped
dt, got, k = run({"Pattern": "\\s.+", "Replacement": ""}, fa, 0)
report("fasta5k_name_strip", n, fa, dt, got, want)
del fa, want, got

# FASTA-1k, one line per sequence (-w 0): -s on the per-byte path and on the Pike VM (BSK_REPLACE=vm)
n = int(gb * 1e9) // 1012
ids = np.arange(n, dtype=np.int64)
seq = ACGT[rng.integers(0, 4, size=(n, 1000), dtype=np.uint8)]
nl = lit(b"\n", n)
fa = records([lit(b">r", n), digits(ids, 8), nl, seq, nl])
head = records([lit(b">r", n), digits(ids, 8), nl]).reshape(n, 11)
tu = records([head, np.where(seq == ord("T"), ord("U"), seq).astype(np.uint8), nl])
keep = (seq != ord("G")) & (seq != ord("C"))
# (every row keeps a different number of bases: a mask over the whole rows)
flat = np.concatenate([head, seq, nl], axis=1)
mask = np.concatenate([np.ones((n, 11), bool), keep, np.ones((n, 1), bool)], axis=1)
gc = flat[mask]
gc_end = np.cumsum(12 + keep.sum(axis=1))  # end of record i in gc
del flat, mask, keep, seq
base = {"Config": {"LineWidth": 0}, "BySeq": True}
m = n // 64  # the Pike VM path (one lane per record, slow): the first 1/64 of the records
for name, opts, expect, end_m in (("fasta1k_seq_T_to_U", dict(base, Pattern="T", Replacement="U"), tu, m * 1012),
                                  ("fasta1k_seq_drop_GC", dict(base, Pattern="[GC]", Replacement=""), gc, int(gc_end[m - 1]))):
    dt, got, k = run(opts, fa, 0)
    report(name, n, fa, dt, got, expect)
    small = fa[:m * 1012]
    dt, got, k = run(opts, small, 0, {"BSK_REPLACE": "vm"})
    report(name + "_vm_1_64", m, small, dt, got, expect[:end_m])
print(json.dumps({"metric": "replace on HBM-resident shards", "gb_per_shard": gb, "reps": reps, "results": res}))
