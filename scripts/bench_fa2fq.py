#!/usr/bin/env python3
"""`fa2fq` on an HBM-resident synthetic FASTQ-150 shard (1 GPU) with a FASTA file made from it: ms per call, bytes read
(shard) and written, algorithmic GB/s, the fraction of the 8 TB/s peak, and `exact` -- the output compared byte for byte
with the answer built independently (numpy, from the fixed record layout).  Three cases: every read present and trimmed by
a few bases at each end; the same with every second needle taken from the reverse complement; one read in a hundred
present.  `subseq -r` of the same slice on the same shard is timed beside them as the yardstick of a pass that reads a
record and writes a slice of it.  Prints one JSON object.  Not the driver's bench (that is bench.py).
  python scripts/bench_fa2fq.py [GB of shard, default 2] [reps, default 3]"""
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bigseqkit_amd as bsk
from bigseqkit_amd import _lib
from bigseqkit_amd._lib import lib, check

gb = float(sys.argv[1]) if len(sys.argv) > 1 else 2.0
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
rng = np.random.default_rng(1)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
LO, HI = 3, 146  # the FASTA sequence of a read is its bases [LO, HI): trimmed by 3 and by 4


def digits(v, width):  # (N,) ints -> (N, width) ASCII, zero-padded
    out = np.empty((len(v), width), dtype=np.uint8)
    for k in range(width - 1, -1, -1):
        out[:, k] = 48 + v % 10
        v = v // 10
    return out


def records(parts):
    return np.concatenate(parts, axis=1).reshape(-1)


def lit(s, n):
    return np.broadcast_to(np.frombuffer(s, dtype=np.uint8), (n, len(s)))


def timed(name, run_fn, opts, t):
    out = _lib.Out()
    with bsk.Operator(name, json.dumps(opts), 0) as op:
        call = lambda: check(run_fn(op.ctx, C.c_void_p(t.data_ptr()), t.numel(), 1, 1, 0, None, C.byref(out)), op.ctx)
        call()  # (uploads the table, sizes the buffers)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
            torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        host = np.empty(max(1, out.len), dtype=np.uint8)
        check(lib.bsk_out_to_host(op.ctx, C.byref(out), host.ctypes.data_as(C.c_void_p), out.len), op.ctx)
    return dt, host[:out.len]


res = {}


def report(name, nrec, data, dt, got, expect):
    alg = data.size + got.size
    res[name] = {"records": nrec, "in_GB": round(data.size / 1e9, 3), "out_GB": round(got.size / 1e9, 3), "ms": round(dt * 1e3, 2),
                 "algorithmic_GBps": round(alg / dt / 1e9, 1), "frac_of_8TBps": round(alg / dt / 8e12, 4),
                 "exact": bool(got.size == expect.size and np.array_equal(got, expect))}
    print(name, json.dumps(res[name]), file=sys.stderr, flush=True)


# FASTQ-150, header @S%010d: 317 bytes per record
n = int(gb * 1e9) // 317
ids = np.arange(n, dtype=np.int64)
seq = ACGT[rng.integers(0, 4, size=(n, 150), dtype=np.uint8)]
qual = rng.integers(ord("5"), ord("J"), size=(n, 150), dtype=np.uint8)
nl = lit(b"\n", n)
name = digits(ids, 10)
fq = records([lit(b"@S", n), name, nl, seq, lit(b"\n+\n", n), qual, nl])
comp = np.arange(256, dtype=np.uint8)
comp[list(b"ACGT")] = list(b"TGCA")
s_plus, q_plus = seq[:, LO:HI], qual[:, LO:HI]
s_minus, q_minus = comp[s_plus[:, ::-1]], q_plus[:, ::-1]
odd = (ids % 2 == 1)[:, None]
s_half, q_half = np.where(odd, s_minus, s_plus), np.where(odd, q_minus, q_plus)
t = torch.from_numpy(fq).cuda()
tmp = tempfile.mkdtemp(prefix="bench_fa2fq_")
cases = (("all_trimmed", s_plus, q_plus, np.ones(n, bool)), ("half_reverse_complement", s_half, q_half, np.ones(n, bool)),
         ("one_in_a_hundred", s_plus, q_plus, ids % 100 == 0))
for case, s, q, keep in cases:
    k = int(keep.sum())
    path = os.path.join(tmp, case + ".fa")
    records([lit(b">S", k), name[keep], nl[:k], s[keep], nl[:k]]).tofile(path)
    want = records([lit(b"@S", k), name[keep], nl[:k], s[keep], lit(b"\n+\n", k), q[keep], nl[:k]])
    dt, got = timed("Fa2Fq", lib.bsk_fa2fq_run, {"Config": {"Quiet": True, "SeqType": "dna"}, "FastaFile": path}, t)
    report(case, n, fq, dt, got, want)
    os.remove(path)
    del want, got
os.rmdir(tmp)
# the yardstick: subseq -r LO+1:HI writes the same slice of every record (whole header)
want = records([lit(b"@S", n), name, nl, s_plus, lit(b"\n+\n", n), q_plus, nl])
dt, got = timed("SubseqTransform", lib.bsk_subseq_run, {"Config": {"Quiet": True}, "Region": "%d:%d" % (LO + 1, HI)}, t)
report("subseq_region_yardstick", n, fq, dt, got, want)
print(json.dumps({"metric": "fa2fq on an HBM-resident FASTQ-150 shard", "gb": gb, "reps": reps, "results": res}))
