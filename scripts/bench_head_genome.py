#!/usr/bin/env python3
"""`head-genome` on an HBM-resident synthetic shard (1 GPU): a FASTA-1k shard from bsk_synth_device whose header texts are
rewritten in place, same length, to ">r G dddd" (first genome: the prefix is "G 0000", every other record shares one word)
and ">r H dddd" from record `cut` on (no shared word: the cut).  Legs: the cut after 10 records, after 10^4 and never
(every record kept), each with growing windows (the default) and with one window over the whole shard
(head_genome_window = 0).  Yardsticks on the same shard in the same run: `head -n <cut>` (the same bytes out, found by
counting instead of comparing) and `seq` without options on the whole shard (what reading and printing everything costs).
Every output is compared byte for byte (`exact`) with the rows of the fixed layout.  Per leg: median ms, the spread
(max - min) / median, the per-stage device times and the bytes the window index passes read (bsk_profile_dump, one extra
profiled call).  Prints one JSON object.  Not the driver's bench (that is bench.py).
  python scripts/bench_head_genome.py [GB, default 2] [reps, default 5]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bigseqkit_amd as bsk
from bigseqkit_amd import _lib
from bigseqkit_amd._lib import lib, check

gb = float(sys.argv[1]) if len(sys.argv) > 1 else 2.0
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5

rb = lib.bsk_synth_record_bytes(1)
n = int(gb * 1e9) // rb
t = torch.empty(n * rb, dtype=torch.uint8, device="cuda")
check(lib.bsk_synth_device(1, 42, 0, 0, C.c_void_p(t.data_ptr()), n * rb, 0, None))
rows = t.view(n, rb)
idx = torch.arange(n, device="cuda")
num = torch.where(idx == 0, torch.zeros_like(idx), idx % 9000 + 1000)
for k in range(4):
    rows[:, 5 + k] = (48 + (num // 10 ** (3 - k)) % 10).to(torch.uint8)
rows[:, 1:5] = torch.tensor(list(b"r G "), dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()


def timed(op_name, fn, opts, switches=()):
    out = _lib.Out()
    with bsk.Operator(op_name, json.dumps(opts), 0) as op:
        for k, v in switches:
            check(lib.bsk_ctx_set(op.ctx, k.encode(), v.encode()), op.ctx)

        def call():
            if op_name == "HeadGenome":
                check(lib.bsk_head_genome_reset(op.ctx), op.ctx)
            check(fn(op.ctx, C.c_void_p(t.data_ptr()), t.numel(), 1, 0, 0, None, C.byref(out)), op.ctx)
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
                stages[k] = int(v.split("/")[1]) if k == "hg_indexed_bytes" else round(float(v.split("/")[0]), 3)
        got = torch.empty(out.len, dtype=torch.uint8, device="cuda")
        if out.len:
            check(lib.bsk_device_copy(C.c_void_p(got.data_ptr()), out.d_data, out.len, 3))
    ms.sort()
    med = ms[len(ms) // 2]
    return {"ms": round(med, 3), "spread": round((ms[-1] - ms[0]) / med, 3), "stages": stages, "out_GB": round(out.len / 1e9, 3)}, got


range_fn = lambda ctx, p, nb, dev, fmt, pid, st, out: lib.bsk_range_run(ctx, p, nb, dev, fmt, pid, 0, st, out)
res = {}
seq_leg, got = timed("SeqTransform", lib.bsk_seq_run, {})
seq_leg["exact"] = bool(torch.equal(got, t))
res["yardstick seq, whole shard"] = seq_leg
del got
for cut in (10, 10 ** 4, n):
    cut = min(cut, n)
    if cut < n:
        rows[cut:, 3] = ord("H")
    torch.cuda.synchronize()
    want = rows[:cut].reshape(-1)
    for label, sw in (("windows", ()), ("one window", (("head_genome_window", "0"),))):
        leg, got = timed("HeadGenome", lib.bsk_head_genome_run, {}, sw)
        leg["exact"] = bool(got.numel() == want.numel() and torch.equal(got, want))
        res["cut after %d, %s" % (cut, label)] = leg
        print(cut, label, json.dumps(leg), file=sys.stderr, flush=True)
    yard, got = timed("Head", range_fn, {"N": cut})
    yard["exact"] = bool(got.numel() == want.numel() and torch.equal(got, want))
    res["cut after %d, yardstick head -n" % cut] = yard
    rows[:, 3] = ord("G")
    del got, want
print(json.dumps({"metric": "head-genome on an HBM-resident FASTA-1k shard", "gb": gb, "reps": reps, "records": n, "results": res}))
