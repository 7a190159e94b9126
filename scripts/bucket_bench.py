"""What the bucket benchmarks share (bench_{sort,rmdup,rename,common,pair,concat}_buckets.py, bench_bucket_calls.py): the synthetic
shards in HBM, the timing of a leg, its profiled extra call and the copy of a result.  Importing it puts the repository root on
sys.path, so the scripts import bigseqkit_amd after it."""
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


def synth_at(kind, t, at, n):
    """n bytes of the synthetic file `kind` from its start, written to t[at:]"""
    check(lib.bsk_synth_device(kind, 42, 0, 0, C.c_void_p(t.data_ptr() + at), n, 0, None))


def synth(kind, nbytes):
    """one shard of whole records: (tensor, records)"""
    rb = lib.bsk_synth_record_bytes(kind)
    n = int(nbytes) // rb * rb
    t = torch.empty(n, dtype=torch.uint8, device="cuda")
    synth_at(kind, t, 0, n)
    torch.cuda.synchronize()
    return t, n // rb


def synth_two_files(nbytes, share2, shuffled):
    """FASTQ-150: file 1 and, behind it in one tensor, file 2 = the first share2 (in quarters) of file 1, as it stands or
    shuffled: (tensor, bytes of file 1)"""
    rb = lib.bsk_synth_record_bytes(0)
    n1 = int(nbytes) // (4 * rb) * 4 * rb
    n2 = n1 // 4 * share2
    t = torch.empty(n1 + n2, dtype=torch.uint8, device="cuda")
    synth_at(0, t, 0, n1)
    if shuffled:
        out = _lib.Out()
        with bsk.Operator("Shuffle", json.dumps({"Seed": 11}), 0) as op:
            check(lib.bsk_shuffle_run(op.ctx, C.c_void_p(t.data_ptr()), n2, 1, 1, 0, None, C.byref(out)), op.ctx)
            assert out.len == n2
            check(lib.bsk_device_copy(C.c_void_p(t.data_ptr() + n1), out.d_data, n2, 3))
    else:
        synth_at(0, t, n1, n2)
    torch.cuda.synchronize()
    return t, n1


def stages_of(op):
    pb = C.create_string_buffer(1 << 16)
    check(lib.bsk_profile_dump(op.ctx, pb, len(pb)), op.ctx)
    stages = {}
    for item in pb.value.decode().split(";"):
        if "=" in item:
            k, v = item.rsplit("=", 1)
            stages[k] = round(float(v.split("/")[0]), 3)
    return stages


def device_copy(out):
    got = torch.empty(out.len, dtype=torch.uint8, device="cuda")
    if out.len:
        check(lib.bsk_device_copy(C.c_void_p(got.data_ptr()), out.d_data, out.len, 3))
    return got


def measure(run, reps):
    run(False)  # (sizes the buffers)
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run(False)
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    med = ms[len(ms) // 2]
    return {"ms": round(med, 3), "spread": round((ms[-1] - ms[0]) / med, 3)}


def profiled(op, run, leg):
    lib.bsk_profile_reset(op.ctx)
    lib.bsk_profile_enable(op.ctx, 1)
    got = run(True)
    leg["stages_ms"] = stages_of(op)
    return got
