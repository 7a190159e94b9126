#!/usr/bin/env python3
"""BGZF input next to the plain load, file -> text in HBM on 1 GPU.  The input is a synthetic FASTQ-150 text (bsk_synth_host) of
`MB` megabytes, compressed with zlib level 6 in blocks of 65 280 text bytes and written `copies` times -- still valid BGZF -- next to
the plain text written as often.  Timed, one after the other in every repetition so that the legs see the same machine:
    bgzf_load      bsk_bgzf_load of the compressed file (bsk_shard_load + inflate)
    plain_load     bsk_shard_load of the plain file: the yardstick
    inflate        bsk_bgzf_inflate_device alone, the compressed bytes already in HBM
Per leg: median ms over the repetitions, the spread (max - min) / median, text GB/s out and, for the compressed legs, compressed
GB/s in and `ratio_to_plain` (its text GB/s over the plain load's).  One more, profiled call gives the device times of the stages
bgzf_find / bgzf_sizes / bgzf_inflate (bsk_profile_dump).  The inflated text is compared with the plain file's bytes once
(`exact`).  Nothing about the speed of this path has been tuned.  Prints one JSON object.  Not the driver's bench (that is bench.py).
  python scripts/bench_bgzf.py [MB of text per copy, default 256] [copies, default 8] [reps, default 3]"""
import ctypes as C
import json
import os
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import bigseqkit_amd as bsk
from bigseqkit_amd._lib import lib, check
import bgzf_ref

argv = sys.argv[1:]
mb = int(argv[0]) if len(argv) > 0 else 256
copies = int(argv[1]) if len(argv) > 1 else 8
reps = int(argv[2]) if len(argv) > 2 else 3
BLOCK = bgzf_ref.MAX_BLOCK


def synth_text(nbytes):
    rb = lib.bsk_synth_record_bytes(0)
    n = nbytes // rb * rb
    buf = C.create_string_buffer(n)
    check(lib.bsk_synth_host(0, 42, 0, 0, buf, n))
    return buf.raw[:n]


def compress(text):
    def one(i):
        piece = text[i:i + BLOCK]
        return bgzf_ref.member(bgzf_ref.deflate(piece, level=6), piece)
    with ThreadPoolExecutor(16) as pool:   # (zlib releases the interpreter lock)
        return b"".join(pool.map(one, range(0, len(text), BLOCK)))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def leg(ms, text_bytes, comp_bytes=None):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    r = {"ms": round(med, 3), "spread": round((ms[-1] - ms[0]) / med, 3), "text_GBps": round(text_bytes / med / 1e6, 2)}
    if comp_bytes:
        r["compressed_GBps"] = round(comp_bytes / med / 1e6, 2)
    return r


def main():
    text = synth_text(mb << 20)
    comp = compress(text)
    with tempfile.TemporaryDirectory() as d:
        fz, fp = os.path.join(d, "x.fq.gz"), os.path.join(d, "x.fq")
        with open(fz, "wb") as f:
            for _ in range(copies):
                f.write(comp)
            f.write(bgzf_ref.EOF_BLOCK)
        with open(fp, "wb") as f:
            for _ in range(copies):
                f.write(text)
        n_text, n_comp = len(text) * copies, len(comp) * copies + len(bgzf_ref.EOF_BLOCK)
        zfd, pfd = os.open(fz, os.O_RDONLY), os.open(fp, os.O_RDONLY)

        def bgzf_load():
            p, n = C.c_void_p(), C.c_size_t()
            check(lib.bsk_bgzf_load(zfd, 0, 0, C.byref(p), C.byref(n)))
            assert n.value == n_text
            return p

        def plain_load():
            p = C.c_void_p()
            check(lib.bsk_shard_load(pfd, 0, n_text, 0, 0, C.byref(p)))
            return p

        d_comp = C.c_void_p()
        check(lib.bsk_shard_load(zfd, 0, n_comp, 0, 0, C.byref(d_comp)))

        def inflate():
            p, n = C.c_void_p(), C.c_size_t()
            check(lib.bsk_bgzf_inflate_device(d_comp, n_comp, 0, C.byref(p), C.byref(n)))
            return p

        # exact, once (this is also the warm-up of every leg)
        a, b = bgzf_load(), plain_load()
        ta, tb = torch.empty(n_text, dtype=torch.uint8, device="cuda"), torch.empty(n_text, dtype=torch.uint8, device="cuda")
        check(lib.bsk_device_copy(C.c_void_p(ta.data_ptr()), a, n_text, 3))
        check(lib.bsk_device_copy(C.c_void_p(tb.data_ptr()), b, n_text, 3))
        exact = bool(torch.equal(ta, tb))
        del ta, tb
        lib.bsk_device_free(a)
        lib.bsk_device_free(b)
        lib.bsk_device_free(inflate())
        times = {"bgzf_load": [], "plain_load": [], "inflate": []}
        for _ in range(reps):
            for name, fn in (("bgzf_load", bgzf_load), ("plain_load", plain_load), ("inflate", inflate)):
                ms, p = timed(fn)
                times[name].append(ms)
                lib.bsk_device_free(p)
        res = {"text_bytes": n_text, "compressed_bytes": n_comp, "compression": round(n_text / n_comp, 3), "blocks": (len(text) + BLOCK - 1) // BLOCK * copies + 1,
               "reps": reps, "exact": exact, "raw_ms": {k: [round(x, 3) for x in v] for k, v in times.items()},
               "bgzf_load": leg(times["bgzf_load"], n_text, n_comp), "plain_load": leg(times["plain_load"], n_text),
               "inflate": leg(times["inflate"], n_text, n_comp)}
        for k in ("bgzf_load", "inflate"):
            res[k]["ratio_to_plain"] = round(res[k]["text_GBps"] / res["plain_load"]["text_GBps"], 3)
        with bsk.Operator("Stats", "{}", 0) as op:   # (any context: the BGZF stages are the process's)
            check(lib.bsk_profile_reset(op.ctx))
            check(lib.bsk_profile_enable(op.ctx, 1))
            lib.bsk_device_free(inflate())
            pb = C.create_string_buffer(1 << 16)
            check(lib.bsk_profile_dump(op.ctx, pb, len(pb)), op.ctx)
            check(lib.bsk_profile_enable(op.ctx, 0))
            res["stages_ms"] = {k: round(float(v.split("/")[0]), 3) for k, v in (i.rsplit("=", 1) for i in pb.value.decode().split(";") if "=" in i)
                                if k.startswith("bgzf_")}
        lib.bsk_device_free(d_comp)
        os.close(zfd)
        os.close(pfd)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
