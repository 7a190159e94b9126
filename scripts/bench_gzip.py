#!/usr/bin/env python3
"""Plain gzip input next to BGZF and to the plain load, file -> text in HBM on 1 GPU.  The input is a synthetic FASTQ-150 text
(bsk_synth_host) of `MB` megabytes, compressed once as ONE gzip member at zlib level 6 and written `copies` times -- a gzip file of
`copies` members --, next to the same text as BGZF and plain.  Timed in the same run, one after the other in every repetition:
    gzip_load      bsk_gzip_load at the default chunk size, and at half and twice that size (with the plan counts of each)
    bgzf_load      bsk_bgzf_load of the same text as BGZF
    plain_load     bsk_shard_load of the plain file: the yardstick
    zlib_host      zlib.decompress of one member on one host thread, scaled to the file
One more, profiled gzip_load per chunk size gives the device times of the stages gzip_find / gzip_size / gzip_decode /
gzip_windows / gzip_translate / gzip_crc (bsk_profile_dump).  The inflated text is compared with the plain file's bytes once
(`exact`).  Nothing about the speed of this path has been tuned: a run is "measured once, untuned", and the stage that bounds
the call is the next thing to work on.  Prints one JSON object.  Not the driver's bench (that is bench.py).
  python scripts/bench_gzip.py [MB of text per member, default 256] [copies, default 8] [reps, default 3]"""
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


def as_bgzf(text):
    def one(i):
        piece = text[i:i + BLOCK]
        return bgzf_ref.member(bgzf_ref.deflate(piece, level=6), piece)
    with ThreadPoolExecutor(16) as pool:   # (zlib releases the interpreter lock)
        return b"".join(pool.map(one, range(0, len(text), BLOCK)))


def as_gzip(text):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(text) + c.flush()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def leg(ms, text_bytes):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"ms": round(med, 3), "spread": round((ms[-1] - ms[0]) / med, 3), "text_GBps": round(text_bytes / med / 1e6, 2)}


def main():
    text = synth_text(mb << 20)
    gz, bz = as_gzip(text), as_bgzf(text)
    t0 = time.perf_counter()
    assert zlib.decompress(gz, 31) == text
    zlib_ms = (time.perf_counter() - t0) * 1e3 * copies
    with tempfile.TemporaryDirectory() as d:
        paths = {k: os.path.join(d, "x." + k) for k in ("gz", "bgz", "fq")}
        for k, data, tail in (("gz", gz, b""), ("bgz", bz, bgzf_ref.EOF_BLOCK), ("fq", text, b"")):
            with open(paths[k], "wb") as f:
                for _ in range(copies):
                    f.write(data)
                f.write(tail)
        n_text, n_gz = len(text) * copies, len(gz) * copies
        fds = {k: os.open(p, os.O_RDONLY) for k, p in paths.items()}

        def gzip_load(chunk):
            def run():
                p, n = C.c_void_p(), C.c_size_t()
                check(lib.bsk_gzip_load(fds["gz"], 0, 0, chunk, C.byref(p), C.byref(n)))
                assert n.value == n_text
                return p
            return run

        def bgzf_load():
            p, n = C.c_void_p(), C.c_size_t()
            check(lib.bsk_bgzf_load(fds["bgz"], 0, 0, C.byref(p), C.byref(n)))
            assert n.value == n_text
            return p

        def plain_load():
            p = C.c_void_p()
            check(lib.bsk_shard_load(fds["fq"], 0, n_text, 0, 0, C.byref(p)))
            return p

        # exact, once (this is also the warm-up), and the default chunk size from the plan
        a, b = gzip_load(0)(), plain_load()
        default_chunk = bsk.GzipPlan()["chunk_bytes"]
        ta, tb = torch.empty(n_text, dtype=torch.uint8, device="cuda"), torch.empty(n_text, dtype=torch.uint8, device="cuda")
        check(lib.bsk_device_copy(C.c_void_p(ta.data_ptr()), a, n_text, 3))
        check(lib.bsk_device_copy(C.c_void_p(tb.data_ptr()), b, n_text, 3))
        exact = bool(torch.equal(ta, tb))
        del ta, tb
        lib.bsk_device_free(a)
        lib.bsk_device_free(b)
        lib.bsk_device_free(bgzf_load())
        legs = [("gzip_load_%d" % c, gzip_load(c)) for c in (default_chunk // 2, default_chunk, default_chunk * 2)]
        legs += [("bgzf_load", bgzf_load), ("plain_load", plain_load)]
        times = {name: [] for name, _ in legs}
        plans = {}
        for _ in range(reps):
            for name, fn in legs:
                ms, p = timed(fn)
                times[name].append(ms)
                lib.bsk_device_free(p)
                if name.startswith("gzip"):
                    plans[name] = bsk.GzipPlan()
        res = {"text_bytes": n_text, "gzip_bytes": n_gz, "compression": round(n_text / n_gz, 3), "members": copies, "reps": reps, "exact": exact,
               "default_chunk_bytes": default_chunk, "raw_ms": {k: [round(x, 3) for x in v] for k, v in times.items()},
               "zlib_host": {"ms": round(zlib_ms, 1), "text_GBps": round(n_text / zlib_ms / 1e6, 3)}}
        for name, _ in legs:
            res[name] = leg(times[name], n_text)
            res[name]["ratio_to_plain"] = round(min(times["plain_load"]) / min(times[name]), 3)
            if name in plans:
                res[name]["plan"] = plans[name]
        with bsk.Operator("Stats", "{}", 0) as op:   # (any context: the stages are the process's)
            for name, fn in legs[:3]:
                check(lib.bsk_profile_reset(op.ctx))
                check(lib.bsk_profile_enable(op.ctx, 1))
                lib.bsk_device_free(fn())
                pb = C.create_string_buffer(1 << 16)
                check(lib.bsk_profile_dump(op.ctx, pb, len(pb)), op.ctx)
                check(lib.bsk_profile_enable(op.ctx, 0))
                res[name]["stages_ms"] = {k: round(float(v.split("/")[0]), 3) for k, v in (i.rsplit("=", 1) for i in pb.value.decode().split(";") if "=" in i)
                                          if k.startswith("gzip_")}
        for fd in fds.values():
            os.close(fd)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
