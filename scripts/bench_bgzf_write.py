#!/usr/bin/env python3
"""BGZF output next to the plain copy, text in HBM -> bytes on the host, on 1 GPU: the mirror of scripts/bench_bgzf.py.  The text
is the synthetic FASTQ-150 of bsk_synth_host, `MB` megabytes of it (default 2048), put on the device once.  Timed, one after the
other in every repetition so that the legs see the same machine:
    deflate        bsk_bgzf_deflate_device alone: text in HBM -> the BGZF image in HBM
    to_host_bgzf   bsk_out_to_host_bgzf: the text leaves compressed, 64 MiB of text a piece, into pageable host memory
    to_host_plain  bsk_out_to_host of the same text: the yardstick
    zlib_level_1   Python's zlib at level 1 on ONE host thread over the same blocks (the first `REF_MB` megabytes, default 256;
                   the sizes of level 1 and level 6 are taken on those blocks and compared with ours on the same blocks)
Per leg: median ms over the repetitions, the spread (max - min) / median, text GB/s in.  One more, profiled call gives the
device times of the stages bgzf_deflate / bgzf_pack (bsk_profile_dump).  The compressed bytes are checked once: gzip.decompress
of the first 16 MB of text's blocks is that text, and the host encoder writes the same bytes (`exact`).  Nothing about the
speed of this path has been tuned.  Prints one JSON object.  Not the driver's bench (that is bench.py).
  python scripts/bench_bgzf_write.py [MB of text, default 2048] [reps, default 3] [REF_MB, default 256]"""
import ctypes as C
import gzip
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bigseqkit_amd as bsk
from bigseqkit_amd import _lib
from bigseqkit_amd._lib import lib, check

argv = sys.argv[1:]
mb = int(argv[0]) if len(argv) > 0 else 2048
reps = int(argv[1]) if len(argv) > 1 else 3
ref_mb = int(argv[2]) if len(argv) > 2 else 256
BLOCK = 65280


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


def zlib_blocks(text, level):
    total = 0
    for off in range(0, len(text), BLOCK):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        total += len(c.compress(text[off:off + BLOCK]) + c.flush()) + 26
    return total


def main():
    rb = lib.bsk_synth_record_bytes(0)
    n = (mb << 20) // rb * rb
    host = C.create_string_buffer(n)
    check(lib.bsk_synth_host(0, 42, 0, 0, host, n))
    t = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    check(lib.bsk_device_copy(C.c_void_p(t.data_ptr()), host, n, 1))
    torch.cuda.synchronize()
    n_ref = min(n, (ref_mb << 20) // BLOCK * BLOCK)
    ref_text = host.raw[:n_ref]
    del host
    cap = lib.bsk_bgzf_deflate_bound(n, 0)
    sink = C.create_string_buffer(cap)
    plain_sink = C.create_string_buffer(n)
    sizes = {}
    with bsk.Operator("Stats", "{}", 0) as op:   # (any context: its device is where the text is compressed)
        out = _lib.Out()
        out.d_data, out.len, out.n_segments = t.data_ptr(), n, 0

        def deflate():
            p, k = C.c_void_p(), C.c_size_t()
            check(lib.bsk_bgzf_deflate_device(C.c_void_p(t.data_ptr()), n, 0, 0, 1, C.byref(p), C.byref(k)))
            sizes["deflate"] = k.value
            return p

        def to_host_bgzf():
            k = C.c_size_t()
            check(lib.bsk_out_to_host_bgzf(op.ctx, C.byref(out), 1, sink, cap, C.byref(k)), op.ctx)
            sizes["to_host_bgzf"] = k.value

        def to_host_plain():
            check(lib.bsk_out_to_host(op.ctx, C.byref(out), plain_sink, n), op.ctx)

        # exact, once (this is also the warm-up of every leg)
        lib.bsk_device_free(deflate())
        to_host_bgzf()
        to_host_plain()
        head = min(n, (16 << 20) // BLOCK * BLOCK)
        ours_head = bsk.BgzfDeflate(t[:head], eof=True)
        exact = gzip.decompress(ours_head) == ref_text[:head] and ours_head == bsk.BgzfDeflateHost(ref_text[:head]) and sink.raw[:len(ours_head) - 28] == ours_head[:-28]
        times = {"deflate": [], "to_host_bgzf": [], "to_host_plain": []}
        for _ in range(reps):
            ms, p = timed(deflate)
            times["deflate"].append(ms)
            lib.bsk_device_free(p)
            for name, fn in (("to_host_bgzf", to_host_bgzf), ("to_host_plain", to_host_plain)):
                ms, _ = timed(fn)
                times[name].append(ms)
        t0 = time.perf_counter()
        l1 = zlib_blocks(ref_text, 1)
        zms = (time.perf_counter() - t0) * 1e3
        l6 = zlib_blocks(ref_text, 6)
        ours_ref = len(bsk.BgzfDeflate(t[:n_ref], eof=False))
        res = {"text_bytes": n, "compressed_bytes": sizes["deflate"], "ratio": round(sizes["deflate"] / n, 4), "blocks": (n + BLOCK - 1) // BLOCK, "reps": reps,
               "exact": bool(exact), "raw_ms": {k: [round(x, 3) for x in v] for k, v in times.items()},
               "deflate": leg(times["deflate"], n), "to_host_bgzf": leg(times["to_host_bgzf"], n), "to_host_plain": leg(times["to_host_plain"], n),
               "zlib_level_1": {"ms": round(zms, 3), "text_GBps": round(n_ref / zms / 1e6, 3), "threads": 1, "text_bytes": n_ref},
               "size_on_ref_blocks": {"text": n_ref, "ours": ours_ref, "level_1": l1, "level_6": l6, "ours_over_level_1": round(ours_ref / l1, 4),
                                      "ours_over_level_6": round(ours_ref / l6, 4)}}
        res["to_host_bgzf"]["ratio_to_plain"] = round(res["to_host_bgzf"]["text_GBps"] / res["to_host_plain"]["text_GBps"], 3)
        check(lib.bsk_profile_reset(op.ctx))
        check(lib.bsk_profile_enable(op.ctx, 1))
        lib.bsk_device_free(deflate())
        pb = C.create_string_buffer(1 << 16)
        check(lib.bsk_profile_dump(op.ctx, pb, len(pb)), op.ctx)
        check(lib.bsk_profile_enable(op.ctx, 0))
        res["stages_ms"] = {k: round(float(v.split("/")[0]), 3) for k, v in (i.rsplit("=", 1) for i in pb.value.decode().split(";") if "=" in i)
                            if k.startswith("bgzf_")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
