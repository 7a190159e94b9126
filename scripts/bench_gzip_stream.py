#!/usr/bin/env python3
"""`stats -a` on a FASTQ file written as plain gzip, read through the segment reader (bsk_gzip_reader_*), next to the two paths
it stands between, on 1 GPU.  The input is that of scripts/bench_gzip.py: a synthetic FASTQ-150 text (bsk_synth_host) of `MB`
megabytes, compressed once as ONE gzip member at zlib level 6 and written `copies` times, next to the same text as BGZF.  Three
runs of the command line, one after the other in the same run, wall time each:
    streamed_gzip    BSK_GZIP=1 BSK_GZIP_STREAM=1 BSK_HOST_PIPELINE_FROM=0: the gzip file through the reader, segment by segment
    resident_gzip    BSK_GZIP=1: the gzip file through bsk_gzip_load -- the file, its text and its symbols whole on the device
    streamed_bgzf    BSK_BGZF_STREAM=1 BSK_HOST_PIPELINE_FROM=0: the BGZF file through its piece reader
and the reader alone, in this process, with its default sizes: wall time, the stages of bsk_profile_dump, the share of the wall
time that was NOT under the gzip_* stages -- the reads, the copies, the walk of the chain on the host, the staging copy and the
moves of the carried head where a segment's kernels do not hide them -- and what bsk_gzip_reader_info says.  The three tables
are compared.  The expectation to hold streamed_gzip against is resident_gzip of the same run: k_gz_decode bounds both.  Nothing
about the speed of this path has been tuned.  Prints one JSON object.  Not the driver's bench (that is bench.py).
  python scripts/bench_gzip_stream.py [MB of text per member, default 256] [copies, default 8]"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bigseqkit_amd as bsk
from bigseqkit_amd._lib import lib, check

CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")
argv = sys.argv[1:]
mb = int(argv[0]) if len(argv) > 0 else 256
copies = int(argv[1]) if len(argv) > 1 else 8


def run(args, env):
    e = {k: v for k, v in os.environ.items() if not k.startswith(("BSK_GZIP", "BSK_BGZF_STREAM", "BSK_HOST_PIPELINE"))}
    t0 = time.perf_counter()
    p = subprocess.run([CLI, *args], capture_output=True, env=dict(e, **env))
    ms = (time.perf_counter() - t0) * 1e3
    if p.returncode != 0:
        raise SystemExit(p.stderr.decode()[-2000:])
    return ms, p.stdout


def main():
    rb = lib.bsk_synth_record_bytes(0)
    n1 = (mb << 20) // rb * rb
    host = C.create_string_buffer(n1)
    check(lib.bsk_synth_host(0, 42, 0, 0, host, n1))
    text = host.raw[:n1]
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    gz = c.compress(text) + c.flush()
    bz = bsk.BgzfDeflate(text, device=0, eof=False)
    eof = bsk.BgzfDeflate(b"", device=0, eof=True)
    n = n1 * copies
    with tempfile.TemporaryDirectory() as d:
        paths = {k: os.path.join(d, "reads." + k) for k in ("fq.gz", "bgzf.fq.gz")}
        for k, data, tail in (("fq.gz", gz, b""), ("bgzf.fq.gz", bz, eof)):
            with open(paths[k], "wb") as f:
                for _ in range(copies):
                    f.write(data)
                f.write(tail)
        res = {"text_bytes": n, "gzip_bytes": len(gz) * copies, "bgzf_bytes": len(bz) * copies + len(eof), "members": copies}
        tables = {}
        for name, key, env in (("streamed_gzip", "fq.gz", {"BSK_GZIP": "1", "BSK_GZIP_STREAM": "1", "BSK_HOST_PIPELINE_FROM": "0"}),
                               ("resident_gzip", "fq.gz", {"BSK_GZIP": "1"}),
                               ("streamed_bgzf", "bgzf.fq.gz", {"BSK_BGZF_STREAM": "1", "BSK_HOST_PIPELINE_FROM": "0"})):
            ms, out = run(["stats", "-a", "-T", paths[key]], env)
            tables[name] = out.replace(paths[key].encode(), b"F")
            res[name] = {"wall_ms": round(ms, 1), "text_GBps": round(n / ms / 1e6, 2)}
        res["tables_equal"] = tables["streamed_gzip"] == tables["resident_gzip"] == tables["streamed_bgzf"] and bool(tables["streamed_gzip"])
        res["streamed_over_resident"] = round(res["streamed_gzip"]["wall_ms"] / res["resident_gzip"]["wall_ms"], 3)
        # the reader alone
        with bsk.Operator("Stats", "{}", 0) as op:
            check(lib.bsk_profile_reset(op.ctx))
            check(lib.bsk_profile_enable(op.ctx, 1))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pieces = total = 0
            with bsk.GzipReader(paths["fq.gz"], bsk.FORMAT_FASTQ, device=0) as r:
                for t, lo, hi in r:
                    pieces += 1
                    total += t.numel()
                info = r.info()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            pb = C.create_string_buffer(1 << 16)
            check(lib.bsk_profile_dump(op.ctx, pb, len(pb)), op.ctx)
            check(lib.bsk_profile_enable(op.ctx, 0))
        stages = {k: v for k, v in (i.rsplit("=", 1) for i in pb.value.decode().split(";") if "=" in i) if k.startswith("gzip_")}
        under = sum(float(v.split("/")[0]) for v in stages.values())
        res["reader_alone"] = {"wall_ms": round(wall, 1), "text_GBps": round(total / wall / 1e6, 2), "pieces": pieces, "text_bytes": total,
                               "stages_ms_over_launches": stages, "share_of_wall_not_under_gzip_stages": round(1 - under / wall, 3), "info": info,
                               "synchronisations_per_segment": 4}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
