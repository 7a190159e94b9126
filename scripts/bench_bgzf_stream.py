#!/usr/bin/env python3
"""`stats -a` on a FASTQ file written as BGZF, streamed through the piece reader (bsk_bgzf_reader_*), next to the two paths
it stands between, on 1 GPU.  The text is the synthetic FASTQ-150 of bsk_synth_host, `MB` megabytes of it (default 2048),
written once as a plain file and once as BGZF (compressed on the device).  Three runs of the command line, wall time each:
    streamed_bgzf    BSK_HOST_PIPELINE_FROM=0 BSK_BGZF_STREAM=1: the BGZF file through the reader, piece by piece, never held whole
    resident_bgzf    the BGZF file through bsk_bgzf_load: the file and its text whole on the device
    streamed_plain   BSK_HOST_PIPELINE_FROM=0: the plain file streamed from its mapping
and the reader alone, in this process, with its default sizes: wall time, the stages of bsk_profile_dump, and the share of the
wall time that was NOT under the stage bgzf_inflate -- what the reads, the copies, the walk of the chain, the cut and the moves
of the carried head cost where they are not hidden under a chunk's inflate.  The three tables are compared.  Nothing about the
speed of this path has been tuned.  Prints one JSON object.  Not the driver's bench (that is bench.py).
  python scripts/bench_bgzf_stream.py [MB of text, default 2048] [piece MiB for the reader alone, default 1024]"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bigseqkit_amd as bsk
from bigseqkit_amd._lib import lib, check

CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")
argv = sys.argv[1:]
mb = int(argv[0]) if len(argv) > 0 else 2048
piece_mib = int(argv[1]) if len(argv) > 1 else 1024
SLAB = 256 << 20


def run(args, env):
    t0 = time.perf_counter()
    p = subprocess.run([CLI, *args], capture_output=True, env=dict(os.environ, **env))
    ms = (time.perf_counter() - t0) * 1e3
    if p.returncode != 0:
        raise SystemExit(p.stderr.decode()[-2000:])
    return ms, p.stdout


def main():
    rb = lib.bsk_synth_record_bytes(0)
    n = (mb << 20) // rb * rb
    with tempfile.TemporaryDirectory() as d:
        plain, packed = os.path.join(d, "reads.fq"), os.path.join(d, "reads.fq.gz")
        comp_bytes = 0
        with open(plain, "wb") as fp, open(packed, "wb") as fz:   # (slabs of whole records: neither file is held whole here)
            per = SLAB // rb * rb
            for off in range(0, n, per):
                k = min(per, n - off)
                host = C.create_string_buffer(k)
                check(lib.bsk_synth_host(0, 42, 0, off // rb, host, k))
                fp.write(host.raw)
                z = bsk.BgzfDeflate(host.raw, device=0, eof=off + k == n)
                fz.write(z)
                comp_bytes += len(z)
        res = {"text_bytes": n, "compressed_bytes": comp_bytes, "ratio": round(comp_bytes / n, 4)}
        stream = {"BSK_HOST_PIPELINE_FROM": "0", "BSK_BGZF_STREAM": "1"}
        tables = {}
        for name, path, env in (("streamed_bgzf", packed, stream), ("resident_bgzf", packed, {}), ("streamed_plain", plain, stream)):
            ms, out = run(["stats", "-a", "-T", path], env)
            tables[name] = out.replace(path.encode(), b"F")
            res[name] = {"wall_ms": round(ms, 1), "text_GBps": round(n / ms / 1e6, 2)}
        res["tables_equal"] = tables["streamed_bgzf"] == tables["resident_bgzf"] == tables["streamed_plain"] and bool(tables["streamed_bgzf"])
        # the reader alone
        with bsk.Operator("Stats", "{}", 0) as op:
            check(lib.bsk_profile_reset(op.ctx))
            check(lib.bsk_profile_enable(op.ctx, 1))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pieces = total = 0
            with bsk.BgzfReader(packed, bsk.FORMAT_FASTQ, device=0, piece_text_bytes=piece_mib << 20) as r:
                for t, lo, hi in r:
                    pieces += 1
                    total += t.numel()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            pb = C.create_string_buffer(1 << 16)
            check(lib.bsk_profile_dump(op.ctx, pb, len(pb)), op.ctx)
            check(lib.bsk_profile_enable(op.ctx, 0))
        stages = {k: v for k, v in (i.rsplit("=", 1) for i in pb.value.decode().split(";") if "=" in i) if k.startswith("bgzf_")}
        inflate_ms = float(stages.get("bgzf_inflate", "0/0").split("/")[0])
        res["reader_alone"] = {"wall_ms": round(wall, 1), "text_GBps": round(total / wall / 1e6, 2), "pieces": pieces, "text_bytes": total,
                               "piece_MiB": piece_mib, "stages_ms_over_launches": stages,
                               "share_of_wall_not_under_bgzf_inflate": round(1 - inflate_ms / wall, 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
