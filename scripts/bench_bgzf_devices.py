#!/usr/bin/env python3
"""`stats -a` on a FASTQ file written as BGZF under --devices (BSK_BGZF_DEVICES=1: block-aligned cuts, a shard per worker), next
to the resident single-device run it is built from, on 1 GPU.  The text is the synthetic FASTQ-150 of bsk_synth_host, `MB`
megabytes of it (default 2048), written as BGZF (compressed on the device), as scripts/bench_bgzf_stream.py writes it.  Three
runs of the command line, wall time each:
    resident      --device 0: the file through bsk_bgzf_load, whole on the device
    devices_0     --devices 0: one worker -- the cut points, then the one shard through bsk_bgzf_shard_load
    devices_0_0   --devices 0,0: two workers that SHARE the one GPU.  For information only: it says nothing about scaling
and, from BSK_CLI_TIMING of the --devices runs, the time between the marks "device count + cut points" and "bgzf cut points"
-- what the host rule costs -- and the marks of the workers.  The only expectation: devices_0 should cost no more than resident
plus the cut-point time it reports (and what --devices costs a plain file: the communicator).  The three tables are compared.
Nothing about the speed of this path has been tuned; scaling over real GPUs is not measured here.  Prints one JSON object.
Not the driver's bench (that is bench.py).
  python scripts/bench_bgzf_devices.py [MB of text, default 2048]"""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402
import bigseqkit_amd as bsk  # noqa: E402
from bigseqkit_amd._lib import lib, check  # noqa: E402

CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")
mb = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
SLAB = 256 << 20


def run(args, env):
    t0 = time.perf_counter()
    p = subprocess.run([CLI, *args], capture_output=True, env=dict(os.environ, **env))
    ms = (time.perf_counter() - t0) * 1e3
    if p.returncode != 0:
        raise SystemExit(p.stderr.decode()[-2000:])
    return ms, p.stdout, p.stderr.decode()


def marks(stderr):
    """[(seconds, text)] of BSK_CLI_TIMING"""
    return [(float(m.group(1)), m.group(2)) for m in re.finditer(r"\[timing\]\s+([0-9.]+) s  (.*)", stderr)]


def main():
    rb = lib.bsk_synth_record_bytes(0)
    n = (mb << 20) // rb * rb
    with tempfile.TemporaryDirectory() as d:
        packed = os.path.join(d, "reads.fq.gz")
        comp_bytes = 0
        with open(packed, "wb") as fz:   # (slabs of whole records: the file is not held whole here)
            per = SLAB // rb * rb
            for off in range(0, n, per):
                k = min(per, n - off)
                host = C.create_string_buffer(k)
                check(lib.bsk_synth_host(0, 42, 0, off // rb, host, k))
                z = bsk.BgzfDeflate(host.raw, device=0, eof=off + k == n)
                fz.write(z)
                comp_bytes += len(z)
        res = {"text_bytes": n, "compressed_bytes": comp_bytes, "ratio": round(comp_bytes / n, 4)}
        on = {"BSK_BGZF_DEVICES": "1", "BSK_CLI_TIMING": "1"}
        tables = {}
        for name, args, env in (("resident", ["--device", "0"], {}), ("devices_0", ["--devices", "0"], on), ("devices_0_0", ["--devices", "0,0"], on)):
            ms, out, err = run(["stats", "-a", "-T", packed, *args], env)
            tables[name] = out
            res[name] = {"wall_ms": round(ms, 1), "text_GBps": round(n / ms / 1e6, 2)}
            m = marks(err)
            if m:
                at = {text: s for s, text in m}
                res[name]["cut_points_ms"] = round((at["bgzf cut points"] - at["device count + cut points"]) * 1e3, 1)
                res[name]["marks_s"] = [[s, text] for s, text in m]
        res["tables_equal"] = tables["resident"] == tables["devices_0"] == tables["devices_0_0"] and bool(tables["resident"])
        res["devices_0_minus_resident_minus_cut_points_ms"] = round(res["devices_0"]["wall_ms"] - res["resident"]["wall_ms"] - res["devices_0"]["cut_points_ms"], 1)
        t0 = time.perf_counter()
        v = bsk.BgzfCutPoints(packed, bsk.FORMAT_FASTQ, 8)
        res["cut_points_world_8_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["cut_points_world_8"] = v
    print(json.dumps(res))


if __name__ == "__main__":
    main()
