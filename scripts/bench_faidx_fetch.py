#!/usr/bin/env python3
"""`faidx FILE regions` through the index (`-d IDX`, PARITY FAIX) next to the whole-file run it replaces, on 1 GPU.  The input
is a wrapped FASTA (60 bases a line) of `MB` megabytes (default 2048) in 8 chromosome-sized records of random ACGT, plain.
Cases: 1, 100 and 10 000 regions of 1 kb (given with -l) and one whole record.  Per case the wall time of the command line
    whole   faidx FILE -l regions            (the file is loaded, indexed, one lane per record)
    fetch   faidx FILE -l regions -d IDX     (IDX present: the spans of the regions are read)
-- the whole-file run once, the fetch three times (min and median) -- and whether the bytes are equal.  For the whole-record
case also the fetch kernel's device time (stage k_faidx_fetch of bsk_profile_read) and its bytes written per second, beside the
stages of `seq` printing the same record from a device-resident copy (bsk_profile_dump).  No threshold: nobody has measured
any of this before.  Prints one JSON object.  Not the driver's bench (that is bench.py).
  python scripts/bench_faidx_fetch.py [MB of text, default 2048]"""
import ctypes as C
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bigseqkit_amd as bsk  # noqa: E402
from bigseqkit_amd import _lib  # noqa: E402
from bigseqkit_amd._lib import lib, check  # noqa: E402

CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")
mb = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
NREC, LB = 8, 60


class Opts:
    def __init__(self, d):
        self.d = d

    def to_json(self):
        return json.dumps(self.d)


def run(args):
    t0 = time.perf_counter()
    p = subprocess.run([CLI, "faidx", *args], capture_output=True)
    ms = (time.perf_counter() - t0) * 1e3
    if p.returncode != 0:
        raise SystemExit(p.stderr.decode()[-2000:])
    return ms, p.stdout


def main():
    rng = random.Random(1)
    block_lines = 1 << 18  # 16 MiB of lines, repeated: the content does not matter to either path
    block = b"".join(bytes(rng.choice(b"ACGT") for _ in range(LB)) + b"\n" for _ in range(4096)) * (block_lines // 4096)
    per = max(1, (mb << 20) // NREC // len(block))
    length = per * block_lines * LB
    with tempfile.TemporaryDirectory() as d:
        path, idx = os.path.join(d, "genome.fa"), os.path.join(d, "genome.fa.fai")
        rows, off = [], 0
        with open(path, "wb") as f:
            for k in range(NREC):
                head = b">chr%d\n" % (k + 1)
                f.write(head)
                off += len(head)
                rows.append(b"chr%d\t%d\t%d\t%d\t%d\n" % (k + 1, length, off, LB, LB + 1))
                for _ in range(per):
                    f.write(block)
                off += per * len(block)
        with open(idx, "wb") as f:
            f.write(b"".join(rows))
        res = {"file_bytes": off, "records": NREC, "record_bases": length}
        for name, regions in (("1_region", 1), ("100_regions", 100), ("10000_regions", 10000), ("whole_record", 0)):
            rf = os.path.join(d, name + ".txt")
            if regions:
                # (one query per ID is the reference's rule: the regions go to distinct names only up to NREC, so the hits
                # are spread by giving every region file the same 8 names with different starts -- and the first wins.  More
                # than 8 hits therefore need more names: the records are addressed through copies of the rows)
                qs = []
                for j in range(regions):
                    b = rng.randrange(1, length - 1000)
                    qs.append("chr%d_%d:%d-%d" % (j % NREC + 1, j, b, b + 999))
                with open(idx + "." + name, "wb") as f:
                    f.write(b"".join(rows[j % NREC].replace(b"chr%d\t" % (j % NREC + 1), b"chr%d_%d\t" % (j % NREC + 1, j), 1) for j in range(regions)))
                use_idx = idx + "." + name
            else:
                qs, use_idx = ["chr3"], idx
            with open(rf, "w") as f:
                f.write("\n".join(qs) + "\n")
            fetch = [run([path, "-l", rf, "-d", use_idx, "-o", "-"]) for _ in range(3)]
            case = {"fetch_wall_ms_min": round(min(m for m, _ in fetch), 1), "fetch_wall_ms_median": round(statistics.median(m for m, _ in fetch), 1),
                    "output_bytes": len(fetch[0][1])}
            if not regions or regions <= NREC:
                # the whole-file run can answer only names the file has: the cases of up to 8 regions and the whole record
                with open(rf, "w") as f:
                    f.write("\n".join(q.split("_")[0] + (":" + q.split(":")[1] if ":" in q else "") for q in qs) + "\n")
                ms, out = run([path, "-l", rf, "-o", "-"])
                again = run([path, "-l", rf, "-d", idx, "-o", "-"])
                case.update(whole_wall_ms=round(ms, 1), equal=out == again[1], fetch_same_names_wall_ms=round(again[0], 1))
            res[name] = case
        # the kernel alone on one whole record, and `seq` printing the same record from the device
        o = Opts({"Regions": ["chr3"]})
        fd = os.open(path, os.O_RDONLY)
        with bsk.FaidxFetchPlan(b"".join(rows), o, off, device=0) as plan:
            check(lib.bsk_profile_enable(plan.op.ctx, 1), plan.op.ctx)
            times = []
            for _ in range(4):
                check(lib.bsk_profile_reset(plan.op.ctx), plan.op.ctx)
                out = _lib.Out()
                t0 = time.perf_counter()
                check(lib.bsk_faidx_fetch_run(plan.op.ctx, fd, None, 0, plan.ptr, 0, 0, None, C.byref(out)), plan.op.ctx)
                call_ms = (time.perf_counter() - t0) * 1e3
                ms, n = C.c_double(), C.c_uint64()
                check(lib.bsk_profile_read(plan.op.ctx, b"k_faidx_fetch", C.byref(ms), C.byref(n)), plan.op.ctx)
                times.append((ms.value, call_ms))
            k_ms = min(t for t, _ in times[1:])
            res["kernel_whole_record"] = {"k_faidx_fetch_ms": round(k_ms, 3), "out_bytes": out.len, "out_GBps": round(out.len / k_ms / 1e6, 1),
                                          "call_ms_min": round(min(c for _, c in times[1:]), 1), "info": plan.info()}
        os.close(fd)
        with open(path, "rb") as f:
            f.seek(int(rows[2].split(b"\t")[2]) - len(b">chr3\n"))
            rec = f.read(len(b">chr3\n") + per * len(block))
        t = torch.frombuffer(bytearray(rec), dtype=torch.uint8).cuda()
        with bsk.Operator("SeqTransform", "{}", 0) as op:
            check(lib.bsk_profile_enable(op.ctx, 1), op.ctx)
            best = None
            for _ in range(4):
                check(lib.bsk_profile_reset(op.ctx), op.ctx)
                out = _lib.Out()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                check(lib.bsk_seq_run(op.ctx, C.c_void_p(t.data_ptr()), t.numel(), 1, bsk.FORMAT_FASTA, 0, None, C.byref(out)), op.ctx)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
                buf = C.create_string_buffer(1 << 16)
                check(lib.bsk_profile_dump(op.ctx, buf, len(buf)), op.ctx)
                if best is None or ms < best[0]:
                    best = (ms, buf.value.decode(), out.len)
            res["seq_same_record"] = {"call_ms_min": round(best[0], 2), "out_bytes": best[2], "out_GBps_of_call": round(best[2] / best[0] / 1e6, 1),
                                      "stages": best[1]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
