"""k_stats<FASTQ, default, DPP> searches the record starts at both ends of a range itself (no k_prep in front of it).  The
search wants many scalar registers, and spilled scalar registers live in lanes of vector registers: its first version cost
the default row four spilled VGPRs and 12 bytes of scratch per lane.  This reads the compiler's resource report (no GPU
needed): every FASTQ kernel on the DPP scan -- the ones that run unless a switch says otherwise -- keeps what it had before
the search moved in: no scratch, no spilled vector register, 6 waves per SIMD for the default row, 5 for the two of `-a`."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# k_stats<FASTQ, ALL, DPP, ROLES_T> -> waves per SIMD
WANT = {"7k_statsILb1ELb0ELb1ELb1E": 6,   # default row
        "7k_statsILb1ELb1ELb1ELb1E": 5,   # -a by line roles
        "7k_statsILb1ELb1ELb1ELb0E": 5}   # -a on the dense path (stats_a=dense)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_fastq_k_stats_keeps_registers_and_occupancy(tmp_path):
    src = os.path.join(ROOT, "bigseqkit_amd", "csrc", "stream_stats.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", str(tmp_path / "s.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = set()
    for b in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        name = b.split(" ", 1)[0].split()[0]
        key = next((k for k in WANT if k in name), None)
        if key is None:
            continue
        seen.add(key)
        num = lambda what: int(re.search(re.escape(what) + r": (\d+)", b).group(1))
        assert (num("ScratchSize [bytes/lane]"), num("VGPRs Spill")) == (0, 0), (name, b[:600])
        assert num("Occupancy [waves/SIMD]") >= WANT[key], (name, b[:600])
    assert seen == set(WANT)
