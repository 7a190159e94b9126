"""`fa2fq` without a GPU: the Python restatement against the hand-written fixtures, Before() of the reference
(bigseqkit-lib/fa2fq.go:29-57: messages and their order, the log line), the option builder and the command line's flags."""
import ctypes as C
import json
import os
import random
import re
import subprocess

import pytest

import bigseqkit_amd as bsk
from bigseqkit_amd._lib import lib
import fa2fq_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "fa2fq_fixtures.json")))
CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")


def create(opts):
    ctx = C.c_void_p()
    rc = lib.bsk_create(b"Fa2Fq", json.dumps(opts).encode(), -1, C.byref(ctx))
    if rc == 0:
        log = lib.bsk_log_text(ctx).decode()
        lib.bsk_destroy(ctx)
        return 0, log
    return rc, lib.bsk_global_error().decode()


@pytest.mark.parametrize("case", FIX, ids=[c["name"] for c in FIX])
def test_reference_model_on_fixtures(case):
    assert F.fa2fq(case["fastq"].encode(), case["fasta"].encode(), case["opts"]) == case["want"].encode()


def test_fixtures_cover_every_verdict():
    kinds = set()
    for c in FIX:
        kinds |= {v[0] for v in F.verdicts(c["fastq"].encode(), c["fasta"].encode(), c["opts"])}
    assert kinds == {"plus", "minus", "absent", "nohit"}


def test_before_messages_in_order(tmp_path):
    good = tmp_path / "t.fa"
    good.write_text(">r1\nACGT\n>r2 d\nAC\nGT\n>r1\nTTTT\n")
    empty = tmp_path / "empty.fa"
    empty.write_text("no header here\n\n")
    missing = str(tmp_path / "none.fa")
    # the alphabet error comes first (fa2fq.go:31-34), then the flag, then the file, then its content
    rc, msg = create({"Config": {"SeqType": "xyz"}})
    assert rc == 2 and msg == "invalid sequence type: xyz, available value: dna|rna|protein|unlimit|auto"
    rc, msg = create({"Config": {"SeqType": "xyz"}, "FastaFile": missing})
    assert rc == 2 and msg.startswith("invalid sequence type: xyz")
    assert create({}) == (2, "flag -f (--fasta-file) needed")
    assert create({"OnlyPositiveStrand": True}) == (2, "flag -f (--fasta-file) needed")
    assert create({"FastaFile": missing}) == (2, "open " + missing + ": no such file or directory")
    assert create({"FastaFile": str(empty)}) == (2, "no sequences found in fasta file: " + str(empty))
    # three headers, two distinct names: len(map)
    assert create({"FastaFile": str(good)}) == (0, "[INFO] 2 sequences loaded\n")
    assert create({"FastaFile": str(good), "OnlyPositiveStrand": True, "Config": {"SeqType": "dna"}}) == (0, "[INFO] 2 sequences loaded\n")
    assert create({"FastaFile": str(good), "Config": {"Quiet": True}}) == (0, "")


def test_large_table_loads(tmp_path):
    """(the table is a map: loading is linear in the file)"""
    f = tmp_path / "many.fa"
    f.write_text("".join(">read%d\nACGT\n" % (i % 150000) for i in range(200000)))
    assert create({"FastaFile": str(f)}) == (0, "[INFO] 150000 sequences loaded\n")


def test_generator_exercises_every_branch():
    """the GPU test's random cases: each of plus / minus / absent / nohit covers at least a tenth of the records"""
    import test_fa2fq_gpu as G
    count, total = {}, 0
    rng = random.Random(G.SEED)
    for _ in range(G.N_RANDOM):
        fq, fa, opts = G.random_case(rng)
        for v in F.verdicts(fq, fa, opts):
            count[v[0]] = count.get(v[0], 0) + 1
            total += 1
    assert total > 3000
    for kind in ("plus", "minus", "absent", "nohit"):
        assert count.get(kind, 0) * 10 >= total, (kind, count, total)


def test_python_options_and_api():
    o = bsk.SeqKitFa2FqOptions().FastaFile("t.fa").OnlyPositiveStrand(True).Config(bsk.SeqKitConfig().SeqType("dna"))
    j = json.loads(o.to_json())
    assert (j["FastaFile"], j["OnlyPositiveStrand"], j["Config"]["SeqType"]) == ("t.fa", True, "dna")
    j = json.loads(bsk.SeqKitFa2FqOptions().to_json())
    assert j["FastaFile"] is None and j["OnlyPositiveStrand"] is None   # unset: the library's setDefaults() fills them
    assert callable(bsk.Fa2Fq)


def test_match_kernels_use_no_scratch():
    """the lane and the wave search keep their state in registers (build() needs hipcc: so does this)"""
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c",
                          "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage",
                          os.path.join(ROOT, "bigseqkit_amd", "csrc", "ops_fa2fq.hip")], capture_output=True, text=True)
    found = re.findall(r"Function Name: (\S*k_fa2fq\S*).*?ScratchSize \[bytes/lane\]: (\d+)", out.stderr, re.S)
    assert len(found) >= 4 and all(int(s) == 0 for _, s in found), out.stderr[-2000:]


def test_cli_flag_table_and_help():
    """bigseqkit-cli/fa2fq.go:21-49: both flags reach their Fa2FqOptions field; the help text is the reference's"""
    p = subprocess.run([CLI, "fa2fq", "-f", "t.fa", "-P", "x.fq", "--dry-run"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    op, js = p.stdout.splitlines()[:2]
    assert op == "Fa2Fq"
    o = json.loads(js)
    assert (o["FastaFile"], o["OnlyPositiveStrand"]) == ("t.fa", True)
    p = subprocess.run([CLI, "fa2fq", "--fasta-file=u.fa", "x.fq", "--dry-run"], capture_output=True, text=True)
    o = json.loads(p.stdout.splitlines()[1])
    assert (o["FastaFile"], o["OnlyPositiveStrand"]) == ("u.fa", False)
    p = subprocess.run([CLI, "fa2fq", "--help"], capture_output=True, text=True)
    assert p.returncode == 0
    assert p.stdout.startswith("retrieve corresponding FASTQ records by a FASTA file\nAttention:\n"
                               "  1. We assume the FASTA file comes from the FASTQ file,\n"
                               "     so they share sequence IDs, and sequences in FASTA\n"
                               "     should be subseq of sequences in FASTQ file.\n")
    assert "  -f, --fasta-file string      FASTA file)\n" in p.stdout
    assert "  -P, --only-positive-strand   only search on positive strand\n" in p.stdout
    assert "fa2fq" in subprocess.run([CLI, "--help"], capture_output=True, text=True).stdout
