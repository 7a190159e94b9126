"""`head-genome` without a GPU (PARITY.md HEADG): the Python restatement against the hand-derived fixtures, the option error
at create time, the flag table of the command line, the refusals that are decided before a device is touched, and the
resource report of the new kernels (no scratch)."""
import json
import os
import re
import subprocess

import pytest

import bigseqkit_amd as bsk
from bigseqkit_amd._lib import BskError
import head_genome_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "head_genome_fixtures.json")))
CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
M_ERR = "value of flag --mini-common-words should be greater than 0"


@pytest.mark.parametrize("case", FIX["cases"], ids=[c["name"] for c in FIX["cases"]])
def test_restatement_against_the_hand_fixtures(case):
    m = case["m"]
    if "descs" in case:  # the rule itself, on descriptions no header text can produce
        assert R.verdicts([d.encode() for d in case["descs"]], m) == (case["cut"], case["error_at"])
        return
    data = case["input"].encode()
    if "create_error" in case:
        with pytest.raises(R.HeadGenomeError, match=re.escape(case["create_error"])):
            R.head_genome(data, False, m)
    elif "error" in case:
        with pytest.raises(R.HeadGenomeError) as e:
            R.head_genome(data, False, m)
        assert str(e.value) == case["error"]
    else:
        assert R.head_genome(data, False, m, FIX["line_width"]) == case["want"].encode()
        if data:
            assert R.cut_byte(data, False, m)[1] == case["kept"]


def test_words_and_shared_count():
    assert R.words(b"a\tb  c \t") == [b"a", b"b", b"c"] and R.words(b" \t ") == [] and R.words(b"y\r") == [b"y\r"]
    assert R.shared([b"a", b"b"], [b"a", b"b", b"c"]) == 2 and R.shared([b"a", b"b", b"c", b"d"], [b"a", b"b", b"c"]) == 3
    assert R.shared([], [b"a"]) == 0 and R.shared([b"x"], [b"a"]) == 0
    # the help example's counts, word by word
    hs = R.heads(FIX["cases"][0]["input"].encode(), False)
    prefix = R.words(hs[0][2])
    assert [R.shared(R.words(d), prefix) for _, _, d in hs[1:]] == [4, 4, 3, 3]


def test_no_description_under_the_other_id_expressions():
    """Desc is empty under --id-ncbi and under a custom --id-regexp, as written (helper.go:364-368): the first record fails"""
    data = b">gi|110645304|ref|NC_002516.2| Pseudomonas aeruginosa PAO1\nACGT\n>gi|2|ref|X| Pseudomonas aeruginosa PAO1\nAC\n"
    assert R.head_genome(data, False) == data
    with pytest.raises(R.HeadGenomeError, match=re.escape("no description: NC_002516.2")):
        R.head_genome(data, False, regexp=R.NCBI)
    with pytest.raises(R.HeadGenomeError, match=re.escape("no description: gi")):
        R.head_genome(data, False, regexp=r"^(\w+)\|")


@pytest.mark.parametrize("m", [0, -1, -(1 << 40)])
def test_option_error_at_create_time(m):
    with pytest.raises(BskError, match=re.escape(M_ERR)):
        bsk.Operator("HeadGenome", json.dumps({"MiniCommonWords": m}), -1)
    with pytest.raises(BskError, match=re.escape(M_ERR)):
        bsk.Operator("HeadGenome", bsk.SeqKitHeadGenomeOptions(mini_common_words=m).to_json(), -1)


def test_options_defaults():
    with bsk.Operator("HeadGenome", "{}", -1) as op:
        assert json.loads(op.opts_json())["MiniCommonWords"] == 1
    with bsk.Operator("HeadGenome", bsk.SeqKitHeadGenomeOptions(mini_common_words=3, line_width=7).to_json(), -1) as op:
        o = json.loads(op.opts_json())
        assert o["MiniCommonWords"] == 3 and o["Config"]["LineWidth"] == 7
    assert bsk.SeqKitHeadGenomeOptions().MiniCommonWords(2).get("MiniCommonWords") == 2


def _cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, timeout=600)


def test_command_line_flag_table():
    p = _cli("head-genome", "a.fa", "--dry-run")
    assert p.returncode == 0, p.stderr
    op, js, f = p.stdout.decode().splitlines()
    assert op == "HeadGenome" and f == "a.fa" and json.loads(js)["MiniCommonWords"] == 1
    for flag in (["-m", "3"], ["--mini-common-words", "3"], ["--mini-common-words=3"]):
        p = _cli("head-genome", *flag, "-w", "0", "a.fa", "b.fa", "--dry-run")
        assert p.returncode == 0, p.stderr
        lines = p.stdout.decode().splitlines()
        o = json.loads(lines[1])
        assert o["MiniCommonWords"] == 3 and o["Config"]["LineWidth"] == 0 and lines[2:] == ["a.fa", "b.fa"]
    p = _cli("head-genome", "--help")
    assert p.returncode == 0 and b"-m, --mini-common-words int   minimal shared prefix words (default 1)" in p.stdout
    assert b">NZ_JSTP01000001.1 Vibrio cholerae strain 2012HC-12 NODE_79" in p.stdout


@pytest.mark.parametrize("m", ["0", "-2"])
def test_command_line_refuses_m_below_one(m):
    p = _cli("head-genome", "-m", m, "a.fa")
    assert p.returncode != 0 and M_ERR in p.stderr.decode()


def test_command_line_refuses_devices_before_a_device_is_touched(tmp_path):
    """the cut is sequential over the whole input: --devices is an explicit refusal, decided on the flags alone (the file
    does not even exist)"""
    p = _cli("head-genome", str(tmp_path / "missing.fa"), "--devices", "0,1")
    err = p.stderr.decode()
    assert p.returncode != 0 and "head-genome" in err and "--devices" in err and "one device" in err
    assert "no such file" not in err and "HIP" not in err


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_use_no_scratch(tmp_path):
    src = os.path.join(ROOT, "bigseqkit_amd", "csrc", "ops_headgenome.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", str(tmp_path / "o.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = set()
    for b in r.stderr.split("Function Name: ")[1:]:
        sym = b.split(" ", 1)[0]
        for k in ("k_hg_counts", "k_hg_cut", "k_hg_finish", "k_hg_fastq_start"):
            if k in sym:
                seen.add(k)
                assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, sym
                assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, sym
    assert len(seen) == 4, seen
