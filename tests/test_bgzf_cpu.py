"""BGZF input without a GPU (PARITY.md BGZF): the restatement against zlib, what the corpus exercises, the decoder of
bgzf_inflate_dev.hpp on host threads against zlib and on every malformed input, the probe, the chunked CRC, the compiler's
resource report for the kernels, and the decoder alone under the host's sanitizers."""
import ctypes as C
import gzip
import os
import re
import subprocess
import zlib

import pytest

import bgzf_ref as R
import bigseqkit_amd as bsk
from bigseqkit_amd._lib import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
INFLATE = bsk.BgzfInflate   # what this file is about: without the BGZF entry points there is nothing to compare


@pytest.fixture(scope="module")
def corpus():
    files = R.corpus()
    return {k: (v, gzip.decompress(v) if v else b"") for k, v in files.items()}


@pytest.fixture(scope="module")
def bad():
    return R.malformed()


def test_ref_equals_zlib_and_corpus_covers(corpus):
    """the restatement inflates the corpus to zlib's bytes, and every member exercises what it is there for"""
    repeats, reports = set(), {}
    for name, (data, want) in corpus.items():
        got, rep = R.inflate(data)
        assert got == want, name
        reports[name] = rep
        repeats |= rep.repeat_codes
    assert set(R.EXPECT) <= set(corpus)
    for name, holds in R.EXPECT.items():
        assert holds(reports[name]), (name, vars(reports[name]))
    assert repeats == {16, 17, 18}
    assert max(r.max_code_len for r in reports.values()) >= 13
    assert R.EOF_BLOCK == R.member(R.deflate(b""), b"") and len(R.EOF_BLOCK) == 28   # the standard empty block


def test_host_inflate_equals_zlib(corpus):
    for name, (data, want) in corpus.items():
        assert INFLATE(data, device=-1) == want, name


def test_host_inflate_refuses_malformed(bad):
    M, good, text = bad
    assert INFLATE(good, device=-1) == text
    for name, (data, code, block, word) in M.items():
        with pytest.raises(bsk.BskError) as e:
            INFLATE(data, device=-1)
        assert e.value.code == code, (name, str(e.value))
        if block is not None:
            assert ("block %d at offset" % block) in str(e.value), (name, str(e.value))
        assert word in str(e.value), (name, str(e.value))
        if name not in ("bsize_past_end", "plain_gzip"):   # zlib refuses them too (it does not read BSIZE, and plain gzip is its own)
            with pytest.raises(Exception):
                gzip.decompress(data)
    assert INFLATE(good, device=-1) == text   # and a good file afterwards is exact


def test_size_query_and_capacity(corpus):
    data, want = corpus["fq_l6"]
    n = C.c_size_t()
    assert lib.bsk_bgzf_inflate_host(data, len(data), None, 0, C.byref(n), 1) == 0 and n.value == len(want)
    buf = C.create_string_buffer(100)
    assert lib.bsk_bgzf_inflate_host(data, len(data), buf, 100, C.byref(n), 1) == 7   # BSK_ERR_CAPACITY


def test_probe(corpus):
    data = corpus["fq_l6"][0]
    assert bsk.BgzfProbe(data) == 1 and bsk.BgzfProbe(corpus["extra_subfields"][0]) == 1 and bsk.BgzfProbe(R.EOF_BLOCK) == 1
    assert bsk.BgzfProbe(gzip.compress(b"@r\nACGT\n+\nIIII\n")) == 2
    assert bsk.BgzfProbe(b">seq1\nACGT\n") == 0 and bsk.BgzfProbe(b"@r\nACGT\n+\nIIII\n") == 0
    # 0 .. 17 bytes of a BGZF file: nothing is gzip before the magic is there, and BGZF needs the whole BC subfield
    for k in range(18):
        assert bsk.BgzfProbe(data[:k]) == (0 if k < 2 else 2), k
    assert bsk.BgzfProbe(data[:18]) == 1


def test_chunked_crc():
    """1 KiB chunks from the end, folded with the advance operator: zlib's CRC32 at every length around the chunk borders"""
    import random
    rng = random.Random(11)
    for n in (0, 1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 65535, 65536):
        d = rng.randbytes(n)
        assert lib.bsk_selftest_bgzf_crc(d, n) == zlib.crc32(d), n


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_use_no_scratch(tmp_path):
    """the compiler's resource report for gfx950: no scratch and no spilled register in any kernel of the file.  LDS: the wave
    that inflates a block holds the 32 KiB window, the two decode tables with their canonical codes, the code lengths, the CRC
    table and the advance operator, 37 504 bytes: four waves per CU; the others none"""
    src = os.path.join(ROOT, "bigseqkit_amd", "csrc", "ops_bgzf.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", str(tmp_path / "o.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want = {"k_bgzf_find": 0, "k_bgzf_sizes": 0, "k_bgzf_desc": 0, "k_bgzf_inflate": 37504}
    assert sorted(re.findall(r"void (k_\w+)\(", open(src).read())) == sorted(want)          # every kernel of the file
    seen = {}
    for b in r.stderr.split("Function Name: ")[1:]:
        sym = b.split(" ", 1)[0]
        for k in want:
            if re.search(r"\d" + k + "E", sym):
                seen[k] = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
                assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, sym
                assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0 and int(re.search(r"SGPRs Spill: (\d+)", b).group(1)) == 0, sym
    assert seen == want, seen
    assert 4 * want["k_bgzf_inflate"] <= 160 * 1024


def test_decoder_under_sanitizers(tmp_path, corpus, bad):
    """tests/host_c/bgzf_host_check.cpp -- the decoder header and nothing of the library -- built with the host's address and
    undefined-behaviour sanitizers: exact on the corpus, a refusal on every malformed input, and no report"""
    exe = str(tmp_path / "bgzf_host_check")
    src = os.path.join(ROOT, "tests", "host_c", "bgzf_host_check.cpp")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("the sanitizer runtime cannot be linked here")
    assert r.returncode == 0, r.stderr[-2000:]
    for name, (data, want) in corpus.items():
        (tmp_path / "in").write_bytes(data)
        (tmp_path / "want").write_bytes(want)
        p = subprocess.run([exe, str(tmp_path / "in"), str(tmp_path / "want")], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and p.stdout.startswith("ok ") and not p.stderr, (name, p.stdout, p.stderr[-2000:])
    for name, (data, code, block, word) in bad[0].items():
        (tmp_path / "in").write_bytes(data)
        p = subprocess.run([exe, str(tmp_path / "in"), "-"], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and p.stdout.startswith("refused ") and not p.stderr, (name, p.stdout, p.stderr[-2000:])
        if block is not None:
            assert int(p.stdout.split()[1]) == block, (name, p.stdout)
