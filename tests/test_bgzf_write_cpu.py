"""BGZF output without a GPU (PARITY.md BGZFW): the encoder of bgzf_deflate_dev.hpp on host threads -- the bytes the kernel
writes, lane count being no part of their definition -- judged by zlib on every text of the corpus; what keeps a do-nothing
encoder from passing; the size against `bgzip -l 1` of the same blocks; the compiler's resource report for the kernels; and
the encoder and the decoder alone under the host's sanitizers."""
import ctypes as C
import gzip
import os
import re
import subprocess

import pytest

import bgzf_ref as R
import bgzf_write_corpus as W
import bigseqkit_amd as bsk
from bigseqkit_amd._lib import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
DEFLATE = bsk.BgzfDeflateHost   # what this file is about


@pytest.fixture(scope="module")
def corpus():
    return W.build()


@pytest.fixture(scope="module")
def encoded(corpus):
    """every text once, with the EOF block, on 8 threads"""
    return {name: DEFLATE(text, 0, True, 8) for name, (text, _) in corpus.items()}


def test_every_text_is_exact_and_well_formed(corpus, encoded):
    for name, (text, _) in corpus.items():
        out = encoded[name]
        W.check_file(out, text, W.BT, True)
        assert bsk.BgzfInflate(out, device=-1) == text, name
        assert len(out) <= lib.bsk_bgzf_deflate_bound(len(text), 0), name
        assert DEFLATE(text, 0, True, 1) == out, name           # 1 thread and 8 threads: the same bytes
        bare = DEFLATE(text, 0, False, 8)
        assert bare == out[:-28], name
        W.check_file(bare, text, W.BT, False)
    assert encoded["empty"] == R.EOF_BLOCK and DEFLATE(b"", 0, False) == b""


def test_small_blocks_and_pieces():
    """97 bytes of text a block: over 5 000 blocks; and pieces without EOF, one EOF block behind them, are one file"""
    text = W.fastq_500k()
    out = DEFLATE(text, 97, True, 8)
    W.check_file(out, text, 97, True)
    assert len(R.index(out)) - 1 > 5000
    assert DEFLATE(text, 97, True, 1) == out
    assert bsk.BgzfInflate(out, device=-1) == text
    assert len(out) <= lib.bsk_bgzf_deflate_bound(len(text), 97)
    big = DEFLATE(text, W.BT, True, 8)
    W.check_file(big, text, W.BT, True)
    cut = 3 * W.BT
    joined = DEFLATE(text[:cut], 0, False) + DEFLATE(text[cut:], 0, False) + DEFLATE(b"", 0, True)
    assert joined == big and gzip.decompress(joined) == text


def test_block_bytes_are_checked():
    n = C.c_size_t()
    buf = C.create_string_buffer(1000)
    assert lib.bsk_bgzf_deflate_host(b"abc", 3, 65281, 1, buf, 1000, C.byref(n), 1) == 1   # BSK_ERR_INVALID_ARG
    assert lib.bsk_bgzf_deflate_host(b"abc" * 100, 300, 0, 1, buf, 10, C.byref(n), 1) == 7   # BSK_ERR_CAPACITY
    assert n.value > 10                                                                      # ... and what it needs
    assert lib.bsk_bgzf_deflate_bound(0, 0) == 28 and lib.bsk_bgzf_deflate_bound(65281, 0) == 65281 + 2 * 31 + 28


def test_a_do_nothing_encoder_fails(corpus, encoded):
    """derivable, not measured: a constant block needs matches (even matches capped at 64 bytes cost under 20 bits each with
    fixed codes: 2.5 KB); random ACGT needs dynamic codes (literals at about 2.25 bits and a header: fixed codes and stored
    both miss 0.40); random bytes need the stored form"""
    assert len(encoded["constant"]) - 28 < 4096
    assert len(encoded["acgt"]) - 28 < 0.40 * len(corpus["acgt"][0])
    assert len(encoded["random"]) - 28 <= len(corpus["random"][0]) + 31
    # the only repeat lies 32 768 back: used (noise alone cannot beat the stored form); 32 769 back: out of reach, stored
    assert len(encoded["far32768"]) - 28 < len(corpus["far32768"][0]) + 31 - 100
    assert len(encoded["far32769"]) - 28 == len(corpus["far32769"][0]) + 31
    # 700 equal bytes: two matches of 258 and a shorter one, not 700 literals and not eleven matches of 64
    assert len(encoded["run258"]) - 28 < 200


def test_size_against_level_1(corpus, encoded):
    """the yardstick is zlib level 1 on the same blocks (what bgzip -l 1 writes): at most 15 % above it, and 64 bytes a block
    for the header choices of tiny outputs"""
    texts = {name: text for name, (text, kind) in corpus.items() if kind == "ratio"}
    texts["fastq_500k"] = W.fastq_500k()
    for name, text in sorted(texts.items()):
        ours = len(encoded[name] if name in encoded else DEFLATE(text, 0, True, 8)) - 28
        ref1, ref6 = W.level1_blocks(text), W.level1_blocks(text, level=6)
        nblocks = (len(text) + W.BT - 1) // W.BT
        print("%-16s text %7d  ours %7d (%.4f)  level 1 %7d (%.4f)  level 6 %7d (%.4f)" % (name, len(text), ours, ours / len(text), ref1, ref1 / len(text), ref6, ref6 / len(text)))
        assert ours <= 1.15 * ref1 + 64 * nblocks, name


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_use_no_scratch(tmp_path):
    """the compiler's resource report for gfx950: no scratch and no spilled register in any kernel of the file.  LDS: the wave
    that encodes a block holds the hash table (32 KiB), the histograms, the codes and the bits of 64 tokens on their way out,
    40 540 bytes: four waves per CU; the pack kernel none"""
    src = os.path.join(ROOT, "bigseqkit_amd", "csrc", "ops_bgzf_write.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", str(tmp_path / "o.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want = {"k_bgzf_deflate": 40540, "k_bgzf_pack": 0}
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
    assert 4 * want["k_bgzf_deflate"] <= 160 * 1024


def test_encoder_under_sanitizers(tmp_path, corpus, encoded):
    """tests/host_c/bgzf_deflate_check.cpp -- the two BGZF headers and nothing of the library -- built with the host's address
    and undefined-behaviour sanitizers: every text encoded, decoded back and compared, no report, and the library's bytes"""
    exe = str(tmp_path / "bgzf_deflate_check")
    src = os.path.join(ROOT, "tests", "host_c", "bgzf_deflate_check.cpp")
    flags = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # (is the runtime there?  Asked of an empty program BEFORE the check is built: a failure to build the check is a failure)
    (tmp_path / "empty.cpp").write_text("int main() { return 0; }\n")
    if subprocess.run(flags + ["-o", str(tmp_path / "empty"), str(tmp_path / "empty.cpp")], capture_output=True, timeout=600).returncode != 0:
        pytest.skip("the sanitizer runtime cannot be linked here")
    r = subprocess.run(flags + ["-o", exe, src], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for name, (text, _) in corpus.items():
        (tmp_path / "in").write_bytes(text)
        p = subprocess.run([exe, "-o", str(tmp_path / "out"), str(tmp_path / "in")], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and p.stdout.startswith("ok ") and not p.stderr, (name, p.stdout, p.stderr[-2000:])
        assert (tmp_path / "out").read_bytes() == encoded[name], name
    (tmp_path / "in").write_bytes(W.fastq_500k()[:100000])
    p = subprocess.run([exe, "-b", "97", str(tmp_path / "in")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("ok ") and not p.stderr, (p.stdout, p.stderr[-2000:])
