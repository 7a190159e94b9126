"""Plain gzip input without a GPU (PARITY.md GZIP): the method of gzip_spec_dev.hpp with one host lane against zlib, whole and in
chunks, on the corpus and on every malformed input; the library's finder against the restatement of gzip_ref, and against the
true block starts of every file; the plan counts that the row was specified with; the compiler's resource report for the
kernels; and the header alone under the host's sanitizers."""
import ctypes as C
import os
import re
import subprocess

import pytest

import gzip_ref as G
import bigseqkit_amd as bsk
from bigseqkit_amd._lib import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
INFLATE, PLAN = bsk.GzipInflate, bsk.GzipPlan   # what this file is about


@pytest.fixture(scope="module")
def corpus():
    return {k: (data, chunk, G.expected(data)) for k, (data, chunk) in G.corpus().items()}


@pytest.fixture(scope="module")
def walks(corpus):
    return {k: G.walk(data) for k, (data, chunk, want) in corpus.items()}


def lib_find(data, chunk):
    n = (len(data) + chunk - 1) // chunk
    out = (C.c_uint64 * n)()
    assert lib.bsk_selftest_gzip_find(data, len(data), chunk, out, n) == 0
    return list(out)


def test_host_inflate_equals_zlib_whole_and_chunked(corpus, walks):
    for name, (data, chunk, want) in corpus.items():
        assert INFLATE(data, device=-1) == want, name
        assert PLAN()["chunks"] == PLAN()["on_chain"] == 1 and PLAN()["text_bytes"] == len(want), name
        assert INFLATE(data, device=-1, chunk_bytes=chunk) == want, name
        plan = PLAN()
        assert plan["chunks"] == (len(data) + chunk - 1) // chunk and plan["members"] == walks[name][1] and plan["text_bytes"] == walks[name][2] == len(want), (name, plan)
    data, _, want = corpus["three_members"]
    for chunk in (1024, 3000, 65536, 1 << 30):   # (3000: rounded down to 2048, the plan says so)
        assert INFLATE(data, device=-1, chunk_bytes=chunk) == want, chunk
        assert PLAN()["chunk_bytes"] == min(len(data), {3000: 2048}.get(chunk, chunk))
    assert INFLATE(b"", device=-1) == b""


def test_finder_equals_the_restatement(corpus):
    for name, (data, chunk, want) in corpus.items():
        assert lib_find(data, chunk) == G.find(data, chunk), name


def test_a_true_header_is_never_rejected(corpus, walks):
    """every non-final dynamic block of every file, by the walk of gzip_ref: the library's predicate takes its start (and the
    restatement does); it takes no start of a block of another kind"""
    seen = 0
    for name, (data, chunk, want) in corpus.items():
        for pos, final, btype in walks[name][0]:
            mine = lib.bsk_selftest_gzip_header_ok(data, len(data), pos)
            assert mine == (1 if (btype == 2 and not final) else 0), (name, pos, final, btype)
            if mine:
                seen += 1
                assert G.header_ok(data, pos), (name, pos)
    assert seen > 300


def test_plan_counts_as_specified(corpus, walks):
    """the level and memLevel files: the chunks behind the first and those with a candidate are the numbers the row was specified
    with, every candidate is a true block start, every one is on the chain, and at least half of the chunks are"""
    for name in list(G.LEVELS) + list(G.MEMLEVELS):
        data, chunk, want = corpus[name]
        S = lib_find(data, chunk)
        true_starts = {pos for pos, final, btype in walks[name][0]}
        found = [s for s in S[1:] if s != G.NONE]
        assert (len(S) - 1, len(found)) == G.SPECIFIED[name], name
        assert all(s in true_starts for s in found), name
        assert INFLATE(data, device=-1, chunk_bytes=chunk) == want
        plan = PLAN()
        assert (plan["with_candidate"], plan["on_chain"], plan["off_chain"], plan["dropped_bytes"]) == (len(found), len(found) + 1, 0, 0), (name, plan)
        assert 2 * (plan["on_chain"] - 1) >= len(S) - 1, (name, plan)


def test_false_candidates_only(corpus, walks):
    data, chunk, want = corpus["stored_false"]
    S = lib_find(data, chunk)
    assert [k for k, s in enumerate(S) if s != G.NONE] == [1, 2, 3, 5] and len(S) == 8
    starts = walks["stored_false"][0]
    assert [t for _, _, t in starts] == [0, 0, 0] and not ({s for s in S} & {pos for pos, _, _ in starts})
    assert INFLATE(data, device=-1, chunk_bytes=chunk) == want
    plan = PLAN()
    assert plan["with_candidate"] == 4 and plan["on_chain"] == 1 and plan["off_chain"] == 4 and plan["dropped_bytes"] > 0, plan


def test_no_candidate_at_all(corpus):
    for name in ("fixed_only", "level0", "far_32768"):
        data, chunk, want = corpus[name]
        assert INFLATE(data, device=-1, chunk_bytes=chunk) == want
        assert PLAN()["with_candidate"] == 0 and PLAN()["on_chain"] == 1 and PLAN()["chunks"] > 1, name


def test_reach_in_front_of_the_member():
    """a match in the second member that the first member's text would satisfy is refused, whole (the member's start is known)
    and in chunks (by_dictionary: through markers that name a byte in front of the member)"""
    R = G.reach_before_member()
    for name, (data, chunk) in R.items():
        for c in (0, chunk):
            with pytest.raises(bsk.BskError) as e:
                INFLATE(data, device=-1, chunk_bytes=c)
            assert e.value.code == 3 and "member 1 at offset" in str(e.value) and "distance too far back" in str(e.value), (name, c, str(e.value))
    assert "in chunk" in str(e.value)


def test_malformed_are_refused():
    good, chunk = G.corpus()["fq_l6"]
    for name, (data, c, code, words) in G.malformed().items():
        for cb in (0, c):
            with pytest.raises(bsk.BskError) as e:
                INFLATE(data, device=-1, chunk_bytes=cb)
            assert e.value.code == code and words in str(e.value), (name, cb, str(e.value))
    assert INFLATE(good, device=-1, chunk_bytes=chunk) == G.expected(good)   # and a good file afterwards is exact


def test_bgzf_calls_still_refuse_plain_gzip(corpus):
    data = corpus["fq_l6"][0]
    assert bsk.BgzfProbe(data) == 2 and bsk.BgzfProbe(corpus["bgzf_file"][0]) == 1
    with pytest.raises(bsk.BskError) as e:
        bsk.BgzfInflate(data, device=-1)
    assert e.value.code == 4 and "bgzip" in str(e.value)


CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")


def cli(args, env=None):
    e = {k: v for k, v in os.environ.items() if not k.startswith(("BSK_GZIP", "BSK_BGZF_STREAM"))}
    e.update(env or {})
    return subprocess.run([CLI, *args], capture_output=True, timeout=120, env=e)


def test_command_line_dry_run_and_refusals(tmp_path, corpus):
    """what the command line says of a plain gzip file before a device is touched, with and without BSK_GZIP"""
    z = str(tmp_path / "plain.fq.gz")
    open(z, "wb").write(corpus["ml1_l6"][0])
    on = {"BSK_GZIP": "1"}
    a, b = cli(["stats", "-a", z, "--dry-run"]), cli(["stats", "-a", z, "--dry-run"], on)
    assert a.returncode == 0 and b.returncode == 0 and a.stdout == b.stdout and z.encode() in a.stdout, (a.stderr, b.stderr)
    for args in (["stats", z], ["stats", "--devices", "0", z], ["pair", "-O", str(tmp_path / "o"), z, z]):
        r = cli(args)   # without the switch: the refusal as before, which names the switch
        assert r.returncode == 1 and b"not BGZF" in r.stderr and b"bgzip" in r.stderr and b"BSK_GZIP=1" in r.stderr, (args, r.stderr)
    r = cli(["stats", "--devices", "0", z], on)
    assert r.returncode == 1 and b"not BGZF" in r.stderr and b"--devices cuts" in r.stderr and b"virtual offsets" in r.stderr and b"bgzip" in r.stderr, r.stderr
    r = cli(["common", z, z], dict(on, BSK_COMMON_BUDGET_BYTES="1000"))
    assert r.returncode == 1 and b"not BGZF" in r.stderr and b"buckets of 'common'" in r.stderr and b"virtual offsets" in r.stderr, r.stderr
    refusals_in_full(tmp_path)


# The refusals that end without a device, whole: exit status 1 and these lines on stderr, the file's name in front.  The texts are
# those of the command line before its admission rule had one owner (recorded from that binary).
NO_SWITCH = (" is gzip but not BGZF: one gzip stream cannot be cut into independent blocks, so it is not read; recompress it with bgzip "
             "(gzip -dc FILE | bgzip > FILE.gz) or decompress it first, or set BSK_GZIP=1 to have it inflated whole, in speculative chunks, "
             "where the file and its text fit one GPU")
IN_PIECES = (" is gzip but not BGZF, and %s a file in pieces: a gzip stream has no virtual offsets to re-enter at, so BSK_GZIP=1 reads it "
             "only where a file is read whole; decompress it first (gzip -d), or recompress it with bgzip (gzip -dc FILE | bgzip > FILE.gz)")
BY_BYTES = " is BGZF-compressed, and %s a file by its bytes, which a compressed file does not allow yet; %s"
UNSET_BUDGET = ("decompress it first (bgzip -d), or unset the budget if the file and its text fit one GPU, or set BSK_BGZF_STREAM=1 to read "
                "it in record-aligned pieces, inflated once per pass")
ONE_DEVICE = "run it on one device (--device N), or decompress it first (bgzip -d)"
NO_DEVICE = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}


def refusals_in_full(tmp_path):
    """a 1-record FASTQ as plain text, as BGZF and as gzip: every refusal that is issued before a device is touched, with no
    device visible -- the whole of stderr, not words of it"""
    import bgzf_ref
    import gzip
    text = b"@r0 d=0\nACGTACGTAC\n+\nIIIIIIIIII\n"
    p, b, z = (str(tmp_path / n) for n in ("one.fq", "one.bgzf.fq.gz", "one.fq.gz"))
    open(p, "wb").write(text)
    open(b, "wb").write(bgzf_ref.write(text))
    open(z, "wb").write(gzip.compress(text, mtime=0))
    assert bsk.BgzfProbe(open(p, "rb").read()) == 0 and bsk.BgzfProbe(open(b, "rb").read()) == 1 and bsk.BgzfProbe(open(z, "rb").read()) == 2

    def refused(args, env, want):
        r = cli(args, dict(NO_DEVICE, **env))
        assert r.returncode == 1 and r.stderr.decode() == "Error: " + want + "\n", (args, env, r.stderr)

    on, stream = {"BSK_GZIP": "1"}, {"BSK_BGZF_STREAM": "1"}
    bucketed = {"concat": ["concat"], "common": ["common"], "pair": ["pair", "-O", str(tmp_path / "o")]}
    # any command on the gzip file without BSK_GZIP, whatever else is set
    for args in (["stats", z], ["seq", z], ["head-genome", z], ["stats", "--devices", "0", z], ["concat", z, z], ["common", p, z], ["pair", "-O", str(tmp_path / "o"), z, z]):
        for env in ({}, stream, {"BSK_GZIP": "0"}):
            refused(args, env, z + NO_SWITCH)
    for use, args in bucketed.items():
        budget = {"BSK_%s_BUDGET_BYTES" % use.upper(): "1"}
        buckets = "the buckets of '%s' read" % use
        refused([*args, z, z], budget, z + NO_SWITCH)
        # the buckets on a BGZF input without BSK_BGZF_STREAM (a plain file in front of it changes nothing)
        for files in ([b, b], [p, b]):
            for env in ({}, {"BSK_BGZF_STREAM": "0"}, on):
                refused([*args, *files], dict(budget, **env), b + BY_BYTES % (buckets, UNSET_BUDGET))
        # the buckets on a gzip input with BSK_GZIP=1, with and without BSK_BGZF_STREAM; gzip is refused before BGZF
        for files in ([z, z], [p, z], [b, z]):
            for env in (on, dict(on, **stream)):
                refused([*args, *files], dict(budget, **env), z + IN_PIECES % buckets)
    # --devices
    for env in ({}, stream, on, dict(on, **stream)):
        refused(["stats", "--devices", "0", b], env, b + BY_BYTES % ("--devices cuts", ONE_DEVICE))
    for env in (on, dict(on, **stream)):
        refused(["stats", "--devices", "0", z], env, z + IN_PIECES % "--devices cuts")


LDS = {"k_gz_find": 8, "k_gz_size": 3672, "k_gz_decode": 69216, "k_gz_windows": 0, "k_gz_translate": 0, "k_gz_crc": 1152}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_use_no_scratch(tmp_path):
    """the compiler's resource report for gfx950: no scratch and no spilled register in any kernel of the file.  LDS: the wave that
    sizes a chunk holds the tables and what it parked, the wave that decodes one the ring of 32 Ki symbols besides: two per CU"""
    src = os.path.join(ROOT, "bigseqkit_amd", "csrc", "ops_gzip.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", str(tmp_path / "o.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(re.findall(r"void (k_\w+)\(", open(src).read())) == sorted(LDS)          # every kernel of the file
    seen = {}
    for b in r.stderr.split("Function Name: ")[1:]:
        sym = b.split(" ", 1)[0]
        for k in LDS:
            if re.search(r"\d" + k + "E", sym):
                seen[k] = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
                assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, sym
                assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0 and int(re.search(r"SGPRs Spill: (\d+)", b).group(1)) == 0, sym
    assert seen == LDS, seen
    assert 2 * LDS["k_gz_decode"] <= 160 * 1024


def test_method_under_sanitizers(tmp_path, corpus):
    """tests/host_c/gzip_host_check.cpp -- the header and nothing of the library -- built with the host's address and
    undefined-behaviour sanitizers: exact on the corpus whole and in chunks, a refusal on every malformed input, the finder
    equal to the decoder bit by bit, and no report"""
    exe = str(tmp_path / "gzip_host_check")
    src = os.path.join(ROOT, "tests", "host_c", "gzip_host_check.cpp")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("the sanitizer runtime cannot be linked here")
    assert r.returncode == 0, r.stderr[-2000:]
    for name, (data, chunk, want) in corpus.items():
        (tmp_path / "in").write_bytes(data)
        (tmp_path / "want").write_bytes(want)
        p = subprocess.run([exe, str(tmp_path / "in"), str(tmp_path / "want"), str(chunk)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and p.stdout.startswith("ok ") and not p.stderr, (name, p.stdout, p.stderr[-2000:])
    bad = {k: (d, c) for k, (d, c, _, _) in G.malformed().items()}
    bad.update(G.reach_before_member())
    for name, (data, chunk) in bad.items():
        (tmp_path / "in").write_bytes(data)
        p = subprocess.run([exe, str(tmp_path / "in"), "-", str(chunk)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and p.stdout.startswith("refused ") and not p.stderr, (name, p.stdout, p.stderr[-2000:])
