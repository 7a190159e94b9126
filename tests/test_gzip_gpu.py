"""Plain gzip input on the GPU (PARITY.md GZIP): k_gz_find / k_gz_size / k_gz_decode / k_gz_windows / k_gz_translate / k_gz_crc
against zlib on the corpus of gzip_ref, each file at the chunk size it is there for, with the plan counts that keep a test
from passing by chunk 0 decoding everything, and through ReadSeqFile(gzip=True) and the operators."""
import gzip
import json
import os
import subprocess

import pytest
import torch

import bgzf_ref as B
import gzip_ref as G
import bigseqkit_amd as bsk
import oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")
INFLATE, PLAN = bsk.GzipInflate, bsk.GzipPlan
BSK_ERR_UNSUPPORTED = 4


class _Opts:
    def __init__(self, d):
        self.d = dict(d)
        self._v = self.d

    def to_json(self):
        return json.dumps(self.d)


def host(t):
    return bytes(t.cpu().numpy().tobytes())


@pytest.fixture(scope="module")
def corpus():
    return {k: (data, chunk, G.expected(data)) for k, (data, chunk) in G.corpus().items()}


def test_corpus_same_text_and_same_plan_as_the_host_path(corpus):
    for name, (data, chunk, want) in corpus.items():
        got = INFLATE(data, chunk_bytes=chunk)
        plan = PLAN()
        assert got.is_cuda and got.dtype == torch.uint8 and host(got) == want, name
        assert INFLATE(data, device=-1, chunk_bytes=chunk) == want, name
        assert PLAN() == plan, name
        assert plan["text_bytes"] == len(want) and plan["chunk_bytes"] == min(chunk, len(data)), name


def test_chain_share(corpus):
    """the level and memLevel files are decoded by their chunks, not by chunk 0: the counts are those of the reference finder,
    every candidate is on the chain, at least half of the chunks behind the first are"""
    for name in list(G.LEVELS) + list(G.MEMLEVELS):
        data, chunk, want = corpus[name]
        S = G.find(data, chunk)
        behind, found = len(S) - 1, sum(1 for s in S[1:] if s != G.NONE)
        assert (behind, found) == G.SPECIFIED[name], name
        assert host(INFLATE(data, chunk_bytes=chunk)) == want, name
        plan = PLAN()
        assert (plan["chunks"], plan["with_candidate"], plan["on_chain"], plan["off_chain"]) == (behind + 1, found, found + 1, 0), (name, plan)
        assert 2 * (plan["on_chain"] - 1) >= behind, (name, plan)


def test_false_candidates_only(corpus):
    data, chunk, want = corpus["stored_false"]
    assert host(INFLATE(data, chunk_bytes=chunk)) == want
    plan = PLAN()
    assert plan["chunks"] == 8 and plan["with_candidate"] >= 3 and plan["on_chain"] == 1 and plan["off_chain"] == plan["with_candidate"], plan
    assert plan["dropped_bytes"] > 0


def test_the_text_does_not_depend_on_the_chunk_size(corpus):
    data, _, want = corpus["three_members"]
    for chunk in (1024, 4096, 65536, 0):
        assert host(INFLATE(data, chunk_bytes=chunk)) == want, chunk
    assert PLAN()["chunks"] == 1   # (the default: at least 256 KiB, the file is smaller)
    # from a device tensor that does not begin on a 16-byte boundary
    shifted = torch.frombuffer(bytearray(b"\0" + data), dtype=torch.uint8).cuda()[1:]
    assert shifted.data_ptr() % 16 != 0 and host(INFLATE(shifted, chunk_bytes=4096)) == want
    assert INFLATE(b"").numel() == 0


def test_reach_in_front_of_the_member():
    for name, (data, chunk) in G.reach_before_member().items():
        for c in (0, chunk):
            with pytest.raises(bsk.BskError) as e:
                INFLATE(data, chunk_bytes=c)
            assert e.value.code == 3 and "member 1 at offset" in str(e.value) and "distance too far back" in str(e.value), (name, c, str(e.value))
            if c:
                with pytest.raises(bsk.BskError) as h:
                    INFLATE(data, device=-1, chunk_bytes=c)
                assert str(h.value) == str(e.value), name
    assert "in chunk" in str(e.value)   # (by_dictionary in chunks: found through the markers)


def test_malformed_same_refusal_as_the_host_path(corpus):
    good, chunk, want = corpus["fq_l6"]
    for name, (data, c, code, words) in G.malformed().items():
        with pytest.raises(bsk.BskError) as e:
            INFLATE(data, chunk_bytes=c)
        assert e.value.code == code and words in str(e.value), (name, str(e.value))
        with pytest.raises(bsk.BskError) as h:
            INFLATE(data, device=-1, chunk_bytes=c)
        assert str(h.value) == str(e.value) and h.value.code == code, name
    assert host(INFLATE(good, chunk_bytes=chunk)) == want   # and a good file afterwards is exact


@pytest.fixture(scope="module")
def seqfiles(tmp_path_factory):
    d = tmp_path_factory.mktemp("gzip")
    fq, fa = B.fastq_text(150000, seed=21), B.fasta_text(150000, seed=22)
    fq += fq[:fq.index(b"@read3/")]      # the first three records once more, for rmdup
    out = {}
    for name, text in (("x.fq", fq), ("x.fa", fa)):
        (d / name).write_bytes(text)
        (d / (name + ".gz")).write_bytes(gzip.compress(text))
        (d / (name + ".bgzf.gz")).write_bytes(B.write(text))
        out[name] = (str(d / name), str(d / (name + ".gz")), text)
        out[name + ".bgzf"] = str(d / (name + ".bgzf.gz"))
    out["dir"] = d
    return out


@pytest.mark.parametrize("name", ["x.fq", "x.fa"])
def test_through_the_operators(seqfiles, name, monkeypatch):
    plain, gz, text = seqfiles[name]
    fastq = name.endswith("fq")
    monkeypatch.setenv("BSK_GZIP_CHUNK_BYTES", "4096")   # (the default would make one chunk of so small a file)
    z, p = bsk.ReadSeqFile(gz, gzip=True), bsk.ReadSeqFile(plain)
    assert PLAN()["chunk_bytes"] == 4096 and PLAN()["chunks"] > 8 and (PLAN()["on_chain"] > 1 or not fastq)   # (zlib cuts the FASTA into few blocks)
    assert z.format == p.format == (bsk.FORMAT_FASTQ if fastq else bsk.FORMAT_FASTA)
    assert z.shards[0].is_cuda and host(z.shards[0]) == text
    o = bsk.SeqKitStatsOptions().All(True).Tabular(True)
    want = oracle.stats_string(text, fastq, json.dumps({"All": True, "Tabular": True}))
    assert bsk.StatsString("input0", "N/A", z, o) == bsk.StatsString("input0", "N/A", p, o) == want
    for fn, ofn, opts in ((bsk.Seq, oracle.seq, {"Name": True}), (bsk.Grep, oracle.grep, {"Pattern": ["ACGTAC"], "BySeq": True}),
                          (bsk.RmDup, oracle.rmdup, {"BySeq": True})):
        assert fn(z, _Opts(opts)) == fn(p, _Opts(opts)) == ofn(text, fastq, json.dumps(opts)), fn.__name__
    with pytest.raises(bsk.BskError) as e:
        bsk.ReadSeqFile(gz)
    assert e.value.code == BSK_ERR_UNSUPPORTED and "bgzip" in str(e.value)


# ---- the command line under BSK_GZIP=1 (plain.fq.gz is what `gzip` writes: one member)
GZ = {"BSK_GZIP": "1", "BSK_GZIP_CHUNK_BYTES": "4096"}


def cli(args, env=None):
    e = {k: v for k, v in os.environ.items() if not k.startswith("BSK_GZIP")}
    e.update(env or {})
    return subprocess.run([CLI, *args], capture_output=True, timeout=300, env=e)


@pytest.mark.parametrize("args", [["stats", "-a", "-T"], ["seq", "-n", "-o", "-"], ["grep", "-s", "-p", "ACGTAC", "-o", "-"], ["rmdup", "-s", "-o", "-"]])
def test_command_line(seqfiles, args):
    """the command on the gzip file writes what it writes on the plain one"""
    plain, z, _ = seqfiles["x.fq"]
    a, b = cli(args + [plain]), cli(args + [z], GZ)
    assert a.returncode == 0 and b.returncode == 0, (args, a.stderr, b.stderr)
    if args[0] == "stats":   # (the file column differs by the name)
        assert a.stdout.replace(plain.encode(), b"F") == b.stdout.replace(z.encode(), b"F") and a.stdout, args
    else:
        assert a.stdout == b.stdout and a.stdout, args


def test_command_line_mixed_inputs(seqfiles):
    """three inputs: plain, BGZF and gzip"""
    fq, fqz, _ = seqfiles["x.fq"]
    a, b = cli(["seq", "-n", "-o", "-", fq, fq, fq]), cli(["seq", "-n", "-o", "-", fq, seqfiles["x.fq.bgzf"], fqz], GZ)
    assert a.returncode == 0 and b.returncode == 0 and a.stdout == b.stdout and a.stdout, (a.stderr, b.stderr)


def test_command_line_pair_on_host_strings(seqfiles):
    """pair keeps its inputs in host strings: the same method with one host lane"""
    fa, faz, _ = seqfiles["x.fa"]
    d = seqfiles["dir"]
    for out, files, env in (("p_plain", [fa, fa], None), ("p_gz", [faz, fa], GZ)):
        r = cli(["pair", "-u", "-O", str(d / out), *files], env)
        assert r.returncode == 0, r.stderr
    for n in ("paired.1", "paired.2", "unpaired.1", "unpaired.2"):
        assert (d / "p_plain" / n).read_bytes() == (d / "p_gz" / n).read_bytes(), n
    assert (d / "p_gz" / "paired.1").stat().st_size > 0


def test_command_line_gzip_in_gz_out(seqfiles):
    """seq reads.fq.gz -o kept.fq.gz --merge: a gzip input, a BGZF output that gzip reads back"""
    fq, fqz, _ = seqfiles["x.fq"]
    d = seqfiles["dir"]
    a, b = cli(["seq", fq, "-o", str(d / "kept.fq"), "--merge"]), cli(["seq", fqz, "-o", str(d / "kept.fq.gz"), "--merge"], GZ)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    want = (d / "kept.fq").read_bytes()
    assert want and gzip.decompress((d / "kept.fq.gz").read_bytes()) == want
    assert bsk.BgzfProbe((d / "kept.fq.gz").read_bytes()) == 1


def test_command_line_refusals(seqfiles):
    """the whole of stderr, as test_gzip_cpu.py holds it for the refusals that need no device"""
    from test_gzip_cpu import NO_SWITCH, IN_PIECES
    _, fqz, _ = seqfiles["x.fq"]
    said = lambda r, want: r.returncode == 1 and r.stderr.decode() == "Error: " + fqz + want + "\n"
    r = cli(["stats", fqz])   # without the switch: as before, and the message names the switch
    assert said(r, NO_SWITCH) and b"bgzip" in r.stderr and b"BSK_GZIP=1" in r.stderr, r.stderr
    # with it, the paths that read a file in pieces still refuse, and say what to do instead
    r = cli(["stats", "--devices", "0", fqz], GZ)
    assert said(r, IN_PIECES % "--devices cuts") and b"virtual offsets" in r.stderr and b"bgzip" in r.stderr, r.stderr
    for stream in ({}, {"BSK_BGZF_STREAM": "1"}):
        r = cli(["sort", fqz], dict(GZ, BSK_SORT_BUDGET_BYTES="1000", BSK_HOST_PIPELINE_FROM="0", **stream))
        assert said(r, IN_PIECES % "the buckets of 'sort' read"), r.stderr
    r = cli(["stats", fqz], dict(GZ, BSK_HOST_PIPELINE_FROM="0"))
    assert said(r, IN_PIECES % "'stats' streams"), r.stderr
    with pytest.raises(bsk.BskError) as e:   # the piece reader itself, at its first piece
        with bsk.BgzfReader(fqz, bsk.FORMAT_FASTQ) as r:
            list(r)
    assert e.value.code == BSK_ERR_UNSUPPORTED and "bgzip" in str(e.value)
