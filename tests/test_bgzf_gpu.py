"""BGZF input on the GPU (PARITY.md BGZF): k_bgzf_find / k_bgzf_sizes / k_bgzf_inflate against zlib on the corpus of
tests/bgzf_ref.py (whose reports test_bgzf_cpu.py asserts), the refusals of the malformed inputs -- which the decoder has passed
under the host's sanitizers there -- and compressed files through the operators and the command line."""
import gzip
import json
import os
import subprocess

import pytest
import torch

import bgzf_ref as R
import bigseqkit_amd as bsk
import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")
BSK_ERR_FORMAT, BSK_ERR_UNSUPPORTED = 3, 4


class _Opts:
    def __init__(self, d):
        self.d = dict(d)
        self._v = self.d   # (Grep forces Count off in the option object)

    def to_json(self):
        return json.dumps(self.d)


def host(t):
    return bytes(t.cpu().numpy().tobytes())


def dev(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda() if len(b) else torch.empty(0, dtype=torch.uint8, device="cuda")


@pytest.fixture(scope="module")
def corpus():
    files = R.corpus()
    return {k: (v, gzip.decompress(v) if v else b"") for k, v in files.items()}


def test_corpus_from_bytes(corpus):
    for name, (data, want) in corpus.items():
        got = bsk.BgzfInflate(data)
        assert got.is_cuda and got.dtype == torch.uint8 and host(got) == want, name


def test_corpus_from_device_tensor(corpus):
    for name, (data, want) in corpus.items():
        assert host(bsk.BgzfInflate(dev(data))) == want, name
    # a buffer that does not begin on a 16-byte boundary (the kernels load 16 bytes at a time): a view one byte into a tensor
    data, want = corpus["fq_l6"]
    shifted = dev(b"\x00" + data)[1:]
    assert shifted.data_ptr() % 16 != 0 and host(bsk.BgzfInflate(shifted)) == want


def test_many_small_blocks(corpus):
    """more blocks than waves the chip holds at once: 3 * CUs * 4 + 1 blocks of 10 bytes"""
    n = 3 * torch.cuda.get_device_properties(0).multi_processor_count * 4 + 1
    text = (R.fastq_text(4000) * (10 * n // 4000 + 1))[:10 * n]
    data = R.write(text, block=10)
    assert host(bsk.BgzfInflate(data)) == text
    ix = bsk.BgzfBlocks(data)
    assert len(ix) == n + 1 and ix == [(o, c, u) for o, c, u, _ in R.index(data)]


def test_more_headers_than_the_first_list_holds():
    """5 000 empty blocks in 140 KB: more hits than k_bgzf_find's first list is sized for, so it runs once more, to size"""
    text = R.fastq_text(3000, seed=31)
    data = R.EOF_BLOCK * 5000 + R.member(R.deflate(text), text) + R.EOF_BLOCK
    assert host(bsk.BgzfInflate(data)) == text and len(bsk.BgzfBlocks(data)) == 5002


def test_block_index(corpus):
    """the index is the chain from offset 0 -- a header's 16 bytes inside a stored block are found and are not on it, a header
    with other subfields is read from its own bytes"""
    for name in ("signature_in_stored", "extra_subfields", "empty_blocks", "fq_l6", "eof_alone", "zero_bytes", "no_eof"):
        data = corpus[name][0]
        assert bsk.BgzfBlocks(data) == [(o, c, u) for o, c, u, _ in R.index(data)], name
    assert corpus["signature_in_stored"][0].count(R.HEADER_SIGNATURE) > len(R.index(corpus["signature_in_stored"][0]))
    assert bsk.BgzfBlocks(b"") == [] and bsk.BgzfInflate(b"").numel() == 0 and bsk.BgzfInflate(R.EOF_BLOCK).numel() == 0


def test_malformed_are_refused_and_a_good_file_is_exact_afterwards():
    M, good, text = R.malformed()
    assert host(bsk.BgzfInflate(good)) == text
    for name, (data, code, block, word) in M.items():
        with pytest.raises(bsk.BskError) as e:
            bsk.BgzfInflate(data)
        assert e.value.code == code, (name, str(e.value))
        if block is not None:
            assert ("block %d at offset" % block) in str(e.value), (name, str(e.value))
        assert word in str(e.value), (name, str(e.value))
        # the device and the host name the same block and the same reason
        with pytest.raises(bsk.BskError) as h:
            bsk.BgzfInflate(data, device=-1)
        assert str(h.value) == str(e.value), name
    assert host(bsk.BgzfInflate(good)) == text


@pytest.fixture(scope="module")
def seqfiles(tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzf")
    fq, fa = R.fastq_text(150000, seed=21), R.fasta_text(150000, seed=22)
    fq += fq[:fq.index(b"@read3/")]      # the first three records once more, for rmdup
    out = {}
    for name, text in (("x.fq", fq), ("x.fa", fa)):
        (d / name).write_bytes(text)
        (d / (name + ".gz")).write_bytes(R.write(text))
        out[name] = (str(d / name), str(d / (name + ".gz")), text)
    (d / "plain.fq.gz").write_bytes(gzip.compress(fq))
    out["plain_gzip"] = str(d / "plain.fq.gz")
    out["dir"] = d
    return out


@pytest.mark.parametrize("name", ["x.fq", "x.fa"])
def test_through_the_operators(seqfiles, name):
    plain, gz, text = seqfiles[name]
    fastq = name.endswith("fq")
    z, p = bsk.ReadSeqFile(gz), bsk.ReadSeqFile(plain)
    assert z.format == p.format == (bsk.FORMAT_FASTQ if fastq else bsk.FORMAT_FASTA)
    assert z.shards[0].is_cuda and host(z.shards[0]) == text
    so = {"All": True, "Tabular": True}
    want = oracle.stats_string(text, fastq, json.dumps(so))
    o = bsk.SeqKitStatsOptions().All(True).Tabular(True)
    assert bsk.StatsString("input0", "N/A", z, o) == bsk.StatsString("input0", "N/A", p, o) == want
    for fn, ofn, opts in ((bsk.Seq, oracle.seq, {"Name": True}), (bsk.Grep, oracle.grep, {"Pattern": ["ACGTAC"], "BySeq": True}),
                          (bsk.RmDup, oracle.rmdup, {"BySeq": True})):
        got = fn(z, _Opts(opts))
        assert got == fn(p, _Opts(opts)) == ofn(text, fastq, json.dumps(opts)), fn.__name__
    with pytest.raises(bsk.BskError) as e:
        bsk.ReadSeqFile(seqfiles["plain_gzip"])
    assert e.value.code == BSK_ERR_UNSUPPORTED and "bgzip" in str(e.value)


def cli(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([CLI, *args], capture_output=True, timeout=300, env=e)


@pytest.mark.parametrize("args,name", [(["stats", "-a", "-T"], "x.fq"), (["seq", "-n", "-o", "-"], "x.fq"),
                                       (["grep", "-s", "-p", "ACGTAC", "-o", "-"], "x.fq"), (["rmdup", "-s", "-o", "-"], "x.fq"),
                                       (["stats", "-a", "-T"], "x.fa"), (["seq", "-n", "-o", "-"], "x.fa")])
def test_command_line(seqfiles, args, name):
    """the command on the compressed file writes what it writes on the plain one"""
    plain, z, _ = seqfiles[name]
    a, b = cli(args + [plain]), cli(args + [z])
    assert a.returncode == 0 and b.returncode == 0, (args, a.stderr, b.stderr)
    if args[0] == "stats":   # (the file column differs by the name)
        assert a.stdout.replace(plain.encode(), b"F") == b.stdout.replace(z.encode(), b"F") and a.stdout, args
    else:
        assert a.stdout == b.stdout and a.stdout, args


def test_command_line_mixed_inputs(seqfiles):
    """two inputs, one plain and one compressed"""
    fq, fqz, _ = seqfiles["x.fq"]
    a, b = cli(["seq", "-n", "-o", "-", fq, fq]), cli(["seq", "-n", "-o", "-", fq, fqz])
    assert a.returncode == 0 and b.returncode == 0 and a.stdout == b.stdout and a.stdout, (a.stderr, b.stderr)


def test_command_line_pair_on_host_strings(seqfiles):
    """pair keeps its inputs in host strings: the same decoder on host threads"""
    fa, faz, _ = seqfiles["x.fa"]
    d = seqfiles["dir"]
    for out, files in (("p_plain", [fa, fa]), ("p_gz", [faz, fa])):
        r = cli(["pair", "-u", "-O", str(d / out), *files])
        assert r.returncode == 0, r.stderr
    for n in ("paired.1", "paired.2", "unpaired.1", "unpaired.2"):
        assert (d / "p_plain" / n).read_bytes() == (d / "p_gz" / n).read_bytes(), n
    assert (d / "p_gz" / "paired.1").stat().st_size > 0


def test_command_line_refusals(seqfiles):
    _, fqz, _ = seqfiles["x.fq"]
    r = cli(["stats", seqfiles["plain_gzip"]])
    assert r.returncode == 1 and b"bgzip" in r.stderr and b"not BGZF" in r.stderr
    r = cli(["stats", "--devices", "0", fqz])
    assert r.returncode == 1 and b"BGZF-compressed" in r.stderr and b"--devices" in r.stderr and b"--device N" in r.stderr
    r = cli(["sort", fqz], env={"BSK_SORT_BUDGET_BYTES": "1000", "BSK_HOST_PIPELINE_FROM": "0"})
    assert r.returncode == 1 and b"BGZF-compressed" in r.stderr and b"buckets of 'sort'" in r.stderr and b"bgzip -d" in r.stderr
    r = cli(["stats", fqz], env={"BSK_HOST_PIPELINE_FROM": "0"})
    assert r.returncode == 1 and b"BGZF-compressed" in r.stderr and b"streams" in r.stderr
