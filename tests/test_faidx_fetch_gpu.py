"""`faidx -d` on the device (PARITY.md FAIX): the fetch kernel against oracle.faidx_query on the plain text and against
bsk.FaidxQuery on the whole file, over the shapes of fai_fetch_ref.cases (T from bsk_faidx_fetch_info / the plan); the
refusals of an index that does not fit its file; independence of every byte outside the plan; the read condition on an
8 MiB file; the command line."""
import json
import os
import random
import subprocess

import pytest

import fai_fetch_ref as R
import oracle
import seqgen
import bigseqkit_amd as bsk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")
FORMAT = 3


class Opts:
    def __init__(self, d):
        self.d = dict(d)

    def to_json(self):
        return json.dumps(self.d)


def put(tmp_path, name, data):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def frame(data, fastq):
    import torch
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return bsk.SeqFrame(bsk.FORMAT_FASTQ if fastq else bsk.FORMAT_FASTA, [t])


with bsk.FaidxFetchPlan(b"a\t1\t3\t1\t2\n", Opts({"Regions": ["a"]}), 5, device=-1) as _p:
    T = _p.T
CASES = R.cases(T)


@pytest.fixture(scope="module")
def wants():
    return [oracle.faidx_query(text, fastq, json.dumps(o)) for _, text, fastq, o in CASES]


@pytest.mark.parametrize("k", range(len(CASES)))
def test_fetch_is_the_oracle_and_the_whole_file_run(k, tmp_path, wants):
    name, text, fastq, o = CASES[k]
    fai = oracle.faidx(text, fastq, json.dumps({"FullHead": bool(o.get("FullHead"))}))
    path = put(tmp_path, "x.fa", text)
    info = {}
    got = bsk.FaidxFetch(path, fai, Opts(o), info=info)
    assert got == wants[k], name
    if got:
        assert info["T"] == T and info["bytes_written"] == len(got) and info["bytes_read"] <= len(text) + 16
    else:
        assert info == {}  # (no hit, no batch: nothing was read)
    assert got == bsk.FaidxQuery(frame(text, fastq), Opts(o)), name


def test_our_own_rows_and_small_batches(tmp_path):
    """the rows bsk.Faidx writes, and batches of a few hits each: the same bytes"""
    rng = random.Random(4)
    text = seqgen.random_fasta(rng, 300, 0, 2000, width=60, final_newline=False)
    fai = bsk.Faidx(frame(text, False))
    assert fai == oracle.faidx(text, False)
    path = put(tmp_path, "x.fa", text)
    qs = ["s%d:%d-%d" % (k, rng.randint(1, 50), rng.randint(1, 1900)) for k in rng.sample(range(300), 120)]
    o = {"Regions": qs}
    want = oracle.faidx_query(text, False, json.dumps(o))
    info = {}
    assert bsk.FaidxFetch(path, fai, Opts(o), budget=2 * 85536 + 30000, info=info) == want
    assert info["hits"] == want.count(b">") > 60
    assert bsk.FaidxFetch(path, fai, Opts(o)) == want


def refused(path, fai, o):
    with pytest.raises(bsk.BskError) as e:
        bsk.FaidxFetch(path, fai, Opts(o))
    assert e.value.code == FORMAT and R.MSG in str(e.value), str(e.value)
    return str(e.value)


def test_the_index_must_fit_the_file(tmp_path):
    path = put(tmp_path, "two.fa", R.TWO_WIDTHS)
    assert "index row 1 (a), file offset 23" in refused(path, b"a\t18\t3\t6\t7\n", {"Regions": ["a:16-18"]})
    rng = random.Random(5)
    text = seqgen.random_fasta(rng, 30, 50, 400, width=60)
    other = seqgen.random_fasta(rng, 30, 50, 400, width=60)
    path = put(tmp_path, "x.fa", text)
    fai = oracle.faidx(text, False)
    shifted = b"".join(b"\t".join([f[0], f[1], b"%d" % (int(f[2]) + 1)] + f[3:]) + b"\n" for f in (l.split(b"\t") for l in fai.splitlines()))
    for q in (["s3:2-9"], ["s7"], ["s20:70-61"]):
        assert "index row %d (" % (int(q[0].split(":")[0][1:]) + 1) in refused(path, shifted, {"Regions": q, "Config": {"SeqType": "dna"}})
    wrong = oracle.faidx(other, False)
    o = {"Regions": ["s%d" % k for k in range(30)], "Config": {"SeqType": "dna"}}
    with pytest.raises(bsk.BskError) as e:
        bsk.FaidxFetch(path, wrong, Opts(o))
    assert R.MSG in str(e.value) or "beyond the file" in str(e.value)
    # check 1 alone (the end probe passes): a newline where the index has a base, on a line of the region outside its bases,
    # and in a tile that is not the first; the lowest tile names the offset
    big = (">c\n" + "".join("ACGTTGCA" * 8 + "\n" for _ in range(400)) + ">d\nAC\n").encode()
    fai = oracle.faidx(big, False)
    for at, q in ((3 + 65 * 7 + 50, "c:%d-%d" % (64 * 7 + 2, 64 * 7 + 3)), (3 + 65 * 300 + 9, "c:5-%d" % (64 * 399))):
        bad = bytearray(big)
        bad[at] = 10
        assert "index row 1 (c), file offset %d:" % at in refused(put(tmp_path, "bad.fa", bytes(bad)), fai, {"Regions": [q]})


def test_bytes_outside_the_plan_do_not_matter(tmp_path):
    rng = random.Random(9)
    text = seqgen.random_fasta(rng, 400, 100, 3000, width=60)
    fai = oracle.faidx(text, False)
    o = {"Regions": ["s3:5-900", "s200:100-7", "s399", "s120:61-61"]}
    with bsk.FaidxFetchPlan(fai, Opts(o), len(text), device=-1) as p:
        spans = p.batches[0]["spans"]
    junk = R.junk_outside(text, spans)
    assert junk != text
    want = oracle.faidx_query(text, False, json.dumps(o))
    for name, data in (("x.fa", text), ("junk.fa", junk)):
        assert bsk.FaidxFetch(put(tmp_path, name, data), fai, Opts(o)) == want


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    """an 8 MiB FASTA of 64 records, its rows, and a few regions with their oracle"""
    line = b"ACGTTGCAAC" * 6 + b"\n"
    text = b"".join(b">chr%03d\n" % k + line * 2150 + b"ACG\n" for k in range(64))
    assert len(text) >= 8 << 20
    d = tmp_path_factory.mktemp("genome")
    path = put(d, "g.fa", text)
    L = 2150 * 60 + 3
    regions = ["chr%03d:%d-%d" % (k, b, b + 99) for k, b in ((2, 1), (17, 4090), (30, 61), (45, 100000), (63, L - 99))]
    return path, text, oracle.faidx(text, False), regions


def test_conditions_on_an_8_mib_file(genome):
    path, text, fai, regions = genome
    o = {"Regions": regions}
    rows, _ = R.parse_rows(fai, len(text))
    hs = R.hits(rows, regions, len(text))
    assert len(hs) == 5
    info = {}
    got = bsk.FaidxFetch(path, fai, Opts(o), info=info)
    assert got == R.fetch(text, rows, hs) and got.count(b">") == 5
    assert info["bytes_read"] <= R.read_bound(hs) < len(text) // 50 and info["blocks_inflated"] == 0 and info["spans"] <= 10


def test_command_line(genome, tmp_path):
    path, text, fai, regions = genome
    idx = str(tmp_path / "g.fai")

    def run(args):
        r = subprocess.run([CLI, "faidx", *args], capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        return r.stdout

    today = run([path, *regions, "chr007:300-200", "-o", "-"])
    first = run([path, *regions, "chr007:300-200", "-d", idx, "-o", "-"])       # IDX absent: today's run, and the rows are written
    assert first == today and today.count(b">") == 6 and open(idx, "rb").read() == fai
    with bsk.FaidxFetchPlan(fai, Opts({"Regions": regions + ["chr007:300-200"]}), len(text), device=-1) as p:
        junk = put(tmp_path, "junk.fa", R.junk_outside(text, p.batches[0]["spans"]))
    assert run([junk, *regions, "chr007:300-200", "-d", idx, "-o", "-"]) == today  # IDX present: the file is not loaded
    r = subprocess.run([CLI, "faidx", junk, *regions, "chr007:300-200", "-o", "-"], capture_output=True, timeout=300)
    assert r.stdout != today                                                       # (without -d the junk is what is read)
    # a compressed single file out
    gz = str(tmp_path / "out.fa.gz")
    run([junk, *regions, "-d", idx, "-o", gz, "--merge"])
    import gzip
    assert gzip.decompress(open(gz, "rb").read()) == run([path, *regions, "-o", "-"])
    # -r and -l through the index
    rf = put(tmp_path, "regions.txt", ("\n".join(regions) + "\n").encode())
    assert run([junk, "-l", rf, "-d", idx, "-o", "-"]) == run([path, *regions, "-o", "-"])
    want = run([path, "-r", "^chr00[12]$", "-o", "-"])
    assert run([path, "-r", "^chr00[12]$", "-d", idx, "-o", "-"]) == want and want.count(b">") == 2
    # an index that is not this file's is refused with the row named
    r = subprocess.run([CLI, "faidx", put(tmp_path, "moved.fa", text[1:] + b"\n"), regions[1], "-d", idx, "-o", "-"], capture_output=True, timeout=300)
    assert r.returncode == 1 and r.stdout == b"" and R.MSG in r.stderr.decode() and "index row 18 (chr017)" in r.stderr.decode()


# ---------------------------------------------------------------- BGZF: the fetch through the block table
import struct  # noqa: E402

import bgzf_ref as Z  # noqa: E402


@pytest.mark.parametrize("name", sorted(R.BGZF_QUERIES))
def test_bgzf_fetch_is_the_oracle(name, tmp_path):
    """blocks of 100 and of 65 280 bytes, empty blocks in the middle, no EOF block; regions inside a block and across block
    edges; the table from us and from the Python writer"""
    files, _ = R.bgzf_files()
    text, data = files[name]
    path = put(tmp_path, name + ".fa.gz", data)
    fai = oracle.faidx(text, False)
    ours, theirs = bsk.BgzfGzi(path)[0], R.gzi_write(Z.index(data))
    assert ours == theirs
    table = R.gzi_read(theirs)
    o = {"Regions": R.BGZF_QUERIES[name], "Config": {"SeqType": "dna"}}
    want = oracle.faidx_query(text, False, json.dumps(o))
    assert want.count(b">") == len(o["Regions"])
    hs = R.hits(R.parse_rows(fai, len(text))[0], o["Regions"], len(text))
    for gzi in (ours, theirs):
        info = {}
        assert bsk.FaidxFetch(path, fai, Opts(o), gzi=gzi, info=info) == want
        assert 0 < info["blocks_inflated"] <= R.blocks_bound(table, hs, len(text))


def test_bgzf_wrong_table_entries(tmp_path):
    files, _ = R.bgzf_files()
    text, data = files["b100"]
    path = put(tmp_path, "x.fa.gz", data)
    fai = oracle.faidx(text, False)
    table = R.gzi_read(R.gzi_write(Z.index(data)))
    o = {"Regions": ["s0:1-5"], "Config": {"SeqType": "dna"}}
    want = oracle.faidx_query(text, False, json.dumps(o))
    far = len(table) - 3

    def with_entry(k, c, u):
        t = list(table)
        t[k] = (c, u)
        return struct.pack("<Q", len(t) - 1) + b"".join(struct.pack("<QQ", a, b) for a, b in t[1:])

    assert bsk.FaidxFetch(path, fai, Opts(o), gzi=with_entry(far, table[far][0] + 1, table[far][1])) == want   # not touched: accepted
    with pytest.raises(bsk.BskError) as e:
        bsk.FaidxFetch(path, fai, Opts(o), gzi=with_entry(3, table[3][0], table[3][1] + 1))                    # touched: refused
    assert e.value.code == FORMAT and "block table entry 2 (compressed offset %d, text offset %d)" % table[2] in str(e.value)
    bad = bytearray(data)
    bad[table[1][0] + 20] ^= 0x55   # a damaged block that is touched: the refusal of the BGZF reader
    with pytest.raises(bsk.BskError):
        bsk.FaidxFetch(put(tmp_path, "bad.fa.gz", bytes(bad)), fai, Opts(o), gzi=R.gzi_write(Z.index(data)))


def test_bgzf_conditions_and_command_line(genome, tmp_path):
    """the 8 MiB file as BGZF (blocks of 65 280 bytes): blocks inflated <= the blocks the spans overlap + 1 per probe; then the
    command line, .fa.gz in and .fa.gz out, the block table written where it was absent"""
    path, text, fai, regions = genome
    gz = put(tmp_path, "g.fa.gz", bsk.BgzfDeflate(text, device=0, eof=True))
    image, n_text = bsk.BgzfGzi(gz)
    assert n_text == len(text)
    table = R.gzi_read(image)
    rows, _ = R.parse_rows(fai, len(text))
    hs = R.hits(rows, regions, len(text))
    info = {}
    want = R.fetch(text, rows, hs)
    assert bsk.FaidxFetch(gz, fai, Opts({"Regions": regions}), gzi=image, info=info) == want
    print("blocks inflated", info["blocks_inflated"], "bound", R.blocks_bound(table, hs, len(text), probe_blocks=1), "of", len(table))
    assert info["blocks_inflated"] <= R.blocks_bound(table, hs, len(text), probe_blocks=1) < len(table) // 4
    idx = put(tmp_path, "g.fai", fai)
    out = str(tmp_path / "out.fa.gz")
    r = subprocess.run([CLI, "faidx", gz, *regions, "-d", idx, "-o", out, "--merge"], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    import gzip
    assert gzip.decompress(open(out, "rb").read()) == want
    assert open(gz + ".gzi", "rb").read() == image
    r = subprocess.run([CLI, "faidx", gz, *regions, "-d", idx, "-o", "-"], capture_output=True, timeout=300)  # the table is read now
    assert r.returncode == 0 and r.stdout == want, r.stderr.decode()[-2000:]
