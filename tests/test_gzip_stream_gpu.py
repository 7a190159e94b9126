"""The gzip segment reader on the GPU (PARITY.md GZIP "segments"): the device's reader against zlib, against the piece rule
restated in gzip_stream_ref.model and against the host's reader, on the corpus of gzip_ref and on the small shapes of
test_gzip_stream_cpu.py at the same sizes; its refusals against the host reader's; and the two command-line paths that read a
plain gzip file in pieces -- `stats` on a file that is not read whole and the seven bucket commands, asked for by BSK_GZIP=1
BSK_GZIP_STREAM=1 -- against the same commands on the plain files.  Without the new switch both paths refuse as before
(tests/test_gzip_cpu.py holds those texts whole)."""
import ctypes as C
import gzip
import os
import random
import subprocess

import pytest
import torch

import bgzf_ref as R
import bgzf_stream_ref as BS
import gzip_ref as G
import gzip_stream_ref as S
import bigseqkit_amd as bsk
from bigseqkit_amd._lib import lib, check
from test_gzip_stream_cpu import check_file, put

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")
READER = bsk.GzipReader   # what this file is about


@pytest.mark.parametrize("name", list(G.corpus()))
def test_device_reader_equals_zlib_and_the_rule(tmp_path, name):
    """the pieces joined are the text, the offsets are the model's -- and so the host reader's -- at 4 and 16 chunks a segment and
    at one segment that holds the file; piece(lo, hi) gives the bytes again; a piece stays readable after the next call"""
    data, chunk = G.corpus()[name]
    want = S.expected(data)
    piece, look = S.sizes_of(want)
    check_file(tmp_path, name, data, S.fmt_of(name), piece, look, S.settings(data, chunk), device=0)


def test_device_pieces_equal_host_pieces(tmp_path):
    for name in ("ml1_l6", "three_members", "stored_false"):
        data, chunk = G.corpus()[name]
        piece, look = S.sizes_of(S.expected(data))
        path = put(tmp_path, name, data)
        dev, _ = S.read_all(path, S.fmt_of(name), 0, piece, look, 4 * chunk, chunk)
        host, _ = S.read_all(path, S.fmt_of(name), -1, piece, look, 16 * chunk, chunk, again=False)
        assert dev == host, name


def test_small_shapes_on_the_device(tmp_path):
    """the shapes of test_gzip_stream_cpu.py that aim at the resume points, at the same sizes"""
    data, _ = G.corpus()["far_32768"]
    info, = check_file(tmp_path, "far_32768", data, S.FQ, 1000, 500, [S.SMALL], device=0)
    assert info["segments"] == 1 and info["doublings"] >= 4, info
    data, text = S.far_across_segments()
    infos = check_file(tmp_path, "far_across", data, S.FQ, 5000, 500, [S.SMALL, (4096, 1024)], device=0)
    assert infos[0]["segments"] >= 10 and infos[0]["doublings"] == 0, infos[0]
    for name in ("ml1_l6", "sync_flush"):
        data, _ = G.corpus()[name]
        want = S.expected(data)
        info, = check_file(tmp_path, name, data, S.FQ, len(want) // 3, 1000, [S.SMALL], device=0)
        assert info["segments"] >= 10 and len(want) / info["segments"] < 32768, (name, info)
    for name in ("three_members", "empty_between", "header_fields"):
        data, _ = G.corpus()[name]
        want = S.expected(data)
        ends = S.member_ends(data)
        infos = check_file(tmp_path, name, data, S.FQ, len(want) // 4, 1500, S.member_end_settings(ends), device=0)
        assert all(i["members"] == len(ends) for i in infos), (name, infos)
    good, bad, trailer = S.long_member()
    info, = check_file(tmp_path, "long_good", good, S.FQ, 100_000, 2000, [(8192, 1024)], device=0)
    assert info["segments"] >= 6 and info["members"] == 2


def test_pieces_begin_on_256_bytes_and_stay_valid(tmp_path):
    data, chunk = G.corpus()["ml2_l1"]
    want = S.expected(data)
    model = S.model(want, S.FQ, 30_000, 2000)
    with READER(put(tmp_path, "ml2_l1", data), S.FQ, device=0, piece_text_bytes=30_000, lookahead_bytes=2000, segment_bytes=4 * chunk, chunk_bytes=chunk) as r:
        prev = None
        for k, (t, lo, hi) in enumerate(r):
            assert t.is_cuda and t.dtype == torch.uint8 and (t.numel() == 0 or t.data_ptr() % 256 == 0), k
            assert (lo, hi) == model[k]
            if prev is not None:     # (the piece before this one: not yet overwritten)
                assert bytes(prev[0].cpu().numpy().tobytes()) == want[prev[1]:prev[2]], k
            prev = (t, lo, hi)
        for lo, hi in (model[-2], model[1]):
            t = r.piece(lo, hi)
            assert t.data_ptr() % 256 == 0 and bytes(t.cpu().numpy().tobytes()) == want[lo:hi]


def test_device_reader_refuses_as_the_host_reader(tmp_path):
    """every malformed file, both files with a match that reaches in front of its member, the long member with a wrong CRC, and a
    stream that outgrows the segment's cap: the code and the text of the host reader, whole"""
    bad = {k: (d, 4 * c, c) for k, (d, c, _, _) in G.malformed().items()}
    for k, (d, c) in G.reach_before_member().items():
        first = G.gz(G.fastq(100_000, 31), 6)
        bad[k] = (d, len(first), c)
        bad[k + "_small"] = (d, 2048, c)
    bad["long_bad"] = (S.long_member()[1], 8192, 1024)
    bad["level0_cap"] = (G.corpus()["level0"][0], 2048, 1024)
    for name, (data, segment, chunk) in bad.items():
        path = put(tmp_path, name, data)
        host = S.refusal(path, S.FQ, -1, 100_000, 2000, segment, chunk)
        dev = S.refusal(path, S.FQ, 0, 100_000, 2000, segment, chunk)
        assert host[0] != 0 and dev == host, (name, dev, host)


def test_stages_of_the_reader(tmp_path):
    """bsk_profile_dump carries the reader's stages in the one codec registry: the steps of every segment and the cut"""
    data, chunk = G.corpus()["ml1_l6"]
    path = put(tmp_path, "ml1_l6", data)
    with bsk.Operator("Stats", "{}") as op:
        check(lib.bsk_profile_enable(op.ctx, 1), op.ctx)
        check(lib.bsk_profile_reset(op.ctx), op.ctx)
        got, info = S.read_all(path, S.FQ, 0, 30_000, 2000, 4 * chunk, chunk, again=False)
        buf = C.create_string_buffer(1 << 16)
        check(lib.bsk_profile_dump(op.ctx, buf, len(buf)), op.ctx)
        check(lib.bsk_profile_enable(op.ctx, 0), op.ctx)
    stages = {k: int(v.split("/")[1]) for k, v in (x.split("=") for x in buf.value.decode().split(";") if x)}
    assert info["segments"] >= 4
    for s in ("gzip_find", "gzip_size", "gzip_decode", "gzip_windows", "gzip_translate", "gzip_crc"):
        assert stages.get(s, 0) >= info["segments"], (s, stages, info)
    assert stages.get("gzip_stream_cut", 0) >= len(got) - 1, stages


# ------------------------------------------------------------------ the command line
GZIP = {"BSK_GZIP": "1", "BSK_GZIP_STREAM": "1", "BSK_STREAM_PIECE_BYTES": "20000", "BSK_GZIP_LOOKAHEAD_BYTES": "2000", "BSK_GZIP_SEGMENT_BYTES": "32768",
        "BSK_GZIP_CHUNK_BYTES": "1024"}   # (a file is two or three segments: a wave walks a DEFLATE block in some 10 ms, whatever the segment holds)
BGZF = {"BSK_BGZF_STREAM": "1", "BSK_BGZF_LOOKAHEAD_BYTES": "2000", "BSK_BGZF_CHUNK_BYTES": "30000"}


def cli(args, env=None):
    e = {k: v for k, v in os.environ.items() if not k.startswith(("BSK_GZIP", "BSK_BGZF_STREAM"))}
    e.update(env or {})
    return subprocess.run([CLI, *args], capture_output=True, timeout=300, env=e)


def records(seed, n, fastq, ids=None):
    """n short records with the IDs `ids` (default r0 .. r<n-1>), a third of the sequences repeated"""
    r, out = random.Random(seed), []
    seqs = ["".join(r.choice("ACGT") for _ in range(r.randint(30, 90))) for _ in range(max(1, 2 * n // 3))]
    for k in range(n):
        s = r.choice(seqs)
        name = "r%d" % k if ids is None else ids[k]
        if fastq:
            out.append("@%s d=%d\n%s\n+\n%s\n" % (name, k, s, "".join(chr(r.randint(40, 73)) for _ in s)))
        else:
            out.append(">%s d=%d\n%s\n" % (name, k, s))
    return "".join(out).encode()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """two files per format whose IDs overlap (the second in another order, a few IDs twice, some missing): plain, gzip -- the
    second file in two members -- and BGZF"""
    d = tmp_path_factory.mktemp("gzip_stream")
    out = {"dir": d}
    for fastq, ext in ((True, "fq"), (False, "fa")):
        r = random.Random(31 + fastq)
        n = 1500
        ids1 = ["r%d" % (k if k % 50 else k - 1) for k in range(n)]          # (an ID twice now and then)
        ids2 = [i for i in ids1 if r.random() < 0.8] + ["only2_%d" % k for k in range(100)]
        r.shuffle(ids2)
        a, b = records(41 + fastq, n, fastq, ids1), records(43 + fastq, len(ids2), fastq, ids2)
        for name, text in (("a", a), ("b", b)):
            plain, z, bz = d / ("%s.%s" % (name, ext)), d / ("%s.%s.gz" % (name, ext)), d / ("%s.bgzf.%s.gz" % (name, ext))
            plain.write_bytes(text)
            half = text.index(b"\n@" if fastq else b"\n>", len(text) // 2) + 1
            z.write_bytes(G.gz(text, 6) if name == "a" else G.gz(text[:half], 9) + G.gz(text[half:], 1))
            bz.write_bytes(BS.write_mixed(text, 51, 400, 1500) + R.EOF_BLOCK)
            assert gzip.decompress(z.read_bytes()) == text and bsk.BgzfProbe(z.read_bytes()) == 2
            out[name + "." + ext] = (str(plain), str(z), text, str(bz))
    return out


@pytest.mark.parametrize("name", ["a.fq", "b.fa"])
def test_cli_stats_streams_a_gzip_file(inputs, name):
    """BSK_HOST_PIPELINE_FROM=0: every file is "too large to load whole"; with both switches the table of the gzip file is the
    plain file's.  (Without BSK_GZIP_STREAM this run is refused: tests/test_gzip_cpu.py.)"""
    plain, z, _, _ = inputs[name]
    env = {"BSK_GZIP": "1", "BSK_GZIP_STREAM": "1", "BSK_HOST_PIPELINE_FROM": "0", "BSK_STREAM_PIECE_BYTES": "3000", "BSK_GZIP_SEGMENT_BYTES": "4096",
           "BSK_GZIP_CHUNK_BYTES": "1024"}
    a, b, c = cli(["stats", "-a", plain]), cli(["stats", "-a", z], env), cli(["stats", "-a", "-T", z], env)
    assert a.returncode == 0 and b.returncode == 0 and c.returncode == 0, (a.stderr, b.stderr, c.stderr)
    strip = lambda p, path: b" ".join(p.stdout.replace(path.encode(), b"F").split())   # (the file column differs by the name, and so its width)
    assert strip(a, plain) == strip(b, z) and a.stdout, (a.stdout, b.stdout)
    assert c.stdout == cli(["stats", "-a", "-T", plain]).stdout.replace(plain.encode(), z.encode())
    r = cli(["stats", "-a", z], {k: v for k, v in env.items() if k != "BSK_GZIP_STREAM"})
    assert r.returncode == 1 and b"virtual offsets" in r.stderr, r.stderr


BUCKETS = {
    # command -> (arguments in front of the files, files, the budget: bytes of record text or of subjects)
    "shuffle": (["shuffle", "-s", "24"], ("a.fq",), 30000),
    "sort": (["sort"], ("a.fa", "b.fa"), 40000),
    "rmdup": (["rmdup", "-s"], ("a.fq",), 15000),
    "rename": (["rename"], ("a.fq",), 2000),
    "common": (["common"], ("a.fa", "b.fa"), 2000),
    "concat": (["concat", "-f"], ("a.fq", "b.fq"), 12000),
}


def buckets_of(p, use):
    return int(p.stderr.decode().split("%s in " % use)[1].split(" bucket")[0])


@pytest.mark.parametrize("use", list(BUCKETS))
def test_cli_buckets_on_gzip_inputs(inputs, use):
    """three or more buckets: the output on gzip inputs is byte for byte the output on the same inputs plain"""
    args, names, budget = BUCKETS[use]
    env = dict(GZIP, BSK_CLI_TIMING="1", **{"BSK_%s_BUDGET_BYTES" % use.upper(): str(budget)})
    d = inputs["dir"]
    outs = []
    for col in (0, 1):
        out = str(d / ("%s_%d.out" % (use, col)))
        p = cli([*args, *[inputs[n][col] for n in names], "-o", out, "--merge"], env)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert buckets_of(p, use) >= 3, p.stderr.decode()[-2000:]
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1] and outs[0]


def test_cli_pair_on_plain_gzip_and_bgzf_files(inputs):
    """pair in buckets: both plain, file 1 plain and file 2 gzip, file 1 BGZF and file 2 gzip: the four files of the plain pair"""
    d = inputs["dir"]
    env = dict(GZIP, **BGZF, BSK_CLI_TIMING="1", BSK_PAIR_BUDGET_BYTES="5000")
    got = []
    for k, cols in enumerate(((0, 0), (0, 1), (3, 1))):
        out = d / ("pair_%d" % k)
        p = cli(["pair", "-u", inputs["a.fq"][cols[0]], inputs["b.fq"][cols[1]], "-O", str(out)], env)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert buckets_of(p, "pair") >= 3, p.stderr.decode()[-2000:]
        got.append(tuple((out / n).read_bytes() for n in ("paired.1", "paired.2", "unpaired.1", "unpaired.2")))
    assert got[0] == got[1] == got[2] and all(got[0])


def test_cli_buckets_write_bgzf(inputs):
    """a .gz output name: gzip in, BGZF out, the text of the plain run"""
    d = inputs["dir"]
    env = dict(GZIP, BSK_CLI_TIMING="1", BSK_SORT_BUDGET_BYTES="40000")
    plain, z = str(d / "sorted.fq"), str(d / "sorted.fq.gz")
    a = cli(["sort", "-r", inputs["a.fq"][0], "-o", plain, "--merge"], env)
    b = cli(["sort", "-r", inputs["a.fq"][1], "-o", z, "--merge"], env)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert buckets_of(b, "sort") >= 3
    packed = open(z, "rb").read()
    assert bsk.BgzfProbe(packed) == 1 and packed.endswith(R.EOF_BLOCK) and gzip.decompress(packed) == open(plain, "rb").read()


def test_cli_refuses_a_corrupt_member_before_any_output(inputs):
    """the listing pass reads the whole file: a wrong CRC in the second member of file 2 ends the run with no output file"""
    d = inputs["dir"]
    data = open(inputs["b.fq"][1], "rb").read()
    bad = str(d / "bad.fq.gz")
    open(bad, "wb").write(data[:-8] + bytes([data[-8] ^ 1]) + data[-7:])
    out = str(d / "never.out")
    p = cli(["concat", "-f", inputs["a.fq"][1], bad, "-o", out, "--merge"], dict(GZIP, BSK_CONCAT_BUDGET_BYTES="12000"))
    assert p.returncode == 1 and b"member 1 at offset %d: CRC mismatch" % (len(data) - 8) in p.stderr and not os.path.exists(out), p.stderr
