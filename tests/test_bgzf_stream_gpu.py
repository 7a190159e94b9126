"""The piece reader of a BGZF file on the GPU (PARITY.md BGZF "pieces"): the device's reader against zlib, against the rule
restated in bgzf_stream_ref.model and against the host's reader on the cases whose coverage test_bgzf_stream_cpu.py asserts;
k_bgzf_stream_cut against bsk_find_record_start; the refusals; and the two command-line paths that stream a BGZF file --
`stats` on a file of any size and the seven bucket commands, asked for by BSK_BGZF_STREAM=1 -- against the same commands on the
plain files.  Without the switch both paths refuse a BGZF file as before (tests/test_bgzf_gpu.py holds that)."""
import ctypes as C
import gzip
import os
import random
import subprocess

import pytest
import torch

import bgzf_ref as R
import bgzf_stream_ref as S
import bigseqkit_amd as bsk
from bigseqkit_amd._lib import lib, check

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")
READER = bsk.BgzfReader   # what this file is about


@pytest.fixture(scope="module")
def cases():
    return S.cases()


@pytest.mark.parametrize("name", list(S.cases()))
def test_device_reader_equals_zlib_and_the_rule(tmp_path, cases, name):
    """the pieces joined are the text, every boundary is a record start, the offsets are the model's -- and so the host
    reader's -- at every chunk size, and piece(lo, hi) gives the bytes again"""
    S.check_case(tmp_path, name, cases[name], 0)


def test_device_pieces_equal_host_pieces(tmp_path, cases):
    for name in ("fq_mixed", "fa_long_record", "fq_wrapped"):
        data, fmt, piece, look = cases[name]
        path = tmp_path / (name + ".gz")
        path.write_bytes(data)
        assert S.read_all(path, fmt, 0, piece, look, 1000) == S.read_all(path, fmt, -1, piece, look, 4097), name


def test_pieces_begin_on_256_bytes_and_stay_valid(tmp_path, cases):
    """the pointer of every piece is a multiple of 256, also behind a seek into a block; a piece is intact after the next call"""
    data, fmt, piece, look = cases["fa_mixed"]
    want, text = S.model(data, fmt, piece, look)
    path = tmp_path / "fa.gz"
    path.write_bytes(data)
    with READER(path, fmt, device=0, piece_text_bytes=piece, lookahead_bytes=look, comp_chunk_bytes=900) as r:
        prev = None
        for k, (t, lo, hi) in enumerate(r):
            assert t.is_cuda and t.dtype == torch.uint8 and (t.numel() == 0 or t.data_ptr() % 256 == 0), k
            if prev is not None:     # (the piece before this one: not yet overwritten)
                assert bytes(prev[0].cpu().numpy().tobytes()) == text[prev[1]:prev[2]], k
            prev = (t, want[k][0], want[k][1])
        inside = [w for w in want[1:] if w[2] & 0xffff]
        assert inside
        for w in (inside[-1], inside[0]):
            r.seek(w[2])
            t, lo, hi = next(r)
            assert (lo, hi) == (w[2], w[3]) and t.data_ptr() % 256 == 0 and bytes(t.cpu().numpy().tobytes()) == text[w[0]:w[1]]
            t = r.piece(w[2], w[3])
            assert t.data_ptr() % 256 == 0 and bytes(t.cpu().numpy().tobytes()) == text[w[0]:w[1]]


def test_cut_kernel_agrees_or_declines():
    """k_bgzf_stream_cut over fuzzed FASTA and four-line FASTQ windows (and wrapped and damaged ones): its answer is
    bsk_find_record_start's or "declined", never another offset; it is the host function's answer; and on plain text it does
    answer"""
    answered = {S.FA: 0, S.FQ: 0}
    for window, frm, fmt in S.fuzz_windows(9, 400):
        got = S.stream_cut(window, frm, fmt, 0)
        assert got == S.stream_cut(window, frm, fmt, -1), (window, frm, fmt)
        if got != S.DECLINED:
            assert got == S.find_record_start(window, frm, fmt), (window, frm, fmt, got)
            answered[fmt] += 1
    assert answered[S.FA] >= 60 and answered[S.FQ] >= 80, answered


def test_device_reader_refuses_malformed(tmp_path):
    """a bad CRC, a truncated last block and a block of type 3 in the SECOND chunk: the block is numbered over the whole file and
    named with its file offset; plain gzip names bgzip"""
    for name, (data, chunk, code, block, off, word) in S.malformed_in_second_chunk().items():
        path = tmp_path / (name + ".gz")
        path.write_bytes(data)
        with pytest.raises(bsk.BskError) as e:
            with READER(path, S.FQ, device=0, piece_text_bytes=1500, lookahead_bytes=600, comp_chunk_bytes=chunk) as r:
                list(r)
        assert e.value.code == code and word in str(e.value), (name, str(e.value))
        if block is not None:
            assert ("block %d at offset %d:" % (block, off)) in str(e.value), (name, str(e.value))
    M, good, text = R.malformed()
    for name, (data, code, block, word) in M.items():
        path = tmp_path / (name + ".gz")
        path.write_bytes(data)
        with pytest.raises(bsk.BskError) as e:
            with READER(path, S.FQ, device=0, piece_text_bytes=1500, lookahead_bytes=600, comp_chunk_bytes=3000) as r:
                list(r)
        assert e.value.code == code and word in str(e.value), (name, str(e.value))
        if block is not None:
            assert ("block %d at offset" % block) in str(e.value), (name, str(e.value))


def test_stages_of_the_reader(tmp_path, cases):
    """bsk_profile_dump names the reader's stages: the inflate launches and the cut"""
    data, fmt, piece, look = cases["fq_mixed"]
    path = tmp_path / "fq.gz"
    path.write_bytes(data)
    with bsk.Operator("Stats", "{}") as op:
        check(lib.bsk_profile_enable(op.ctx, 1), op.ctx)
        check(lib.bsk_profile_reset(op.ctx), op.ctx)
        n = len(S.read_all(path, fmt, 0, piece, look, 1000))
        buf = C.create_string_buffer(1 << 16)
        check(lib.bsk_profile_dump(op.ctx, buf, len(buf)), op.ctx)
        check(lib.bsk_profile_enable(op.ctx, 0), op.ctx)
    stages = dict(x.split("=") for x in buf.value.decode().split(";") if x)
    assert int(stages["bgzf_stream_cut"].split("/")[1]) >= n - 1 and int(stages["bgzf_inflate"].split("/")[1]) >= n, stages


CODEC_STAGES = ("bgzf_find", "bgzf_sizes", "bgzf_inflate", "bgzf_deflate", "bgzf_pack",
                "gzip_find", "gzip_size", "gzip_decode", "gzip_windows", "gzip_translate", "gzip_crc")


def test_one_registry_holds_the_stages_of_every_codec(monkeypatch):
    """BGZF input, BGZF output and plain gzip feed one process-wide registry: with profiling on, one call of each leaves every
    one of their stages in bsk_profile_dump with at least one launch; a reset empties it; with profiling off nothing is added"""
    text, fq = R.fastq_text(2048)[:2048], R.fastq_text(20000)
    z_bgzf = R.write(text, block=1024)                     # two blocks of 1 KB of text, and the EOF block
    z_gzip = gzip.compress(fq, mtime=0)
    monkeypatch.setenv("BSK_GZIP_CHUNK_BYTES", "4096")     # (more than one chunk)
    assert len(R.index(z_bgzf)) == 3 and len(z_gzip) > 4096

    def one_of_each():
        assert bytes(bsk.BgzfInflate(z_bgzf).cpu().numpy().tobytes()) == text
        assert gzip.decompress(bsk.BgzfDeflate(text, block_bytes=1024)) == text
        assert bytes(bsk.GzipInflate(z_gzip).cpu().numpy().tobytes()) == fq

    def dump(op):
        buf = C.create_string_buffer(1 << 16)
        check(lib.bsk_profile_dump(op.ctx, buf, len(buf)), op.ctx)
        return {k: int(v.split("/")[1]) for k, v in (x.split("=") for x in buf.value.decode().split(";") if x)}

    with bsk.Operator("Stats", "{}") as op:
        check(lib.bsk_profile_enable(op.ctx, 1), op.ctx)
        check(lib.bsk_profile_reset(op.ctx), op.ctx)
        one_of_each()
        stages = dump(op)
        assert all(stages.get(s, 0) >= 1 for s in CODEC_STAGES), stages
        check(lib.bsk_profile_reset(op.ctx), op.ctx)
        assert not set(dump(op)) & set(CODEC_STAGES)
        check(lib.bsk_profile_enable(op.ctx, 0), op.ctx)
        one_of_each()
        assert not set(dump(op)) & set(CODEC_STAGES)


# ------------------------------------------------------------------ the command line
STREAM ={"BSK_BGZF_STREAM": "1", "BSK_STREAM_PIECE_BYTES": "20000", "BSK_BGZF_LOOKAHEAD_BYTES": "2000", "BSK_BGZF_CHUNK_BYTES": "30000"}


def cli(args, env=None):
    e = dict(os.environ)
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
    """two files per format whose IDs overlap (the second in another order, a few IDs twice, some missing), plain and BGZF"""
    d = tmp_path_factory.mktemp("bgzf_stream")
    out = {"dir": d}
    for fastq, ext in ((True, "fq"), (False, "fa")):
        r = random.Random(31 + fastq)
        n = 1500
        ids1 = ["r%d" % (k if k % 50 else k - 1) for k in range(n)]          # (an ID twice now and then)
        ids2 = [i for i in ids1 if r.random() < 0.8] + ["only2_%d" % k for k in range(100)]
        r.shuffle(ids2)
        a, b = records(41 + fastq, n, fastq, ids1), records(43 + fastq, len(ids2), fastq, ids2)
        for name, text in (("a", a), ("b", b)):
            plain, z = d / ("%s.%s" % (name, ext)), d / ("%s.%s.gz" % (name, ext))
            plain.write_bytes(text)
            z.write_bytes(S.write_mixed(text, 51, 400, 1500) + R.EOF_BLOCK)
            out[name + "." + ext] = (str(plain), str(z), text)
    return out


@pytest.mark.parametrize("name", ["a.fq", "a.fa"])
def test_cli_stats_streams_a_bgzf_file(inputs, name):
    """BSK_HOST_PIPELINE_FROM=0: every file is "too large to load whole"; with BSK_BGZF_STREAM=1 the table of the BGZF file is
    the plain file's"""
    plain, z, _ = inputs[name]
    env = dict(STREAM, BSK_HOST_PIPELINE_FROM="0", BSK_STREAM_PIECE_BYTES="3000")
    a, b, c = cli(["stats", "-a", plain]), cli(["stats", "-a", z], env), cli(["stats", "-a", "-T", z], env)
    assert a.returncode == 0 and b.returncode == 0 and c.returncode == 0, (a.stderr, b.stderr, c.stderr)
    strip = lambda p, path: b" ".join(p.stdout.replace(path.encode(), b"F").split())   # (the file column differs by the name, and so its width)
    assert strip(a, plain) == strip(b, z) and a.stdout, (a.stdout, b.stdout)
    assert c.stdout == cli(["stats", "-a", "-T", plain]).stdout.replace(plain.encode(), z.encode())


BUCKETS = {
    # command -> (arguments in front of the files, files, the budget: bytes of record text or of subjects)
    "shuffle": (["shuffle", "-s", "24"], ("a.fq",), 30000),
    "sort": (["sort"], ("a.fa", "b.fa"), 40000),
    "rmdup": (["rmdup", "-s"], ("a.fq",), 15000),
    "rename": (["rename"], ("a.fq",), 2000),
    "common": (["common"], ("a.fa", "b.fa"), 2000),
    "concat": (["concat", "-f"], ("a.fq", "b.fq"), 4000),
}


def buckets_of(p, use):
    return int(p.stderr.decode().split("%s in " % use)[1].split(" bucket")[0])


@pytest.mark.parametrize("use", list(BUCKETS))
def test_cli_buckets_on_bgzf_inputs(inputs, use):
    """three or more buckets: the output on BGZF inputs is byte for byte the output on the same inputs plain"""
    args, names, budget = BUCKETS[use]
    env = dict(STREAM, BSK_CLI_TIMING="1", **{"BSK_%s_BUDGET_BYTES" % use.upper(): str(budget)})
    d = inputs["dir"]
    outs = []
    for col in (0, 1):
        out = str(d / ("%s_%d.out" % (use, col)))
        p = cli([*args, *[inputs[n][col] for n in names], "-o", out, "--merge"], env)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert buckets_of(p, use) >= 3, p.stderr.decode()[-2000:]
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1] and outs[0]


def test_cli_pair_on_a_plain_and_a_bgzf_file(inputs):
    """pair in buckets, file 1 plain and file 2 BGZF, and both BGZF: the four files of the plain pair"""
    d = inputs["dir"]
    env = dict(STREAM, BSK_CLI_TIMING="1", BSK_PAIR_BUDGET_BYTES="5000")
    got = []
    for k, cols in enumerate(((0, 0), (0, 1), (1, 1))):
        out = d / ("pair_%d" % k)
        p = cli(["pair", "-u", inputs["a.fq"][cols[0]], inputs["b.fq"][cols[1]], "-O", str(out)], env)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert buckets_of(p, "pair") >= 3, p.stderr.decode()[-2000:]
        got.append(tuple((out / n).read_bytes() for n in ("paired.1", "paired.2", "unpaired.1", "unpaired.2")))
    assert got[0] == got[1] == got[2] and all(got[0])


def test_cli_buckets_write_bgzf(inputs):
    """a .gz output name: BGZF in, BGZF out, the text of the plain run"""
    d = inputs["dir"]
    env = dict(STREAM, BSK_CLI_TIMING="1", BSK_SORT_BUDGET_BYTES="40000")
    plain, z = str(d / "sorted.fq"), str(d / "sorted.fq.gz")
    a = cli(["sort", "-r", inputs["a.fq"][0], "-o", plain, "--merge"], env)
    b = cli(["sort", "-r", inputs["a.fq"][1], "-o", z, "--merge"], env)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert buckets_of(b, "sort") >= 3
    packed = open(z, "rb").read()
    assert bsk.BgzfProbe(packed) == 1 and packed.endswith(R.EOF_BLOCK) and gzip.decompress(packed) == open(plain, "rb").read()


def test_cli_without_the_switch_refuses_as_before(inputs):
    """the paths that read a BGZF file in pieces are asked for by BSK_BGZF_STREAM=1: without it both refuse as they did, and the
    message names the switch"""
    from test_gzip_cpu import BY_BYTES, UNSET_BUDGET
    z = inputs["a.fq"][1]
    said = lambda r, where, instead: r.returncode == 1 and r.stderr.decode() == "Error: " + z + BY_BYTES % (where, instead) + "\n"
    cut_it = "decompress it first (bgzip -d), or cut it into files that fit, or set BSK_BGZF_STREAM=1 to read it in record-aligned pieces, inflated once per pass"
    r = cli(["stats", z], {"BSK_HOST_PIPELINE_FROM": "0"})
    assert said(r, "'stats' streams a file that does not fit one GPU", cut_it), r.stderr
    r = cli(["sort", z, "-o", "-"], {"BSK_SORT_BUDGET_BYTES": "40000"})
    assert said(r, "the buckets of 'sort' read", UNSET_BUDGET) and b"BSK_BGZF_STREAM=1" in r.stderr, r.stderr
    r = cli(["stats", z], {"BSK_HOST_PIPELINE_FROM": "0", "BSK_BGZF_STREAM": "0"})
    assert said(r, "'stats' streams a file that does not fit one GPU", cut_it), r.stderr


def test_cli_devices_still_refused(inputs):
    """--devices with a BGZF file: refused as before, before a device is touched"""
    from test_gzip_cpu import BY_BYTES, ONE_DEVICE
    z = inputs["a.fq"][1]
    r = cli(["stats", "--devices", "0", z], {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1", "BSK_BGZF_STREAM": "1"})
    assert r.returncode == 1 and r.stderr.decode() == "Error: " + z + BY_BYTES % ("--devices cuts", ONE_DEVICE) + "\n", r.stderr
    assert b"--devices cuts a file by its bytes, which a compressed file does not allow yet" in r.stderr
    assert b"--device N" in r.stderr and b"no HIP device" not in r.stderr
