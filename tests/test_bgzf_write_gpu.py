"""BGZF output on the device (PARITY.md BGZFW): k_bgzf_deflate writes the bytes the host encoder writes -- which zlib judged in
test_bgzf_write_cpu.py -- on every text of the corpus, over more blocks than waves are resident, and in pieces; a result of a
run leaves compressed (bsk_out_to_host_bgzf), as one block and as slices; the store writes BGZF in both its modes; and the
command line compresses whatever it writes under a name that ends in .gz."""
import ctypes as C
import gzip
import json
import os
import re
import subprocess

import pytest

import bgzf_ref as R
import bgzf_write_corpus as W
import bigseqkit_amd as bsk
from bigseqkit_amd import _lib
from bigseqkit_amd._lib import lib, check

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")
DEFLATE = bsk.BgzfDeflate   # what this file is about


def test_device_writes_the_host_bytes():
    for name, (text, _) in W.build().items():
        want = bsk.BgzfDeflateHost(text)
        assert DEFLATE(text) == want, name
        assert DEFLATE(text, eof=False) == want[:-28], name
    assert DEFLATE(b"") == R.EOF_BLOCK and DEFLATE(b"", eof=False) == b""


def test_more_blocks_than_waves_and_pieces():
    """97 bytes a block: over 5 000 blocks, more than the waves of one launch (the grid stride, the scan and the pack); and pieces
    without EOF with one EOF block behind them are the file"""
    import torch
    text = W.fastq_500k()
    out = DEFLATE(text, block_bytes=97)
    assert out == bsk.BgzfDeflateHost(text, 97)
    W.check_file(out, text, 97, True)
    assert len(R.index(out)) - 1 > 5000
    t = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    whole = DEFLATE(t)
    assert whole == bsk.BgzfDeflateHost(text) and gzip.decompress(whole) == text
    cut = 3 * W.BT
    assert DEFLATE(t[:cut], eof=False) + DEFLATE(t[cut:], eof=False) + DEFLATE(b"") == whole
    assert DEFLATE(t[1:cut + 1], eof=False) == bsk.BgzfDeflateHost(text[1:cut + 1], 0, False)    # (a text at an odd address)
    back = bsk.BgzfInflate(whole)                                                              # through k_bgzf_inflate
    assert bytes(back.cpu().numpy().tobytes()) == text


RUN = {"Sort": lib.bsk_sort_run, "SeqTransform": lib.bsk_seq_run, "Grep": lib.bsk_grep_run}


@pytest.mark.parametrize("name,opts,mode", [("Sort", {}, "contiguous"), ("SeqTransform", {"MinLen": 100}, "slices"),
                                            ("Grep", {"Pattern": ["lane=3"], "ByName": True, "UseRegexp": True}, "slices")])
def test_result_to_host_compressed(name, opts, mode):
    import torch
    text = R.fastq_text(300000, 5)
    t = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    op = bsk.Operator(name, json.dumps(opts), 0)
    check(lib.bsk_ctx_set(op.ctx, b"out", mode.encode()), op.ctx)
    out = _lib.Out()
    check(RUN[name](op.ctx, C.c_void_p(t.data_ptr()), t.numel(), 1, bsk.FORMAT_FASTQ, 0, None, C.byref(out)), op.ctx)
    assert (out.n_segments > 0) == (mode == "slices") and out.len > 0
    plain = C.create_string_buffer(out.len)
    check(lib.bsk_out_to_host(op.ctx, C.byref(out), plain, out.len), op.ctx)
    cap = lib.bsk_bgzf_deflate_bound(out.len, 0)
    buf, n = C.create_string_buffer(cap), C.c_size_t()
    for eof in (1, 0):
        check(lib.bsk_out_to_host_bgzf(op.ctx, C.byref(out), eof, buf, cap, C.byref(n)), op.ctx)
        comp = buf.raw[:n.value]
        W.check_file(comp, plain.raw, W.BT, bool(eof))
        assert comp == bsk.BgzfDeflateHost(plain.raw, 0, bool(eof))
    assert lib.bsk_out_to_host_bgzf(op.ctx, C.byref(out), 1, buf, 100, C.byref(n)) == 7   # BSK_ERR_CAPACITY
    op.close()


@pytest.fixture
def small_pieces():
    """the 64 MiB piece of the result copy and of the store brought down to its unit, 1 044 480 bytes (16 blocks, 255 tiles of the
    gather), so that a result of a few MB crosses several piece boundaries"""
    os.environ["BSK_BGZF_PIECE_BYTES"] = "1000000"   # (rounded up to the unit)
    yield 1044480
    del os.environ["BSK_BGZF_PIECE_BYTES"]


@pytest.mark.parametrize("mode", ["slices", "contiguous"])
def test_result_of_several_pieces(mode, small_pieces, tmp_path):
    """a result that is gathered and compressed in several pieces, to the host and through the store: every piece boundary is a
    block boundary (all blocks but the last hold 65 280 bytes) and the file is the host encoder's"""
    import torch
    text = W.fastq_500k() * 7   # (3.5 MB; the repeat lies beyond every block)
    t = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    op = bsk.Operator("Grep", json.dumps({"Pattern": ["lane=3"], "ByName": True, "UseRegexp": True, "InvertMatch": True}), 0)
    check(lib.bsk_ctx_set(op.ctx, b"out", mode.encode()), op.ctx)
    out = _lib.Out()
    check(lib.bsk_grep_run(op.ctx, C.c_void_p(t.data_ptr()), t.numel(), 1, bsk.FORMAT_FASTQ, 0, None, C.byref(out)), op.ctx)
    assert (out.n_segments > 0) == (mode == "slices") and out.len > 2 * small_pieces + 1000      # three pieces at the least
    plain = C.create_string_buffer(out.len)
    check(lib.bsk_out_to_host(op.ctx, C.byref(out), plain, out.len), op.ctx)
    want = bsk.BgzfDeflateHost(plain.raw)
    cap = lib.bsk_bgzf_deflate_bound(out.len, 0)
    buf, n = C.create_string_buffer(cap), C.c_size_t()
    check(lib.bsk_out_to_host_bgzf(op.ctx, C.byref(out), 1, buf, cap, C.byref(n)), op.ctx)
    assert buf.raw[:n.value] == want
    W.check_file(want, plain.raw, W.BT, True)
    st = C.c_void_p()
    path = str(tmp_path / "o.gz")
    check(lib.bsk_store_open(path.encode(), 1, C.byref(st)))
    check(lib.bsk_store_set_bgzf(st, 1))
    check(lib.bsk_store_put(st, op.ctx, 0, C.byref(out)), op.ctx)
    check(lib.bsk_store_close(st, None))
    assert open(path, "rb").read() == want
    op.close()


def test_store_piece_mode_has_no_eof(tmp_path):
    """bsk_store_set_bgzf(s, 2): the file is a piece of a larger one and ends without the EOF block"""
    text = R.fasta_text(70000, 8)
    st = C.c_void_p()
    path = str(tmp_path / "piece.gz")
    check(lib.bsk_store_open(path.encode(), 1, C.byref(st)))
    check(lib.bsk_store_set_bgzf(st, 2))
    check(lib.bsk_store_put_host(st, 0, text, len(text)))
    check(lib.bsk_store_close(st, None))
    data = open(path, "rb").read()
    assert data == bsk.BgzfDeflateHost(text, 0, False) and gzip.decompress(data + R.EOF_BLOCK) == text


@pytest.mark.parametrize("merge", [1, 0])
def test_store_writes_bgzf(merge, tmp_path):
    """two parts put in the order 1, 0 -- one from the device, one from the host: one file with one EOF block, or two files
    part0000N.gz with one each"""
    import torch
    text = R.fastq_text(200000, 6)
    t = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    op = bsk.Operator("SeqTransform", "{}", 0)
    out = _lib.Out()
    check(lib.bsk_seq_run(op.ctx, C.c_void_p(t.data_ptr()), t.numel(), 1, bsk.FORMAT_FASTQ, 0, None, C.byref(out)), op.ctx)
    part1 = C.create_string_buffer(out.len)
    check(lib.bsk_out_to_host(op.ctx, C.byref(out), part1, out.len), op.ctx)
    part0 = R.fasta_text(70000, 8)
    path = str(tmp_path / ("o.gz" if merge else "dir"))
    st = C.c_void_p()
    check(lib.bsk_store_open(path.encode(), merge, C.byref(st)))
    check(lib.bsk_store_set_bgzf(st, 1))
    check(lib.bsk_store_put(st, op.ctx, 1, C.byref(out)), op.ctx)
    assert lib.bsk_store_set_bgzf(st, 0) != 0                       # (not after a put)
    check(lib.bsk_store_put_host(st, 0, part0, len(part0)))
    tot = C.c_uint64()
    check(lib.bsk_store_close(st, C.byref(tot)))
    if merge:
        data = open(path, "rb").read()
        assert tot.value == len(data) and gzip.decompress(data) == part0 + part1.raw
        assert data == bsk.BgzfDeflateHost(part0, 0, False) + bsk.BgzfDeflateHost(part1.raw, 0, True)
        assert [k for k, (off, bsize, isize, xlen) in enumerate(R.index(data)) if isize == 0] == [len(R.index(data)) - 1]   # one EOF block
    else:
        assert sorted(os.listdir(path)) == ["part00000.gz", "part00001.gz"]
        for name, want in (("part00000.gz", part0), ("part00001.gz", part1.raw)):
            data = open(os.path.join(path, name), "rb").read()
            W.check_file(data, want, W.BT, True)
    op.close()
    # and with the switch off nothing about the store changes, names included
    st = C.c_void_p()
    path = str(tmp_path / ("p.gz" if merge else "pdir"))
    check(lib.bsk_store_open(path.encode(), merge, C.byref(st)))
    check(lib.bsk_store_set_bgzf(st, 0))
    check(lib.bsk_store_put_host(st, 0, part0, len(part0)))
    check(lib.bsk_store_close(st, None))
    assert open(path if merge else os.path.join(path, "part00000"), "rb").read() == part0


# ---- the command line: an -o name that ends in .gz is BGZF, any other name is what it was
def cli(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([CLI, *args], capture_output=True, timeout=300, env=e)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzfw")
    fq, fa = d / "x.fq", d / "x.fa"
    fq.write_bytes(R.fastq_text(300000, 5))
    fa.write_bytes(R.fasta_text(200000, 6))
    return d, str(fq), str(fa)


def stats_of(path):
    r = cli(["stats", "-a", "-T", path])
    assert r.returncode == 0 and r.stdout, r.stderr
    return r.stdout.replace(path.encode(), b"F")


CASES = [(["seq"], "x.fq"), (["grep", "-s", "-p", "ACGTAC"], "x.fq"), (["rmdup", "-s"], "x.fq"), (["sort"], "x.fq"), (["seq"], "x.fa"),
         (["sort"], "x.fa")]


@pytest.mark.parametrize("args,name", CASES, ids=["%s-%s" % (a[0], n) for a, n in CASES])
def test_command_line_one_file(inputs, args, name):
    """-o out.gz --merge: gzip reads the file, it holds what the plain -o holds, and read back as input it gives the same table"""
    d, fq, fa = inputs
    src = fq if name.endswith(".fq") else fa
    plain, packed = str(d / ("plain-%s-%s" % (args[0], name))), str(d / ("packed-%s-%s.gz" % (args[0], name)))
    a, b = cli(args + [src, "-o", plain, "--merge"]), cli(args + [src, "-o", packed, "--merge"])
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    want, data = open(plain, "rb").read(), open(packed, "rb").read()
    assert want and gzip.decompress(data) == want
    W.check_file(data, want, W.BT, True)
    assert bsk.BgzfProbe(data) == 1 and stats_of(packed) == stats_of(plain)   # the round trip through k_bgzf_inflate


def test_command_line_part_directory(inputs):
    """several part files: cut at record starts as ever, each a BGZF file of its own, part0000N.gz"""
    d, fq, _ = inputs
    a = cli(["seq", fq, "-o", str(d / "parts"), "--partitions", "3"])
    b = cli(["seq", fq, "-o", str(d / "parts.gz"), "--partitions", "3"])
    c = cli(["seq", fq, "-o", str(d / "one.gz")])
    assert a.returncode == 0 and b.returncode == 0 and c.returncode == 0, (a.stderr, b.stderr, c.stderr)
    assert sorted(os.listdir(d / "parts")) == ["part00000", "part00001", "part00002"]
    assert sorted(os.listdir(d / "parts.gz")) == ["part00000.gz", "part00001.gz", "part00002.gz"]
    for k in range(3):
        want = (d / "parts" / ("part%05d" % k)).read_bytes()
        W.check_file((d / "parts.gz" / ("part%05d.gz" % k)).read_bytes(), want, W.BT, True)
    assert os.listdir(d / "one.gz") == ["part00000.gz"]
    assert gzip.decompress((d / "one.gz" / "part00000.gz").read_bytes()) == open(fq, "rb").read()


def test_command_line_buckets_and_pieces(inputs):
    """sort in three buckets over several pieces: every share leaves the device compressed, one EOF block ends the file"""
    d, fq, _ = inputs
    env = {"BSK_SORT_BUDGET_BYTES": "120000", "BSK_STREAM_PIECE_BYTES": "70000", "BSK_CLI_TIMING": "1"}
    plain, packed = str(d / "b.fq"), str(d / "b.fq.gz")
    a, b = cli(["sort", fq, "-o", plain, "--merge"], env), cli(["sort", fq, "-o", packed, "--merge"], env)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    m = re.search(rb"in (\d+) bucket\(s\) of at most \d+ bytes, (\d+) piece\(s\)", b.stderr)
    assert m and int(m.group(1)) >= 3 and int(m.group(2)) >= 3, b.stderr
    want, data = open(plain, "rb").read(), open(packed, "rb").read()
    assert want == cli(["sort", fq, "-o", "-"]).stdout          # (the buckets change nothing about the order)
    assert gzip.decompress(data) == want and data[-28:] == R.EOF_BLOCK
    assert sum(1 for _, _, isize, _ in R.index(data) if isize == 0) == 1


@pytest.mark.parametrize("env", [{}, {"BSK_HOST_PIPELINE_FROM": "0", "BSK_STAGE_BYTES": "4096", "BSK_STREAM_PIECE_BYTES": "70000"}], ids=["resident", "streamed"])
def test_command_line_devices(inputs, env):
    """--devices 0: the worker's spool is written through a store, the parent joins the spools under ONE EOF block; and a part
    directory holds part00000.gz"""
    d, fq, _ = inputs
    tag = "s" if env else "r"
    plain, packed, pdir = str(d / ("dev-%s.fq" % tag)), str(d / ("dev-%s.fq.gz" % tag)), str(d / ("devdir-%s.gz" % tag))
    a = cli(["seq", "-n", fq, "--devices", "0", "-o", plain, "--merge"], env)
    b = cli(["seq", "-n", fq, "--devices", "0", "-o", packed, "--merge"], env)
    c = cli(["seq", "-n", fq, "--devices", "0", "-o", pdir], env)
    assert a.returncode == 0 and b.returncode == 0 and c.returncode == 0, (a.stderr, b.stderr, c.stderr)
    want, data = open(plain, "rb").read(), open(packed, "rb").read()
    assert want and gzip.decompress(data) == want and data[-28:] == R.EOF_BLOCK
    assert sum(1 for _, _, isize, _ in R.index(data) if isize == 0) == 1
    assert os.listdir(pdir) == ["part00000.gz"]
    part = open(os.path.join(pdir, "part00000.gz"), "rb").read()
    assert gzip.decompress(part) == want and part[-28:] == R.EOF_BLOCK


def test_plain_names_stay_plain(inputs):
    """-o out.fq, -o - and the default <input>-out are text, byte for byte what the library's `seq` gives"""
    import oracle
    d, fq, _ = inputs
    text = open(fq, "rb").read()
    want = oracle.seq(text, True, json.dumps({"Name": True}))
    a = cli(["seq", "-n", fq, "-o", str(d / "p.fq"), "--merge"])
    b = cli(["seq", "-n", fq, "-o", "-"])
    gz = str(d / "in.fq.gz")
    open(gz, "wb").write(bsk.BgzfDeflateHost(text))
    c = cli(["seq", "-n", gz, "--merge"])   # (the default name of a compressed INPUT ends in -out: plain)
    assert a.returncode == 0 and b.returncode == 0 and c.returncode == 0, (a.stderr, b.stderr, c.stderr)
    assert open(str(d / "p.fq"), "rb").read() == want and b.stdout == want and open(gz + "-out", "rb").read() == want


def test_write_seq_file(inputs):
    import torch
    d, fq, _ = inputs
    text = open(fq, "rb").read()
    t = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    n = bsk.WriteSeqFile(d / "w.fq.gz", t)
    data = (d / "w.fq.gz").read_bytes()
    assert n == len(data) and data == bsk.BgzfDeflateHost(text)
    assert bsk.WriteSeqFile(d / "w.fq", t) == len(text) and (d / "w.fq").read_bytes() == text
    back = bsk.ReadSeqFile(d / "w.fq.gz")
    assert back.format == bsk.FORMAT_FASTQ and bytes(back.shards[0].cpu().numpy().tobytes()) == text
    bsk.WriteSeqFile(d / "w2.fq.bgz", bsk.SeqFrame(bsk.FORMAT_FASTQ, [t[:100000], text[100000:200000], t[200000:].cpu()]))
    assert gzip.decompress((d / "w2.fq.bgz").read_bytes()) == text
