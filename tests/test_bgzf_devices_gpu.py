"""BGZF under --devices on the GPU (PARITY.md BGZF "workers"), asked for by BSK_BGZF_DEVICES=1: a worker's shard
(bsk_bgzf_shard_load) over the ranges of the model in bgzf_devices_ref joins to the text zlib gives; the eleven multi-GPU
commands on a BGZF file write what one device writes on the plain text, to every kind of output; which records a worker gets;
empty shards; a range streamed through the piece reader; the join check on a block whose data holds a whole block; and the
refusals.  Workers share the one GPU (--devices 0,0 and 0,0,0).  Without the switch the file is refused as before
(tests/test_bgzf_devices_cpu.py and the older tests hold that)."""
import ctypes as C
import gzip
import os
import re
import subprocess

import pytest

import bgzf_devices_ref as D
import bgzf_ref as R
import bgzf_stream_ref as S
import bigseqkit_amd as bsk
from bigseqkit_amd._lib import lib
from test_run_multi_gpu import fasta as dna_fasta, read_out

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")
ON = {"BSK_BGZF_DEVICES": "1"}
UNSUPPORTED, FORMAT = 4, 3


def cli(args, env=None):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e.update(env or {})
    return subprocess.run([CLI, *args], capture_output=True, cwd=ROOT, env=e, timeout=300)


def ok(args, env=None):
    p = cli(args, env)
    assert p.returncode == 0, (args, p.stderr.decode()[-3000:])
    return p.stdout


def host(t):
    return bytes(t.cpu().numpy().tobytes())


def shard_text(path, lo, hi):
    f = bsk.BgzfShardLoad(path, lo, hi)
    assert len(f.shards) == 1
    return host(f.shards[0])


# ------------------------------------------------------------------ the shard load
@pytest.mark.parametrize("name", list(D.cases()))
def test_shards_join_to_the_text(tmp_path, name):
    """over the model's ranges -- not the library's own cut points -- the shards are the slices of the text"""
    data, fmt = D.cases()[name]
    path = str(tmp_path / (name + (".fq.gz" if fmt == S.FQ else ".fa.gz")))
    open(path, "wb").write(data)
    text = gzip.decompress(data) if data else b""
    starts = S.record_starts(text, fmt)
    for world in D.worlds_of(data):
        _, V, T = D.model(data, fmt, world)
        got = [shard_text(path, V[k], V[k + 1]) for k in range(world)]
        assert got == [text[T[k]:T[k + 1]] for k in range(world)], (name, world)
        assert b"".join(got) == text and all(t in starts for t in T), (name, world)


def test_shard_is_aligned_and_freed_by_its_own_pointer(tmp_path):
    """the pointer handed out is a multiple of 256 also when the shard begins inside a block, and bsk_device_free takes it"""
    data, fmt = D.cases()["fq_mixed"]
    path = str(tmp_path / "a.fq.gz")
    open(path, "wb").write(data)
    _, V, T = D.model(data, fmt, 7)
    inside = [k for k in range(7) if V[k] & 0xFFFF and V[k + 1] & 0xFFFF]
    assert inside
    text = gzip.decompress(data)
    for k in inside[:2]:
        d_text, n = C.c_void_p(), C.c_size_t()
        with open(path, "rb") as f:
            assert lib.bsk_bgzf_shard_load(f.fileno(), V[k], V[k + 1], 0, 0, C.byref(d_text), C.byref(n)) == 0, lib.bsk_global_error()
        assert d_text.value % 256 == 0 and n.value == T[k + 1] - T[k]
        buf = C.create_string_buffer(max(1, n.value))
        assert lib.bsk_device_copy(buf, d_text, n.value, 2) == 0      # BSK_COPY_D2H
        lib.bsk_device_free(d_text)
        assert buf.raw[:n.value] == text[T[k]:T[k + 1]]


def test_join_check_of_the_shard_load(tmp_path):
    """a range that ends at the inner member of the nested file -- bytes that decode as a block but are none of the file's: the
    chain from the range's start steps over it, BSK_ERR_UNSUPPORTED names the offset and says --device N, nothing is handed out"""
    data, fmt, at_inner, true_next = D.nested_member()
    path = str(tmp_path / "nested.fa.gz")
    open(path, "wb").write(data)
    d_text, n = C.c_void_p(), C.c_size_t()
    with open(path, "rb") as f:
        rc = lib.bsk_bgzf_shard_load(f.fileno(), 0, at_inner << 16, 0, 0, C.byref(d_text), C.byref(n))
    msg = lib.bsk_global_error().decode()
    assert rc == UNSUPPORTED and not d_text.value, (rc, msg)
    assert ("offset %d of the file is not a block start" % at_inner) in msg and "--device N" in msg, msg
    # ... and a shard that BEGINS there decodes the inner member, and its chain breaks behind it: a refusal, not bytes
    with pytest.raises(bsk.BskError):
        bsk.BgzfShardLoad(path, at_inner << 16, len(data) << 16)


def test_refusal_of_a_damaged_block_names_the_file_offset(tmp_path):
    data, fmt = D.cases()["fq_small_pieces"]
    idx = R.index(data)
    _, V, _ = D.model(data, fmt, 3)
    first = next(i for i, (o, _, _, _) in enumerate(idx) if o == V[1] >> 16)
    off, bsize = idx[first + 2][0], idx[first + 2][1]
    assert off + bsize <= V[2] >> 16
    bad = bytearray(data)
    bad[off + bsize - 8] ^= 0x10
    path = str(tmp_path / "bad.fq.gz")
    open(path, "wb").write(bytes(bad))
    with pytest.raises(bsk.BskError) as e:
        bsk.BgzfShardLoad(path, V[1], V[2])
    assert e.value.code == FORMAT and "CRC" in str(e.value), str(e.value)
    assert ("block at offset %d (number 2 from the shard's first block at offset %d)" % (off, V[1] >> 16)) in str(e.value), str(e.value)
    assert shard_text(path, V[0], V[1]) == gzip.decompress(data)[:D.model(data, fmt, 3)[2][1]]     # (the shard in front of it is whole)


# ------------------------------------------------------------------ the command line
@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """name -> (plain path, BGZF path, text, format): four-line FASTQ of 260 records and DNA FASTA in blocks of 200 .. 700 text
    bytes, a FASTQ file with duplicates on both sides of every cut, and the FASTA table for fa2fq"""
    d = tmp_path_factory.mktemp("bgzf_devices")
    out = {"dir": d}
    for name, text, fmt in (("fq", S.fastq4(1, 260), S.FQ), ("fa", dna_fasta(40, 12), S.FA), ("dup", D.with_duplicates(), S.FQ)):
        ext = "fa" if fmt == S.FA else "fq"
        plain, z = str(d / ("%s.%s" % (name, ext))), str(d / ("%s.%s.gz" % (name, ext)))
        open(plain, "wb").write(text)
        open(z, "wb").write(S.write_mixed(text, 61) + R.EOF_BLOCK)
        out[name] = (plain, z, text, fmt)
    # fa2fq looks a read's ID up in the table and finds the table's sequence in the read: two reads of three, a part of each
    lines = out["fq"][2].split(b"\n")
    table = str(d / "table.fa")
    open(table, "wb").write(b"".join(b">" + lines[k][1:].split(b" ")[0] + b"\n" + lines[k + 1][2:-2] + b"\n" for k in range(0, len(lines) - 1, 4) if k % 12))
    out["table"] = table
    return out


COMMANDS = {
    # name -> (input, arguments)
    "seq": ("fq", ["seq", "-r", "-p", "-t", "dna", "--quiet"]),
    "seq_fa": ("fa", ["seq", "-w", "70"]),
    "grep": ("fq", ["grep", "-s", "-p", "ACGT"]),
    "grep_fa": ("fa", ["grep", "-s", "-p", "ACGTTG"]),
    "locate": ("fq", ["locate", "-p", "ACGT"]),
    "locate_fa": ("fa", ["locate", "-p", "ACGTTGCA"]),
    "subseq": ("fq", ["subseq", "-r", "2:-2"]),
    "subseq_fa": ("fa", ["subseq", "-r", "5:-5"]),
    "translate": ("fq", ["translate", "-f", "1"]),
    "translate_fa": ("fa", ["translate", "-f", "6", "-x"]),
    "fq2fa": ("fq", ["fq2fa"]),
    "fa2fq": ("fq", ["fa2fq", "-t", "dna", "-f", "TABLE"]),
    "replace": ("fq", ["replace", "-p", "read", "-r", "r"]),
    "replace_fa": ("fa", ["replace", "-s", "-p", "[GC]", "-r", ""]),
    "sample": ("fq", ["sample", "-p", "0.4", "-s", "11"]),
    "sample_fa": ("fa", ["sample", "-p", "0.5", "-s", "7"]),
    "rmdup": ("dup", ["rmdup", "-s"]),
    "rmdup_fa": ("fa", ["rmdup", "-s"]),
}


@pytest.mark.parametrize("name", list(COMMANDS))
def test_every_command_writes_what_one_device_writes(inputs, tmp_path, name):
    """merged on two workers and as a directory of parts on three: the bytes of the single-device run on the plain text"""
    src, args = COMMANDS[name]
    plain, z, _, _ = inputs[src]
    args = [inputs["table"] if a == "TABLE" else a for a in args]
    one, two, three = (str(tmp_path / n) for n in ("one.out", "two.out", "three.out"))
    ok(args + [plain, "-o", one, "--merge"])
    want = open(one, "rb").read()
    assert want
    ok(args + [z, "-o", two, "--merge", "--devices", "0,0"], ON)
    assert open(two, "rb").read() == want
    ok(args + [z, "-o", three, "--devices", "0,0,0"], ON)
    assert sorted(os.listdir(three)) == ["part%05d" % k for k in range(3)] and read_out(three) == want
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]


def test_rmdup_has_duplicates_on_both_sides_of_the_cut(inputs):
    plain, z, text, fmt = inputs["dup"]
    data = open(z, "rb").read()
    _, _, T = D.model(data, fmt, 2)
    seqs = lambda t: set(t.split(b"\n")[1::4])
    assert len(seqs(text[:T[1]]) & seqs(text[T[1]:])) >= 5


@pytest.mark.parametrize("src", ["fq", "fa"])
def test_stats_and_the_grep_count(inputs, src):
    plain, z, _, _ = inputs[src]
    for args in (["stats", "-a", "-T"], ["stats"], ["grep", "-s", "-p", "ACGT", "-C"]):
        want = ok(args + [plain]).replace(plain.encode(), b"F")
        for devs in ("0", "0,0,0"):
            got = ok(args + [z, "--devices", devs], ON).replace(z.encode(), b"F")
            assert want and b" ".join(got.split()) == b" ".join(want.split()), (args, devs, got, want)
            if "-T" in args or "-C" in args:
                assert got == want, (args, devs)


def test_stdout_and_a_gz_output(inputs, tmp_path):
    plain, z, _, _ = inputs["fq"]
    args = ["seq", "-r", "-p", "-t", "dna", "--quiet"]
    want = ok(args + [plain, "-o", "-"])
    assert want and ok(args + [z, "-o", "-", "--devices", "0,0,0"], dict(ON, TMPDIR=str(tmp_path))) == want
    packed = str(tmp_path / "out.fq.gz")
    ok(args + [z, "-o", packed, "--merge", "--devices", "0,0"], ON)
    blob = open(packed, "rb").read()
    assert bsk.BgzfProbe(blob) == 1 and gzip.decompress(blob) == want
    parts = str(tmp_path / "parts.gz")
    ok(args + [z, "-o", parts, "--devices", "0,0"], ON)
    assert sorted(os.listdir(parts)) == ["part00000.gz", "part00001.gz"]
    assert b"".join(gzip.decompress(open(os.path.join(parts, f), "rb").read()) for f in sorted(os.listdir(parts))) == want


def test_a_worker_gets_the_records_of_its_range(inputs, tmp_path):
    """without --merge: part k of `seq` is the single-device result on text[T(V_k), T(V_k+1)) of the model"""
    plain, z, text, fmt = inputs["fq"]
    data = open(z, "rb").read()
    args = ["seq", "-r", "-p", "-t", "dna", "--quiet"]
    for world in (2, 3):
        _, _, T = D.model(data, fmt, world)
        out = str(tmp_path / ("parts%d" % world))
        ok(args + [z, "-o", out, "--devices", ",".join("0" * world)], ON)
        for k in range(world):
            piece = str(tmp_path / ("slice%d_%d.fq" % (world, k)))
            open(piece, "wb").write(text[T[k]:T[k + 1]])
            assert T[k + 1] > T[k]
            assert open(os.path.join(out, "part%05d" % k), "rb").read() == ok(args + [piece, "-o", "-"]), (world, k)


def test_more_workers_than_blocks(tmp_path):
    """three blocks under five workers: shards are empty, every worker still enters every collective and writes its part"""
    text = S.fastq4(8, 12)
    third = len(text) // 3
    data = b"".join(R.member(R.deflate(t), t) for t in (text[:third], text[third:2 * third], text[2 * third:]))
    assert len(R.index(data)) == 3
    plain, z = str(tmp_path / "few.fq"), str(tmp_path / "few.fq.gz")
    open(plain, "wb").write(text)
    open(z, "wb").write(data)
    V = D.model(data, S.FQ, 5)[1]
    assert sum(1 for a, b in zip(V, V[1:]) if a == b) >= 2
    assert ok(["stats", "-a", "-T", z, "--devices", "0,0,0,0,0"], ON) == ok(["stats", "-a", "-T", plain]).replace(plain.encode(), z.encode())
    out = str(tmp_path / "parts")
    ok(["seq", "-r", z, "-o", out, "--devices", "0,0,0,0,0"], ON)
    assert sorted(os.listdir(out)) == ["part%05d" % k for k in range(5)]
    assert read_out(out) == ok(["seq", "-r", plain, "-o", "-"])
    one, many = str(tmp_path / "one.out"), str(tmp_path / "many.out")
    ok(["rmdup", "-s", plain, "-o", one, "--merge"])
    ok(["rmdup", "-s", z, "-o", many, "--merge", "--devices", "0,0,0,0,0"], ON)
    assert open(many, "rb").read() == open(one, "rb").read()


def test_a_record_longer_than_a_workers_range(tmp_path):
    """the 9 000-base FASTA record over 500-byte blocks under seven workers: the ranges inside it are empty shards"""
    data, fmt = D.cases()["fa_long_record"]
    text = gzip.decompress(data)
    plain, z = str(tmp_path / "long.fa"), str(tmp_path / "long.fa.gz")
    open(plain, "wb").write(text)
    open(z, "wb").write(data)
    V = D.model(data, fmt, 7)[1]
    assert any(a == b for a, b in zip(V, V[1:]))
    devs = ",".join("0" * 7)
    assert ok(["stats", "-a", "-T", z, "--devices", devs], ON) == ok(["stats", "-a", "-T", plain]).replace(plain.encode(), z.encode())
    out = str(tmp_path / "parts")
    ok(["seq", "-w", "70", z, "-o", out, "--devices", devs], ON)
    assert read_out(out) == ok(["seq", "-w", "70", plain, "-o", "-"])


def test_stats_streams_a_range_that_is_not_loaded_whole(inputs):
    """BSK_HOST_PIPELINE_FROM=0: no range is loaded whole.  With BSK_BGZF_STREAM=1 every worker reads its range through the piece
    reader, several pieces each, and the table is the single-device table; without it the refusal names the switch"""
    plain, z, _, _ = inputs["fq"]
    env = dict(ON, BSK_HOST_PIPELINE_FROM="0", BSK_BGZF_STREAM="1", BSK_STREAM_PIECE_BYTES="1500")
    want = ok(["stats", "-a", "-T", plain]).replace(plain.encode(), z.encode())
    for devs in ("0,0", "0,0,0"):
        assert ok(["stats", "-a", "-T", z, "--devices", devs], env) == want, devs
    p = cli(["stats", "-a", "-T", z, "--devices", "0,0"], dict(ON, BSK_HOST_PIPELINE_FROM="0"))
    assert p.returncode == 1 and not p.stdout and b"BSK_BGZF_STREAM=1" in p.stderr, p.stderr
    # a failed resident load goes the same way
    assert ok(["stats", "-a", "-T", z, "--devices", "0,0"], dict(ON, BSK_SHARD_FAIL_ALLOC="1", BSK_BGZF_STREAM="1", BSK_STREAM_PIECE_BYTES="1500")) == want


def test_nested_member_under_two_workers(tmp_path):
    """the file whose stored block holds a whole BGZF member behind the nominal cut: the result is the single-device result, or
    the run is refused -- exit status 1, the offset and --device N named -- and has written no part file"""
    data, fmt, at_inner, true_next = D.nested_member()
    text = gzip.decompress(data)
    plain, z = str(tmp_path / "nested.fa"), str(tmp_path / "nested.fa.gz")
    open(plain, "wb").write(text)
    open(z, "wb").write(data)
    out = str(tmp_path / "parts")
    p = cli(["seq", "-w", "70", z, "-o", out, "--devices", "0,0"], ON)
    if p.returncode == 0:
        assert read_out(out) == ok(["seq", "-w", "70", plain, "-o", "-"])
        assert ok(["stats", "-T", z, "--devices", "0,0"], ON) == ok(["stats", "-T", plain]).replace(plain.encode(), z.encode())
    else:
        err = p.stderr.decode()
        assert p.returncode == 1 and re.search(r"offset \d+ of the file is not a block start", err) and "--device N" in err, err
        assert not os.path.isdir(out) or not [f for f in os.listdir(out) if f.startswith("part")], os.listdir(out)


@pytest.mark.parametrize("args", [["seq", "-r"], ["rmdup", "-s"]])
def test_a_shard_above_the_pipeline_line_is_refused(inputs, tmp_path, args):
    """BSK_HOST_PIPELINE_FROM=0 sends every plain shard through the host pipeline, which is not built for compressed shards:
    refused before anything is written, with the sizes and the way out"""
    _, z, _, _ = inputs["fq"]
    out = str(tmp_path / "parts")
    p = cli(args + [z, "-o", out, "--devices", "0,0"], dict(ON, BSK_HOST_PIPELINE_FROM="0"))
    err = p.stderr.decode()
    assert p.returncode == 1 and "more devices make smaller shards" in err and re.search(r"\d+ compressed bytes, \d+ bytes of text", err), err
    assert not os.path.isdir(out) or not [f for f in os.listdir(out) if f.startswith("part")]


def test_timing_names_the_cut_points(inputs):
    _, z, _, _ = inputs["fq"]
    p = cli(["stats", z, "--devices", "0,0"], dict(ON, BSK_CLI_TIMING="1"))
    assert p.returncode == 0 and b"bgzf cut points" in p.stderr and b"bgzf shard on the device" in p.stderr, p.stderr
