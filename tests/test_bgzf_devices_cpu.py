"""BGZF under --devices without a GPU (PARITY.md BGZF "workers"): the cut points of the host rule against the definitions
restated in bgzf_devices_ref -- on every file of the piece reader's tests at five numbers of workers --, false candidates, a
damaged file, the header alone under the host's sanitizers, and what the command line says before a device is touched."""
import ctypes as C
import os
import re
import subprocess

import pytest

import bgzf_devices_ref as D
import bgzf_ref as R
import bgzf_stream_ref as S
import bigseqkit_amd as bsk
from bigseqkit_amd._lib import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")
NO_DEVICE = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}
FORMAT, UNSUPPORTED = 3, 4


def put(tmp_path, name, data):
    p = str(tmp_path / (name + ".gz"))
    with open(p, "wb") as f:
        f.write(data)
    return p


def cut_points(path, fmt, world):
    """(code, voffs, message) straight from the C ABI"""
    voffs = (C.c_uint64 * (world + 1))()
    with open(path, "rb") as f:
        rc = lib.bsk_bgzf_cut_points(f.fileno(), fmt, world, voffs)
    return rc, [int(v) for v in voffs], lib.bsk_global_error().decode()


def test_cut_points_are_the_models(tmp_path):
    seen_empty = seen_inside = 0
    for name, (data, fmt) in D.cases().items():
        path = put(tmp_path, name, data)
        blocks, text = D.layout(data)
        starts = S.record_starts(text, fmt)
        for world in D.worlds_of(data):
            B, V, T = D.model(data, fmt, world)
            got = bsk.BgzfCutPoints(path, fmt, world)
            assert got == V, (name, world, got, V)
            assert len(got) == world + 1 and got[-1] == len(data) << 16 and got == sorted(got), (name, world)
            assert all(t in starts for t in T), (name, world)
            seen_empty += sum(1 for a, b in zip(V, V[1:]) if a == b)
            seen_inside += sum(1 for v in V if v & 0xFFFF)
    assert seen_empty and seen_inside    # (empty shards and cuts inside a block are both among the cases)


@pytest.mark.parametrize("width", [11, 30])
def test_wrapped_fastq_where_the_host_rule_is_exact(tmp_path, width):
    data = R.write(S.fastq_wrapped(4, 120, width), block=400)
    path = put(tmp_path, "wrapped%d" % width, data)
    for world in (2, 3, 7):
        assert bsk.BgzfCutPoints(path, S.FQ, world) == D.model(data, S.FQ, world)[1], (width, world)


def test_a_long_record_gives_empty_shards(tmp_path):
    """the 9 000-base record over 500-byte blocks: at 40 workers several ranges lie inside it"""
    data, fmt = D.cases()["fa_long_record"]
    V = bsk.BgzfCutPoints(put(tmp_path, "long", data), fmt, 40)
    assert V == D.model(data, fmt, 40)[1]
    assert sum(1 for a, b in zip(V, V[1:]) if a == b) >= 5


def test_signature_in_a_stored_block_is_no_cut(tmp_path):
    """a bare header signature inside a stored block, the nominal cut just in front of it: the cut is the true block behind it
    (the signature makes the text no FASTQ: it is read by the FASTA rule, a record wherever a line begins with '>')"""
    base = R.corpus()["signature_in_stored"]
    sig = base.index(R.HEADER_SIGNATURE, 1)
    assert sig not in [off for off, _, _, _ in R.index(base)]
    # F bytes of blocks in front of the file move size // 2 to the byte in front of the signature: (size + F) // 2 == sig + F - 1
    F = len(base) - 2 * sig + 2
    assert F > 200
    pad_text = R.fastq_text(150, seed=3)
    pad_text = pad_text[:pad_text.rfind(b"\n@") + 1]     # (whole records)
    pad = R.member(R.deflate(pad_text, level=0), pad_text)
    front = b""
    while len(front) + 2 * len(pad) <= F:
        front += pad
    # the last one sized to the byte by its header line (a stored block's frame is 18 + 5 + 8 bytes)
    need = F - len(front) - 31
    rec = b"@pad \nACGT\n+\nIIII\n"
    assert need >= len(rec)
    rec = b"@pad " + b"x" * (need - len(rec)) + rec[5:]
    front += R.member(R.deflate(rec, level=0), rec)
    assert len(front) == F
    data = front + base
    sig += F
    assert len(data) // 2 == sig - 1 and data[sig:sig + 16] == R.HEADER_SIGNATURE
    B, V, _ = D.model(data, S.FA, 2)
    assert B[1] > sig
    path = put(tmp_path, "sig", data)
    assert bsk.BgzfCutPoints(path, S.FA, 2) == V
    for world in (3, 5):     # (here the signature lies among the candidates in front of a cut: its chain breaks at once)
        assert bsk.BgzfCutPoints(path, S.FA, world) == D.model(data, S.FA, world)[1], world


def test_nested_member_never_gives_another_answer(tmp_path):
    """the data of a stored block holds a whole valid BGZF member behind the nominal cut: the cut points are the model's, or the
    call does not answer BSK_OK (the worker's join check is what catches a fake cut that passes: test_bgzf_devices_gpu)"""
    data, fmt, at_inner, true_next = D.nested_member()
    assert len(data) // 2 <= at_inner < true_next
    rc, voffs, msg = cut_points(put(tmp_path, "nested", data), fmt, 2)
    assert rc != 0 or voffs == D.model(data, fmt, 2)[1], (rc, voffs, msg)


@pytest.mark.parametrize("what", ["crc", "bsize"])
def test_damaged_block_at_the_cut(tmp_path, what):
    data, fmt = D.cases()["fq_small_pieces"]
    idx = R.index(data)
    nominal = len(data) // 2
    off, bsize = next((o, b) for o, b, _, _ in idx if o <= nominal < o + b)
    bad = bytearray(data)
    if what == "crc":
        bad[off + bsize - 8] ^= 0x10
    else:
        bad[off + 16] = (bad[off + 16] + 3) & 0xFF     # BSIZE: the chain lands inside the next block
    path = put(tmp_path, "damaged_" + what, bytes(bad))
    rc, _, msg = cut_points(path, fmt, 2)
    assert rc == FORMAT, (rc, msg)
    assert str(off) in re.findall(r"\d+", msg), msg
    with pytest.raises(bsk.BskError) as e:
        bsk.BgzfCutPoints(path, fmt, 2)
    assert e.value.code == FORMAT
    # (one worker reads no cut: the damage is the decoder's to report)
    assert bsk.BgzfCutPoints(path, fmt, 1) == [0, len(bad) << 16]


def test_not_bgzf(tmp_path):
    import gzip
    rc, _, msg = cut_points(put(tmp_path, "plain", gzip.compress(S.fastq4(1, 20))), S.FQ, 2)
    assert rc == UNSUPPORTED and "bgzip" in msg
    rc, _, msg = cut_points(put(tmp_path, "text", S.fastq4(1, 20)), S.FQ, 2)
    assert rc == FORMAT and "not gzip" in msg


PRESENT = (" is BGZF-compressed, and --devices cuts a file by its bytes, which a compressed file does not allow yet; run it on one device (--device N), "
           "or decompress it first (bgzip -d)")
GZIP_DEVICES = (" is gzip but not BGZF, and --devices cuts a file by its bytes: where a worker starts in a gzip stream is known only after a pass "
                "over the stream in front of it, so BSK_GZIP_STREAM=1 reads it in pieces on one device only; run it on one device (--device N), or "
                "decompress it first (gzip -d)")
GZIP_PIECES = (" is gzip but not BGZF, and --devices cuts a file in pieces: a gzip stream has no virtual offsets to re-enter at, so BSK_GZIP=1 "
               "reads it only where a file is read whole; decompress it first (gzip -d), or recompress it with bgzip (gzip -dc FILE | bgzip > FILE.gz)")


def test_switch_and_refusals_without_a_device(tmp_path):
    import gzip
    import itertools
    fq = S.fastq4(1, 12)
    b = put(tmp_path, "x.fq", R.write(fq, block=200))
    z = put(tmp_path, "z.fq", gzip.compress(fq, mtime=0))

    def run(args, env):
        e = {k: v for k, v in os.environ.items() if not k.startswith(("BSK_GZIP", "BSK_BGZF"))}
        r = subprocess.run([CLI, *args], capture_output=True, timeout=120, env=dict(e, **NO_DEVICE, **env))
        return r.returncode, r.stdout, r.stderr.decode()

    # without the new switch: the present text, whatever the other three switches say
    for on in itertools.product((False, True), repeat=3):
        env = {k: "1" for k, v in zip(("BSK_BGZF_STREAM", "BSK_GZIP", "BSK_GZIP_STREAM"), on) if v}
        for extra in ({}, {"BSK_BGZF_DEVICES": "0"}, {"BSK_BGZF_DEVICES": ""}):
            assert run(["stats", "--devices", "0", b], dict(env, **extra)) == (1, b"", "Error: " + b + PRESENT + "\n"), (env, extra)
    # with it the file is admitted: the next thing the run needs is a device
    code, out, err = run(["stats", "--devices", "0", b], {"BSK_BGZF_DEVICES": "1"})
    assert (code, out) == (1, b"") and "no HIP device visible" in err and "BGZF-compressed" not in err, err
    # plain gzip keeps its two texts
    for stream in ({}, {"BSK_BGZF_STREAM": "1"}):
        assert run(["stats", "--devices", "0", z], dict(stream, BSK_BGZF_DEVICES="1", BSK_GZIP="1", BSK_GZIP_STREAM="1"))[2] == "Error: " + z + GZIP_DEVICES + "\n"
        assert run(["stats", "--devices", "0", z], dict(stream, BSK_BGZF_DEVICES="1", BSK_GZIP="1"))[2] == "Error: " + z + GZIP_PIECES + "\n"


def test_host_rule_under_sanitizers(tmp_path):
    """tests/host_c/bgzf_cuts_check.cpp -- bgzf_cuts.hpp and nothing of the library -- built with the host's address and
    undefined-behaviour sanitizers: the model's cut points on every case, a refusal on the damaged file, and no report"""
    exe = str(tmp_path / "bgzf_cuts_check")
    src = os.path.join(ROOT, "tests", "host_c", "bgzf_cuts_check.cpp")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("the sanitizer runtime cannot be linked here")
    assert r.returncode == 0, r.stderr[-2000:]

    def run(data, fmt, world):
        path = put(tmp_path, "in", data)
        p = subprocess.run([exe, path, str(fmt), str(world)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and not p.stderr, (p.stdout[-500:], p.stderr[-2000:])
        return p.stdout.split()

    for name, (data, fmt) in D.cases().items():
        for world in (2, 7):
            assert run(data, fmt, world) == ["ok"] + [str(v) for v in D.model(data, fmt, world)[1]], (name, world)
    data, fmt = D.cases()["fq_small_pieces"]
    off, bsize = next((o, b) for o, b, _, _ in R.index(data) if o <= len(data) // 2 < o + b)
    bad = bytearray(data)
    bad[off + bsize - 8] ^= 0x10
    assert run(bytes(bad), fmt, 2)[:2] == ["refused", str(FORMAT)]
    nested, nfmt, _, _ = D.nested_member()
    out = run(nested, nfmt, 2)
    assert out[0] == "refused" or out == ["ok"] + [str(v) for v in D.model(nested, nfmt, 2)[1]]
