"""`head-genome` on the GPU, byte for byte against tests/head_genome_ref.py (PARITY.md HEADG): the block boundaries of the
reduction, every input shape the record readers know, the hand fixtures through the C ABI, growing windows against one
window, any cut into shards, a context that serves a second file, and the command line."""
import ctypes as C
import json
import os
import random
import re
import subprocess

import pytest

import bigseqkit_amd as bsk
from bigseqkit_amd._lib import BskError, Out, lib, check
import oracle
import head_genome_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "head_genome_fixtures.json")))
CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")


def wrap(t, w):
    return "\n".join(t[i:i + w] for i in range(0, len(t), w)) if w else t


def small(kinds, fastq=False):
    """records of about 20 bytes; kinds[i]: 'A' first genome (n = 2), 'B' another one (n = 0 < m), '-' no description"""
    out = []
    for i, k in enumerate(kinds):
        head = "c%d" % i if k == "-" else "c%d %s k%d" % (i, "G A" if k == "A" else "H B", i)
        out.append("@%s\nACGT\n+\nIIII\n" % head if fastq else ">%s\nACGT\n" % head)
    return "".join(out).encode()


def genomes(rng, n_a, n_b, lo, hi, width=0, fastq=False, sep="\n", head_extra=""):
    out = []
    for i in range(n_a + n_b):
        L = rng.randint(lo, hi)
        s = "".join(rng.choice("ACGT") for _ in range(L))
        head = "s%d%s Vibrio cholerae strain %s contig_%d" % (i, head_extra, "M29" if i < n_a else "2012HC-12", i)
        if fastq:
            q = "".join(rng.choice("ABCDEFGHI") for _ in range(L))
            out.append("@%s\n%s\n+\n%s\n" % (head, wrap(s, width), wrap(q, width)))
        else:
            out.append(">%s\n%s%s" % (head, wrap(s, width) + "\n" if L else "", sep[1:]))
    return "".join(out).encode()


def inputs():
    rng = random.Random(91)
    big = ">big Vibrio cholerae strain M29 the_long_one\n" + wrap("".join(rng.choice("ACGT") for _ in range((1 << 20) + 4321)), 70) + "\n"
    a = genomes(rng, 12, 0, 1, 100, 60)
    return [
        ("fasta wrapped", genomes(rng, 150, 90, 0, 400, 60), False),
        ("fasta irregular wrapping", genomes(rng, 60, 40, 1, 300, 7), False),
        ("fasta blank lines", genomes(rng, 70, 50, 1, 120, 50, sep="\n\n\n"), False),
        ("fasta > inside headers", genomes(rng, 70, 50, 1, 120, 0, head_extra=">x"), False),
        ("fasta crlf", genomes(rng, 50, 40, 1, 150, 60).replace(b"\n", b"\r\n"), False),
        ("fasta no final newline, no cut", genomes(rng, 90, 0, 1, 200, 60)[:-1], False),
        ("fasta tiny records", small("A" * 500 + "B" * 300), False),
        ("fasta with a record over a MiB inside the first genome", a + big.encode() + genomes(rng, 10, 15, 1, 100, 60), False),
        ("fastq", genomes(rng, 200, 150, 1, 200, fastq=True), True),
        ("fastq no final newline, no cut", genomes(rng, 120, 0, 1, 100, fastq=True)[:-1], True),
        ("fastq crlf", genomes(rng, 60, 50, 1, 80, fastq=True).replace(b"\n", b"\r\n"), True),
        ("fastq tiny records", small("A" * 600 + "B" * 200, fastq=True), True),
        ("fastq wrapped", genomes(rng, 130, 90, 1, 90, 17, fastq=True), True),
    ]


INPUTS = inputs()
IDS = [x[0] for x in INPUTS]


def frame(data, fastq, parts=1, device=False, cuts=None):
    """`data` as shards that begin on record starts (the oracle's: the cut does not hang on the library under test)"""
    f = (bsk.ReadFASTQN if fastq else bsk.ReadFASTAN)(data, 1)
    if parts > 1 or cuts:
        starts = [s for s, _ in oracle.record_spans(data, fastq)]
        if cuts is None:
            cuts = {starts[len(starts) * k // parts] for k in range(1, parts)} if starts else set()
        else:
            cuts = {starts[k] for k in cuts}
        cuts = sorted({0, len(data)} | cuts)
        f = bsk.SeqFrame(f.format, [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])])
    if device:
        import torch
        f = bsk.SeqFrame(f.format, [torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda() if len(s) else torch.empty(0, dtype=torch.uint8, device="cuda")
                                    for s in f.shards])
    return f


def gpu(data, fastq, parts=1, device=False, cuts=None, **o):
    try:
        return "ok", bsk.HeadGenome(frame(data, fastq, parts, device, cuts), bsk.SeqKitHeadGenomeOptions(**o))
    except BskError as e:
        return "error", str(e)


def ref(data, fastq, **o):
    try:
        return "ok", R.head_genome(data, fastq, o.get("mini_common_words", 1), o.get("line_width", 60), o.get("id_regexp", ""))
    except R.HeadGenomeError as e:
        return "error", str(e)


def same(got, want):
    return got[0] == want[0] and (got[1] == want[1] if got[0] == "ok" else want[1] in got[1])


# ---- the reduction: one verdict per record, a minimum per wave (64), per block (256) and over the blocks
@pytest.mark.parametrize("cut", [1, 63, 64, 65, 255, 256, 257, 511, 513, None])
def test_cut_at_the_boundaries_of_waves_and_blocks(cut):
    data = small("A" * 700) if cut is None else small("A" * cut + "B" + "A" * (699 - cut))
    want = ref(data, False)
    assert want[0] == "ok" and len(R.heads(want[1], False)) == (700 if cut is None else cut)
    assert gpu(data, False) == want
    assert gpu(data, False, device=True) == want
    fq = small("A" * 700, True) if cut is None else small("A" * cut + "B" + "A" * (699 - cut), True)
    assert gpu(fq, True) == ref(fq, True)


def test_the_lower_of_two_cuts_in_different_blocks_wins():
    data = small("A" * 300 + "B" + "A" * 299 + "B" + "A" * 100)
    want = ref(data, False)
    assert len(R.heads(want[1], False)) == 300 and gpu(data, False) == want
    data = small("A" * 600 + "BB" + "A" * 100 + "B")  # (and the higher block's alone)
    assert len(R.heads(ref(data, False)[1], False)) == 600 and gpu(data, False) == ref(data, False)


def test_no_description_behind_and_before_the_cut():
    behind = small("A" * 100 + "B" + "A" * 599 + "-" + "A" * 20)  # a record without description in a block behind the cut
    assert ref(behind, False)[0] == "ok" and gpu(behind, False) == ref(behind, False)
    before = small("A" * 350 + "-" + "A" * 200 + "B" + "A" * 100)  # ... in a block before it: the call fails and names it
    assert ref(before, False) == ("error", "no description: c350") and same(gpu(before, False), ref(before, False))
    two = small("A" * 70 + "-" + "A" * 400 + "-" + "A" * 10)       # the lowest one is named
    assert ref(two, False) == ("error", "no description: c70") and same(gpu(two, False), ref(two, False))
    first = small("-" + "A" * 300)
    assert ref(first, False) == ("error", "no description: c0") and same(gpu(first, False), ref(first, False))
    same_block = small("A" * 10 + "B" + "-" + "A" * 10)            # cut and no description side by side, both orders
    assert ref(same_block, False)[0] == "ok" and gpu(same_block, False) == ref(same_block, False)
    other = small("A" * 10 + "-" + "B" + "A" * 10)
    assert ref(other, False) == ("error", "no description: c10") and same(gpu(other, False), ref(other, False))


# ---- input shapes
@pytest.mark.parametrize("name,data,fastq", INPUTS, ids=IDS)
def test_equals_the_restatement(name, data, fastq):
    for o in ({}, {"line_width": 0}, {"line_width": 7}, {"mini_common_words": 3}, {"mini_common_words": 4}, {"mini_common_words": 9}):
        want = ref(data, fastq, **o)
        assert want[0] == "ok"
        assert gpu(data, fastq, **o) == want, (name, o)
    assert gpu(data, fastq, parts=3, device=True) == ref(data, fastq), name


def test_other_id_expressions_have_no_description():
    data = b">gi|110645304|ref|NC_002516.2| Pseudomonas aeruginosa PAO1\nACGT\n>gi|2|ref|X| Pseudomonas aeruginosa PAO1\nAC\n"
    assert gpu(data, False) == ("ok", data)
    for rx in (R.NCBI, r"^(\w+)\|"):
        want = ref(data, False, id_regexp=rx)
        assert want[0] == "error" and same(gpu(data, False, id_regexp=rx), want), rx


# ---- the hand fixtures, through the C ABI
def run_abi(ctx, data, fmt, on_device=False):
    import torch
    keep = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if on_device and data else (C.c_char * max(1, len(data))).from_buffer_copy(data or b"\0")
    ptr = C.c_void_p(keep.data_ptr()) if on_device and data else C.cast(keep, C.c_void_p)
    out = Out()
    check(lib.bsk_head_genome_run(ctx, ptr, len(data), 1 if on_device and data else 0, fmt, 0, None, C.byref(out)), ctx)
    buf = C.create_string_buffer(max(1, out.len))
    check(lib.bsk_out_to_host(ctx, C.byref(out), buf, out.len), ctx)
    return buf.raw[:out.len]


@pytest.mark.parametrize("case", [c for c in FIX["cases"] if "input" in c], ids=[c["name"] for c in FIX["cases"] if "input" in c])
def test_hand_fixtures(case):
    data = case["input"].encode()
    opts = json.dumps({"MiniCommonWords": case["m"], "Config": {"LineWidth": FIX["line_width"]}})
    if "create_error" in case:
        with pytest.raises(BskError, match=re.escape(case["create_error"])):
            bsk.Operator("HeadGenome", opts, 0)
        return
    with bsk.Operator("HeadGenome", opts, 0) as op:
        for on_device in (False, True):
            check(lib.bsk_head_genome_reset(op.ctx), op.ctx)
            if "error" in case:
                with pytest.raises(BskError, match=re.escape(case["error"])):
                    run_abi(op.ctx, data, bsk.FORMAT_FASTA, on_device)
                continue
            assert run_abi(op.ctx, data, bsk.FORMAT_FASTA, on_device) == case["want"].encode()
            cut, recs = C.c_int(), C.c_uint64()
            check(lib.bsk_head_genome_state(op.ctx, C.byref(cut), C.byref(recs)), op.ctx)
            total = len(oracle.record_spans(data, False)) if data else 0
            assert recs.value == case["kept"] and bool(cut.value) == (case["kept"] < total)


# ---- windows: the cost follows the first genome; the result does not depend on them
def fixed(kinds, size=32):
    """FASTA records of exactly `size` bytes"""
    out = []
    for i, k in enumerate(kinds):
        head = ">c%d G %s" % (i, k)
        out.append(head + "\n" + "A" * (size - len(head) - 2) + "\n")
    return "".join(out).encode()


WINDOW_CASES = [
    ("cut in the first window", fixed("AAAB" + "A" * 400)),
    ("cut exactly at a window end", fixed("A" * 8 + "B" + "A" * 300)),            # record 8 begins at byte 256
    ("cut at the end of the 4096 window", fixed("A" * 128 + "B" + "A" * 300)),     # ... at byte 4096
    ("cut several windows in", fixed("A" * 3000 + "B" + "A" * 500)),
    ("a record longer than a window", fixed("A" * 5) + b">long G A\n" + b"ACGT" * 3000 + b"\n" + fixed("A" * 40 + "B" + "A" * 40)[0:]),
    ("a record longer than a window first", b">long G A\n" + (b"ACGTACGTAC\n" * 1000) + fixed("A" * 40 + "B" + "A" * 40)),
    ("cut never reached", fixed("A" * 2500)),
    ("no description several windows in", fixed("A" * 700) + b">nodesc\nACGT\n" + fixed("A" * 10)),
]


@pytest.mark.parametrize("window", ["256", "4096"])
@pytest.mark.parametrize("name,data", WINDOW_CASES, ids=[c[0] for c in WINDOW_CASES])
def test_windows_against_one_window(name, data, window, monkeypatch):
    want = ref(data, False)
    monkeypatch.setenv("BSK_HEAD_GENOME_WINDOW", "0")
    whole = gpu(data, False, device=True)
    assert same(whole, want), name
    monkeypatch.setenv("BSK_HEAD_GENOME_WINDOW", window)
    for device in (True, False):
        assert gpu(data, False, device=device) == whole, (name, window, device)
    assert gpu(data, False, parts=3, device=True) == whole


@pytest.mark.parametrize("window", ["256", "4096"])
def test_windows_on_every_input_shape(window, monkeypatch):
    monkeypatch.setenv("BSK_HEAD_GENOME_WINDOW", window)
    for name, data, fastq in INPUTS:
        assert gpu(data, fastq, device=True) == ref(data, fastq), (name, window)
    fq = small("A" * 300 + "B" + "A" * 300, True)
    assert gpu(fq, True, device=True) == ref(fq, True)


def test_a_cut_in_the_first_kib_does_not_index_the_shard():
    """the profile of a shard of a few MiB whose cut lies in the first KiB: fewer bytes indexed than the shard holds"""
    import torch
    rng = random.Random(5)
    data = fixed("A" * 20 + "B") + genomes(rng, 0, 12000, 100, 400, 60)
    assert len(data) > 3 << 20
    want = ref(data, False)
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    seen = {}
    for window in ("65536", "0"):
        with bsk.Operator("HeadGenome", "{}", 0) as op:
            check(lib.bsk_ctx_set(op.ctx, b"head_genome_window", window.encode()), op.ctx)
            lib.bsk_profile_reset(op.ctx)
            lib.bsk_profile_enable(op.ctx, 1)
            out = Out()
            check(lib.bsk_head_genome_run(op.ctx, C.c_void_p(t.data_ptr()), t.numel(), 1, bsk.FORMAT_FASTA, 0, None, C.byref(out)), op.ctx)
            buf = C.create_string_buffer(max(1, out.len))
            check(lib.bsk_out_to_host(op.ctx, C.byref(out), buf, out.len), op.ctx)
            assert ("ok", buf.raw[:out.len]) == want
            pb = C.create_string_buffer(1 << 16)
            check(lib.bsk_profile_dump(op.ctx, pb, len(pb)), op.ctx)
            prof = dict(kv.split("=") for kv in pb.value.decode().split(";") if kv)
            for stage in ("hg_window_index", "hg_verdict", "hg_emit"):
                assert stage in prof, prof
            seen[window] = int(prof["hg_indexed_bytes"].split("/")[1])
    assert seen["0"] == len(data)
    assert 0 < seen["65536"] <= 65536 < len(data), seen


# ---- shards: one cut over the whole input
@pytest.mark.parametrize("device", [False, True])
def test_any_cut_into_shards_gives_the_same_bytes(device):
    n_a, n_b = 60, 45
    data = genomes(random.Random(12), n_a, n_b, 1, 120, 60)
    want = ref(data, False)
    assert len(R.heads(want[1], False)) == n_a
    for parts in (1, 2, 3, 7):
        assert gpu(data, False, parts=parts, device=device) == want, parts
    for cuts in ([80], [n_a], [n_a - 1, n_a], [n_a, n_a + 1], [1], [1, 2], [10, 20, 30], [100]):
        # the cut inside shard 0, exactly at a shard boundary, in the last shard; a first shard of one record
        assert gpu(data, False, cuts=cuts, device=device) == want, cuts
    allkept = genomes(random.Random(13), 40, 0, 1, 120, 60)
    for cuts in ([1], [1, 2, 3], [20]):
        assert gpu(allkept, False, cuts=cuts, device=device) == ref(allkept, False), cuts
    fq = genomes(random.Random(14), 50, 30, 1, 100, fastq=True)
    for cuts in ([1], [50], [25, 60], [70]):
        assert gpu(fq, True, cuts=cuts, device=device) == ref(fq, True), cuts
    nodesc = small("A" * 30 + "B" + "A" * 30 + "-")
    assert gpu(nodesc, False, cuts=[1, 40], device=device) == ref(nodesc, False)
    nodesc = small("A" * 30 + "-" + "A" * 30)
    assert same(gpu(nodesc, False, cuts=[1, 20], device=device), ref(nodesc, False))


def test_a_reset_context_serves_a_second_file():
    one = genomes(random.Random(21), 20, 20, 1, 100, 60)
    two = small("A" * 5 + "B" * 5)
    with bsk.Operator("HeadGenome", "{}", 0) as op:
        assert ("ok", run_abi(op.ctx, one, bsk.FORMAT_FASTA)) == ref(one, False)
        assert run_abi(op.ctx, two, bsk.FORMAT_FASTA) == b""  # the cut is reached: what follows is behind it
        check(lib.bsk_head_genome_reset(op.ctx), op.ctx)
        assert ("ok", run_abi(op.ctx, two, bsk.FORMAT_FASTA, True)) == ref(two, False)
        check(lib.bsk_head_genome_reset(op.ctx), op.ctx)
        assert run_abi(op.ctx, b"", bsk.FORMAT_FASTA) == b""
        assert ("ok", run_abi(op.ctx, one, bsk.FORMAT_FASTA, True)) == ref(one, False)


# ---- the command line
def cli(args, env=None):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e.update(env or {})
    return subprocess.run([CLI, *args], capture_output=True, timeout=600, env=e)


def test_command_line(tmp_path):
    a = genomes(random.Random(31), 40, 30, 1, 150, 60)
    b = genomes(random.Random(32), 25, 50, 1, 100, fastq=False, width=60).replace(b"M29", b"N16961")
    big = genomes(random.Random(33), 900, 700, 50, 200, 60)
    for name, text in (("a.fa", a), ("b.fa", b), ("big.fa", big)):
        (tmp_path / name).write_bytes(text)
    p = cli(["head-genome", str(tmp_path / "a.fa"), "-o", "-"])
    assert p.returncode == 0, p.stderr
    assert ("ok", p.stdout) == ref(a, False)
    # two files: each keeps its own first genome, in order
    p = cli(["head-genome", "-w", "0", str(tmp_path / "a.fa"), str(tmp_path / "b.fa"), "-o", "-"])
    assert p.returncode == 0, p.stderr
    assert p.stdout == ref(a, False, line_width=0)[1] + ref(b, False, line_width=0)[1]
    # streamed in small pieces: the state is carried from piece to piece
    for piece in ("3000", "70000"):
        p = cli(["head-genome", str(tmp_path / "big.fa"), "-o", "-"], {"BSK_STREAM_PIECE_BYTES": piece})
        assert p.returncode == 0, p.stderr
        assert ("ok", p.stdout) == ref(big, False), piece
    p = cli(["head-genome", "-m", "9", str(tmp_path / "big.fa"), "-o", str(tmp_path / "out.fa"), "--merge"], {"BSK_STREAM_PIECE_BYTES": "3000"})
    assert p.returncode == 0 and (tmp_path / "out.fa").read_bytes() == ref(big, False, mini_common_words=9)[1]


def test_command_line_errors(tmp_path):
    (tmp_path / "n.fa").write_bytes(small("A" * 400 + "-" + "A" * 10))
    p = cli(["head-genome", str(tmp_path / "n.fa"), "-o", "-"], {"BSK_STREAM_PIECE_BYTES": "2000"})
    assert p.returncode != 0 and b"no description: c400" in p.stderr and p.stdout == b""
    p = cli(["head-genome", str(tmp_path / "n.fa"), "--devices", "0"])
    assert p.returncode != 0 and b"--devices" in p.stderr and b"one device" in p.stderr
    p = cli(["head-genome", "-m", "0", str(tmp_path / "n.fa")])
    assert p.returncode != 0 and b"value of flag --mini-common-words should be greater than 0" in p.stderr
