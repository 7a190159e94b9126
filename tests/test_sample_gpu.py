"""`sample` / `shuffle` on the GPU, byte for byte against tests/sample_ref.py (PARITY.md SAMPLE, SHUF): every input shape the
record readers know, both output contracts, the segmented copy on and off, any cut into shards, host and device shards, the
command line on one device, streamed in pieces and over several workers, and the refusals."""
import json
import os
import random
import subprocess

import pytest

import bigseqkit_amd as bsk
from bigseqkit_amd._lib import BskError
import oracle
import sample_ref as R
import seqgen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "sample_fixtures.json")))
CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")


def wrap(t, w):
    return "\n".join(t[i:i + w] for i in range(0, len(t), w))


def wrapped_fastq(rng, nrec, width):
    out = []
    for i in range(nrec):
        L = rng.randint(1, 90)
        s = "".join(rng.choice("ACGT") for _ in range(L))
        q = "".join(rng.choice("ABCDEFGHI") for _ in range(L))
        out.append("@w%d x\n%s\n+\n%s\n" % (i, wrap(s, width), wrap(q, width)))
    return "".join(out).encode()


def inputs():
    rng = random.Random(77)
    big = ">big one\n" + wrap("".join(rng.choice("ACGT") for _ in range((1 << 20) + 12345)), 70) + "\n"
    fa_headers = b">a >b\nACGT\n\nAC\n>c\n\n\n>d>e\nTTTT\nGG\n\n>f\nA\n"
    return [
        ("fasta", seqgen.random_fasta(rng, 300, 0, 400), False),
        ("fasta blank lines, > in headers", fa_headers * 40, False),
        ("fasta no final newline", seqgen.random_fasta(rng, 120, 1, 200, final_newline=False), False),
        ("fasta crlf", seqgen.random_fasta(rng, 80, 1, 150).replace(b"\n", b"\r\n"), False),
        ("fasta tiny records", b"".join(b">%d\nA\n" % i for i in range(700)), False),
        ("fasta with a record over a MiB", (seqgen.random_fasta(rng, 20, 1, 100) + big.encode() + seqgen.random_fasta(rng, 20, 1, 100)), False),
        ("fastq", seqgen.random_fastq(rng, 400, 0, 200), True),
        ("fastq no final newline", seqgen.random_fastq(rng, 150, 1, 100, final_newline=False), True),
        ("fastq crlf", seqgen.random_fastq(rng, 100, 1, 80).replace(b"\n", b"\r\n"), True),
        ("fastq tiny records", b"".join(b"@%d\nA\n+\nI\n" % i for i in range(900)), True),
        ("fastq wrapped", wrapped_fastq(rng, 250, 17), True),
        ("fastq trailing blank lines", seqgen.random_fastq(rng, 90, 1, 60, trailing_blank=3), True),
    ]


INPUTS = inputs()
IDS = [x[0] for x in INPUTS]


def frame(data, fastq, parts=1, device=False):
    """`data` as `parts` shards that begin on record starts (the oracle's: the cut does not hang on the library under test)"""
    f = (bsk.ReadFASTQN if fastq else bsk.ReadFASTAN)(data, 1)
    if parts > 1:
        starts = [s for s, _ in oracle.record_spans(data, fastq)]
        cuts = sorted({0, len(data)} | {starts[len(starts) * k // parts] for k in range(1, parts)}) if starts else [0, len(data)]
        f = bsk.SeqFrame(f.format, [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])])
    if device:
        import torch
        f = bsk.SeqFrame(f.format, [torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda() if len(s) else torch.empty(0, dtype=torch.uint8, device="cuda")
                                    for s in f.shards])
    return f


def gpu_sample(data, fastq, parts=1, device=False, **o):
    return bsk.Sample(frame(data, fastq, parts, device), bsk.SeqKitSampleOptions(**o))


def gpu_shuffle(data, fastq, parts=1, device=False, **o):
    return bsk.Shuffle(frame(data, fastq, parts, device), bsk.SeqKitShuffleOptions(**o))


@pytest.mark.parametrize("name,data,fastq", INPUTS, ids=IDS)
def test_sample_equals_the_restatement(name, data, fastq):
    n = len(R.records(data, fastq))
    for o in ({"proportion": 0.5}, {"proportion": 0.1, "seed": 23}, {"proportion": 1.0}, {"proportion": 1e-9}, {"proportion": 0.9, "seed": -5},
              {"number": max(1, n // 3)}, {"number": n}, {"number": 5 * n, "seed": 0}, {"number": max(1, n // 2), "proportion": 0.01},
              {"proportion": 0.3, "seed": (1 << 63) - 1}, {"proportion": 0.3, "seed": -(1 << 63)}, {"proportion": 0.3, "seed": 0x123456789ABCDEF}):
        want = R.sample(data, fastq, o.get("seed", 11), o.get("number", 0), o.get("proportion", 0.0))
        assert gpu_sample(data, fastq, **o) == want, (name, o)
    assert R.sample(data, fastq, 11, 0, 1.0) == b"".join(r + b"\n" for r in R.records(data, fastq))


@pytest.mark.parametrize("name,data,fastq", INPUTS, ids=IDS)
def test_shuffle_equals_the_restatement(name, data, fastq):
    recs = R.records(data, fastq)
    got = gpu_shuffle(data, fastq)
    assert got == R.shuffle(data, fastq, 23), name
    assert len(got) == sum(len(r) + 1 for r in recs)
    other = gpu_shuffle(data, fastq, seed=24)
    assert other == R.shuffle(data, fastq, 24) and other != got
    for seed in (-1, (1 << 63) - 1, -(1 << 63)):
        assert gpu_shuffle(data, fastq, seed=seed) == R.shuffle(data, fastq, seed), (name, seed)


def test_shuffle_is_a_permutation_of_the_records():
    rng = random.Random(3)
    for data, fastq in ((seqgen.random_fastq(rng, 500, 1, 100), True), (seqgen.random_fasta(rng, 500, 1, 100), False)):
        recs = R.records(data, fastq)
        got = R.records(gpu_shuffle(data, fastq), fastq)
        assert got != recs and sorted(got) == sorted(recs)
        assert got == [recs[g] for g in R.shuffle_order(23, len(recs))]


@pytest.mark.parametrize("case", range(len(FIX["cases"])))
def test_hand_fixtures(case):
    c = FIX["cases"][case]
    data, fastq = FIX["inputs"][c["name"]].encode(), c["format"] == "fastq"
    if c["command"] == "sample":
        got = bsk.Sample(frame(data, fastq), bsk.SeqKitSampleOptions().Seed(c["seed"]).Number(c["options"].get("Number", 0))
                         .Proportion(c["options"].get("Proportion", 0.0)))
    else:
        got = bsk.Shuffle(frame(data, fastq), bsk.SeqKitShuffleOptions().Seed(c["seed"]))
    assert got == c["want"].encode()


@pytest.mark.parametrize("fastq", [True, False])
def test_empty_and_single_record(fastq):
    one = b"@r\nACGT\n+\nIIII\n" if fastq else b">r d\nACGT\nAC\n"
    for data in (b"", one, one[:-1]):
        n = 1 if data else 0
        assert gpu_shuffle(data, fastq) == (one if data else b"")
        assert gpu_sample(data, fastq, proportion=1.0) == (one if data else b"")
        assert gpu_sample(data, fastq, number=3) == (one if data else b"")      # an empty input: no division error
        assert gpu_sample(data, fastq, proportion=1e-9) == R.sample(data, fastq, 11, 0, 1e-9) == b""
        assert gpu_sample(data, fastq, proportion=0.5, seed=4) == R.sample(data, fastq, 4, 0, 0.5)
        assert len(R.records(data, fastq)) == n


@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("fastq", [True, False])
def test_the_verdict_as_an_interval_of_the_draw(fastq, parts):
    """the kernel compares the draw with a closed interval in place of (draw >> 11) < T: T = 2^53 (all of [0, 2^64 - 1]), the
    smallest T there is (1: [0, 2047], from the smallest fraction the options accept) and one in between"""
    rng = random.Random(90 + fastq)
    data = seqgen.random_fastq(rng, 30, 1, 60) if fastq else seqgen.random_fasta(rng, 30, 1, 90)
    recs = R.records(data, fastq)
    assert len(recs) == 30
    assert gpu_sample(data, fastq, parts=parts, proportion=1.0) == b"".join(r + b"\n" for r in recs)
    tiny = 2.0 ** -149                       # the smallest positive float32: Proportion is one in the reference's options
    assert R.f32(tiny) == tiny and R.threshold(tiny) == 1 and R.f32(tiny / 2) == 0
    for p in (tiny, 0.5):
        for seed in (11, 23):
            assert gpu_sample(data, fastq, parts=parts, proportion=p, seed=seed) == R.sample(data, fastq, seed, 0, p), (p, seed)
    assert 0 < len(R.records(R.sample(data, fastq, 11, 0, 0.5), fastq)) < 30


@pytest.mark.parametrize("out", ["slices", "block"])
@pytest.mark.parametrize("segcopy", ["off", "force", None])
def test_output_contracts_and_copy_paths(out, segcopy, monkeypatch):
    if out == "slices":
        monkeypatch.setenv("BSK_OUT", "slices")
    if segcopy:
        monkeypatch.setenv("BSK_SEGCOPY", segcopy)
    for name, data, fastq in INPUTS:
        for o in ({"proportion": 0.4}, {"proportion": 1.0}, {"number": 7, "seed": 9}):
            assert gpu_sample(data, fastq, **o) == R.sample(data, fastq, o.get("seed", 11), o.get("number", 0), o.get("proportion", 0.0)), (name, o)
            assert gpu_sample(data, fastq, parts=3, device=True, **o) == \
                R.sample(data, fastq, o.get("seed", 11), o.get("number", 0), o.get("proportion", 0.0)), (name, o)
        assert gpu_shuffle(data, fastq) == R.shuffle(data, fastq), name


def test_slices_contract_returns_segments_and_materializes():
    """out = slices: the kept records come back as ordered slices of the shard; bsk_out_materialize makes the block"""
    import ctypes as C
    import torch
    from bigseqkit_amd._lib import Out, lib, check
    data = seqgen.random_fastq(random.Random(8), 600, 1, 150)
    want = R.sample(data, True, 11, 0, 0.5)
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    with bsk.Operator("Sample", '{"Proportion": 0.5}', 0) as op:
        check(lib.bsk_ctx_set(op.ctx, b"out", b"slices"), op.ctx)
        out = Out()
        check(lib.bsk_sample_run(op.ctx, C.c_void_p(t.data_ptr()), t.numel(), 1, bsk.FORMAT_FASTQ, 0, 0, None, C.byref(out)), op.ctx)
        assert out.n_segments == 600 and not out.d_data and out.len == len(want)
        check(lib.bsk_out_materialize(op.ctx, C.byref(out), None), op.ctx)
        assert out.n_segments == 0 and out.d_data
        buf = C.create_string_buffer(out.len)
        check(lib.bsk_out_to_host(op.ctx, C.byref(out), buf, out.len), op.ctx)
        assert buf.raw[:out.len] == want


@pytest.mark.parametrize("name,data,fastq", INPUTS, ids=IDS)
def test_the_same_bytes_for_any_number_of_shards(name, data, fastq):
    n = len(R.records(data, fastq))
    for o in ({"proportion": 0.5}, {"number": max(1, n // 4), "seed": 5}):
        want = R.sample(data, fastq, o.get("seed", 11), o.get("number", 0), o.get("proportion", 0.0))
        for parts in (1, 2, 3, 7):
            for device in (False, True):
                assert gpu_sample(data, fastq, parts=parts, device=device, **o) == want, (name, o, parts, device)
    # shuffle of several shards == shuffle of their concatenation
    want = R.shuffle(data, fastq)
    for parts in (2, 3, 7):
        for device in (False, True):
            assert gpu_shuffle(data, fastq, parts=parts, device=device) == want, (name, parts, device)


def test_paired_files_keep_the_same_mates():
    rng = random.Random(12)
    a, b = seqgen.random_fastq(rng, 700, 1, 120), seqgen.random_fastq(rng, 700, 1, 200)
    ra, rb = R.records(a, True), R.records(b, True)
    for o in ({"proportion": 0.3, "seed": 17}, {"number": 100, "seed": 17}):
        ka = R.records(gpu_sample(a, True, parts=2, **o), True)
        kb = R.records(gpu_sample(b, True, parts=5, **o), True)
        ia, ib = [ra.index(x) for x in ka], [rb.index(x) for x in kb]
        assert ia == ib and 0 < len(ia) < 700
    # ... and one seed shuffles both files alike
    sa, sb = R.records(gpu_shuffle(a, True, seed=17), True), R.records(gpu_shuffle(b, True, seed=17), True)
    assert [ra.index(x) for x in sa] == [rb.index(x) for x in sb]


def test_streamed_chunks_carry_the_record_index(tmp_path, monkeypatch):
    """bsk_run_to_store: the chunks of one call, and with pin_alphabet the calls that feed one partition, count on"""
    import ctypes as C
    from bigseqkit_amd._lib import lib, check
    monkeypatch.setenv("BSK_STAGE_BYTES", "5000")
    for fastq, data in ((True, seqgen.random_fastq(random.Random(5), 900, 1, 150)), (False, seqgen.random_fasta(random.Random(6), 500, 1, 300))):
        fmt = bsk.FORMAT_FASTQ if fastq else bsk.FORMAT_FASTA
        want = R.sample(data, fastq, 11, 0, 0.5)
        path = str(tmp_path / ("s%d" % fastq))
        with bsk.Operator("Sample", '{"Proportion": 0.5}', 0) as op:
            store = C.c_void_p()
            assert lib.bsk_store_open(path.encode(), 1, C.byref(store)) == 0
            nb, nr = C.c_uint64(), C.c_uint64()
            check(lib.bsk_run_to_store(op.ctx, data, len(data), fmt, 0, store, 0, C.byref(nb), C.byref(nr)), op.ctx)
            assert lib.bsk_store_close(store, None) == 0
        assert open(path, "rb").read() == want and nb.value == len(want)
        # a second partition that starts at record `first`
        recs = R.records(data, fastq)
        first = len(recs) // 3
        tail = b"".join(r + b"\n" for r in recs[first:])
        with bsk.Operator("Sample", '{"Proportion": 0.5}', 0) as op:
            store = C.c_void_p()
            assert lib.bsk_store_open(path.encode(), 1, C.byref(store)) == 0
            check(lib.bsk_sample_set_first_record(op.ctx, first), op.ctx)
            check(lib.bsk_run_to_store(op.ctx, tail, len(tail), fmt, 0, store, 0, None, None), op.ctx)
            assert lib.bsk_store_close(store, None) == 0
        assert open(path, "rb").read() == R.sample(tail, fastq, 11, 0, 0.5, first=first)


def test_number_needs_the_count_first():
    import ctypes as C
    from bigseqkit_amd._lib import Out, lib
    data = seqgen.random_fastq(random.Random(1), 20, 1, 50)
    with bsk.Operator("Sample", '{"Number": 5}', 0) as op:
        out = Out()
        assert lib.bsk_sample_run(op.ctx, data, len(data), 0, bsk.FORMAT_FASTQ, 0, 0, None, C.byref(out)) != 0
        assert "bsk_sample_set_count" in lib.bsk_last_error(op.ctx).decode()
    with bsk.Operator("Shuffle", "{}", 0) as op:
        out = Out()
        assert lib.bsk_sample_run(op.ctx, data, len(data), 0, bsk.FORMAT_FASTQ, 0, 0, None, C.byref(out)) != 0
        assert "not a Sample context" in lib.bsk_last_error(op.ctx).decode()


# ------------------------------------------------------------------ the command line
def cli(args, env=None, ok=True):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([CLI, *args], capture_output=True, timeout=900, env=e)
    if ok:
        assert p.returncode == 0, p.stderr.decode()
    return p


def read_dir(path):
    return b"".join(open(os.path.join(path, f), "rb").read() for f in sorted(os.listdir(path)))


STREAM = {"BSK_HOST_PIPELINE_FROM": "0", "BSK_STAGE_BYTES": "4096", "BSK_STREAM_PIECE_BYTES": "30000"}


@pytest.mark.parametrize("fastq", [True, False])
def test_cli_sample(tmp_path, fastq):
    rng = random.Random(40 + fastq)
    data = seqgen.random_fastq(rng, 2500, 1, 150) if fastq else seqgen.random_fasta(rng, 1500, 1, 400)
    src = str(tmp_path / ("in.fq" if fastq else "in.fa"))
    open(src, "wb").write(data)
    n = len(R.records(data, fastq))
    for flags, o in ((["-p", "0.25"], {"proportion": 0.25}), (["-n", str(n // 5), "-s", "99"], {"number": n // 5, "seed": 99}),
                     (["-p", "1", "-2"], {"proportion": 1.0})):
        want = R.sample(data, fastq, o.get("seed", 11), o.get("number", 0), o.get("proportion", 0.0))
        out = str(tmp_path / "one")
        cli(["sample", *flags, src, "-o", out, "--merge"])
        assert open(out, "rb").read() == want, flags
        assert cli(["sample", *flags, src, "-o", "-"]).stdout == want
        for devices in ("0", "0,0", "0,0,0"):
            out = str(tmp_path / ("dev" + devices.replace(",", "_")))
            cli(["sample", *flags, src, "--devices", devices, "-o", out, "--merge"], {"BSK_RUN_SHARE_GPU": "1"})
            assert open(out, "rb").read() == want, (flags, devices)
        out = str(tmp_path / "parts")
        cli(["sample", *flags, src, "--devices", "0,0,0", "-o", out], {"BSK_RUN_SHARE_GPU": "1"})
        assert read_dir(out) == want and len(os.listdir(out)) == 3
        if "-n" in flags:
            p = cli(["sample", *flags, src, "--devices", "0", "-o", str(tmp_path / "x"), "--merge"], STREAM, ok=False)
            assert p.returncode == 1 and "-p (--proportion)" in p.stderr.decode() and "streamed" in p.stderr.decode()
        else:
            out = str(tmp_path / "streamed")
            cli(["sample", *flags, src, "--devices", "0", "-o", out, "--merge"], STREAM)
            assert open(out, "rb").read() == want, flags


def test_cli_shuffle_and_refusals(tmp_path):
    rng = random.Random(50)
    a, b = seqgen.random_fastq(rng, 800, 1, 150), seqgen.random_fastq(rng, 300, 1, 90, final_newline=False)
    fa, fb = str(tmp_path / "a.fq"), str(tmp_path / "b.fq")
    open(fa, "wb").write(a)
    open(fb, "wb").write(b)
    out = str(tmp_path / "o")
    cli(["shuffle", fa, "-o", out, "--merge"])
    assert open(out, "rb").read() == R.shuffle(a, True, 23)
    cli(["shuffle", "-s", "24", "-2", "-k", fb, fa, "-o", out, "--merge"])       # the files are unioned, the order is over both
    assert open(out, "rb").read() == R.shuffle(b + b"\n" + a, True, 24)
    p = cli(["shuffle", fa, "--devices", "0,0", "-o", out], ok=False)
    assert p.returncode == 1 and "'shuffle' runs on one device" in p.stderr.decode()
    p = cli(["sample", "-p", "0.5", fa, fb, "-o", out], ok=False)
    assert p.returncode == 1 and "only 1 file needed" in p.stderr.decode()
    p = cli(["sample", fa, "-o", out], ok=False)
    assert p.returncode == 1 and "one of flags -n (--number) and -p (--proportion) needed" in p.stderr.decode()
    p = cli(["sample", "-p", "1.5", fa, "-o", out], ok=False)
    assert p.returncode == 1 and "value of -p (--proportion) (1.500000) should be in range of (0, 1]" in p.stderr.decode()


def test_cli_pipe_takes_one_part_and_refuses_two(tmp_path):
    """cli/sample.go:11-13 counts the dataframes a `pipe` job hands over too: one part is sampled from record 0, two are refused
    (an error, never the parts judged each from its own record 0)"""
    rng = random.Random(60)
    a, b = seqgen.random_fastq(rng, 400, 1, 100), seqgen.random_fastq(rng, 300, 1, 100)
    fa, fb = str(tmp_path / "a.fq"), str(tmp_path / "b.fq")
    open(fa, "wb").write(a)
    open(fb, "wb").write(b)
    jf = tmp_path / "job.json"
    up = oracle.duplicate(a, True, '{"Times": 2}')   # what the upstream job hands over
    for flags, o in ((["-p", "0.4"], {"proportion": 0.4}), (["-n", "90", "-s", "5"], {"number": 90, "seed": 5})):
        jf.write_text(json.dumps({"pipe": [{"cmd": ["dup", "-n", "2", fa]}], "cmd": ["sample", *flags]}))
        got = cli(["pipe", "--job", str(jf), "-o", "-"]).stdout
        assert got == R.sample(up, True, o.get("seed", 11), o.get("number", 0), o.get("proportion", 0.0)), flags
        for job in ({"pipe": [{"cmd": ["dup", "-n", "2", fa]}, {"cmd": ["seq", fb]}], "cmd": ["sample", *flags]},
                    {"pipe": [{"cmd": ["seq", fa]}], "cmd": ["sample", *flags, fb]}):
            jf.write_text(json.dumps(job))
            p = cli(["pipe", "--job", str(jf), "-o", "-"], ok=False)
            assert p.returncode == 1 and "only 1 file needed" in p.stderr.decode() and p.stdout == b"", job


def test_cli_refusals_of_inputs_that_do_not_fit(tmp_path):
    data = seqgen.random_fastq(random.Random(61), 900, 1, 150)
    src = str(tmp_path / "in.fq")
    open(src, "wb").write(data)
    out = str(tmp_path / "o")
    # several workers whose shards are streamed from the file: the prefix of a worker needs the counts of the shards before it
    p = cli(["sample", "-p", "0.5", src, "--devices", "0,0", "-o", out, "--merge"], dict(STREAM, BSK_RUN_SHARE_GPU="1"), ok=False)
    assert p.returncode == 1 and "is not counted first" in p.stderr.decode() and "one worker" in p.stderr.decode()
    # shuffle of an input that does not fit the device: refused, and not sent to --devices
    p = cli(["shuffle", src, "-o", out, "--merge"], {"BSK_SHARD_FAIL_ALLOC": "1"}, ok=False)
    assert p.returncode == 1 and "must fit one GPU" in p.stderr.decode() and "runs on one device" in p.stderr.decode()
    assert "--devices" not in p.stderr.decode()
    p = cli(["sample", "-p", "0.5", src, "-o", out, "--merge"], {"BSK_SHARD_FAIL_ALLOC": "1"}, ok=False)
    assert p.returncode == 1 and "must fit one GPU" in p.stderr.decode() and "sample" in p.stderr.decode().split("--devices 0-7:")[1]


def test_a_refused_call_does_not_move_the_record_index():
    """a call that is refused before it owns the context (here: a bad format) leaves the running index where it was"""
    import ctypes as C
    from bigseqkit_amd._lib import Out, lib, check
    data = seqgen.random_fastq(random.Random(62), 300, 1, 80)
    recs = R.records(data, True)
    tail = b"".join(r + b"\n" for r in recs[100:])
    with bsk.Operator("Sample", '{"Proportion": 0.5}', 0) as op:
        out = Out()
        check(lib.bsk_sample_set_first_record(op.ctx, 100), op.ctx)
        assert lib.bsk_sample_run(op.ctx, tail, len(tail), 0, 99, 0, 7, None, C.byref(out)) != 0   # bad format: refused
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            store = C.c_void_p()
            path = os.path.join(d, "o")
            assert lib.bsk_store_open(path.encode(), 1, C.byref(store)) == 0
            check(lib.bsk_run_to_store(op.ctx, tail, len(tail), bsk.FORMAT_FASTQ, 0, store, 0, None, None), op.ctx)
            assert lib.bsk_store_close(store, None) == 0
            assert open(path, "rb").read() == R.sample(tail, True, 11, 0, 0.5, first=100)
