"""`sample` / `shuffle` without a GPU: the draw and its pinned values, the conditions the definition has to meet as a random
stream, the driver arithmetic and its messages (bsk_create on a context without a device), the flag tables of the command
line, and the hand-written eight-record fixtures (tests/golden/sample_fixtures.json) against tests/sample_ref.py."""
import ctypes as C
import functools
import json
import math
import os
import random
import subprocess

import pytest

import bigseqkit_amd as bsk
import oracle
import sample_ref as R
import seqgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "sample_fixtures.json")))
CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")
N = 10 ** 6
SEEDS = (11, 23, 0, -1, 12345)


@functools.lru_cache(maxsize=None)
def draws(seed):
    return [R.draw(seed, g) for g in range(N)]


def test_pinned_draws():
    assert len(FIX["pinned"]) == 20
    for p in FIX["pinned"]:
        assert R.draw(p["seed"], int(p["g"])) == int(p["draw"], 16), p
    for seed, row in FIX["first8"].items():
        assert [R.draw(int(seed), g) for g in range(8)] == [int(x, 16) for x in row]
    # the seed enters as (uint64)(int64)seed
    assert R.draw(-1, 5) == R.draw((1 << 64) - 1, 5) and R.draw(-1, 5) != R.draw(1, 5)


@pytest.mark.parametrize("seed", SEEDS)
def test_draws_are_distinct(seed):
    assert len(set(draws(seed))) == N


@pytest.mark.parametrize("seed", SEEDS)
def test_kept_count_is_binomial(seed):
    """Each verdict is a Bernoulli(f) trial if the draw is uniform: the kept count of N records lies within 5 sigma of f N,
    sigma = sqrt(N f (1 - f)) -- a condition on the definition (chance of a miss by a true random stream: 6e-7 per case)."""
    for p in (0.1, 0.5, 0.003):
        f = R.f32(p)
        T = R.threshold(f)
        kept = sum(1 for d in draws(seed) if (d >> 11) < T)
        sigma = math.sqrt(N * f * (1 - f))
        print("seed %d f %.9f kept %d: %+.2f sigma" % (seed, f, kept, (kept - f * N) / sigma))
        assert abs(kept - f * N) <= 5 * sigma, (seed, p, kept)


@pytest.mark.parametrize("seed", SEEDS)
def test_shuffle_order_looks_like_a_random_permutation(seed):
    """Of a uniform random permutation of N the fixed points are Poisson(1) and the ascents (perm[j] < perm[j + 1]) have mean
    (N - 1) / 2 and variance (N + 1) / 12.  The order is a fixed function of these inputs; evaluated on the CPU it has 0-2
    fixed points and an ascent count within 1.5 sigma of the mean for each of the five seeds: those figures are held."""
    d = draws(seed)
    order = sorted(range(N), key=d.__getitem__)
    if seed == 11:
        assert order == R.shuffle_order(seed, N)
    fixed = sum(1 for j, g in enumerate(order) if j == g)
    asc = sum(1 for j in range(N - 1) if order[j] < order[j + 1])
    sigma = math.sqrt((N + 1) / 12)
    print("seed %d: %d fixed points, ascents %+.2f sigma" % (seed, fixed, (asc - (N - 1) / 2) / sigma))
    assert fixed <= 2
    assert abs(asc - (N - 1) / 2) <= 1.5 * sigma


def test_threshold_rule():
    assert R.threshold(1.0) == 1 << 53 and R.threshold(math.inf) == 1 << 53 and R.threshold(0.0) == 0
    assert R.threshold(0.5) == 1 << 52 and R.threshold(2.0 ** -53) == 1 and R.threshold(2.0 ** -60) == 1
    # Proportion is a float32: 0.1 becomes 0.100000001490116...
    assert R.f32(0.1) == 0.10000000149011612 and R.threshold(R.f32(0.1)) == math.ceil(13421773 * 2 ** 26)
    assert R.fraction(0, 0.1) == R.f32(0.1) and R.fraction(3, 0.9, 12) == 0.25  # Number wins
    assert R.fraction(5, 0.0, 0) == math.inf                                    # an empty input is no division error
    # everything is kept at fraction >= 1, nothing the draw could do about it
    assert R.kept_indices(7, 100, R.threshold(1.0)) == list(range(100))


ERRORS = [({}, "one of flags -n (--number) and -p (--proportion) needed"),
          ({"Number": 0, "Proportion": 0.0}, "one of flags -n (--number) and -p (--proportion) needed"),
          ({"Number": -1}, "value of -n (--number) and should be greater than 0"),
          ({"Number": -1, "Proportion": 2.0}, "value of -n (--number) and should be greater than 0"),
          ({"Proportion": 1.5}, "value of -p (--proportion) (1.500000) should be in range of (0, 1]"),
          ({"Proportion": -0.1}, "value of -p (--proportion) (-0.100000) should be in range of (0, 1]"),
          ({"Number": 4, "Proportion": 1.0000001}, "value of -p (--proportion) (1.000000) should be in range of (0, 1]")]


@pytest.mark.parametrize("opts,msg", ERRORS)
def test_option_errors_have_the_reference_texts(opts, msg):
    with pytest.raises(bsk.BskError) as e:
        bsk.Operator("Sample", json.dumps(opts), -1)
    assert msg in str(e.value)
    with pytest.raises(R.SampleError) as e2:
        R.fraction(opts.get("Number", 0), opts.get("Proportion", 0.0), 10)
    assert str(e2.value) == msg


def test_options_defaults_and_count_protocol():
    with bsk.Operator("Sample", '{"Proportion": 0.25}', -1) as op:
        js = json.loads(op.opts_json())
        assert js["Seed"] == 11 and js["Number"] == 0 and js["Proportion"] == 0.25
        needs = C.c_int(7)
        assert bsk.lib.bsk_sample_needs_count(op.ctx, C.byref(needs)) == 0 and needs.value == 0
    with bsk.Operator("Sample", '{"Number": 5, "Proportion": 0.25, "Seed": -9223372036854775808}', -1) as op:
        assert json.loads(op.opts_json())["Seed"] == -(1 << 63)
        needs = C.c_int()
        assert bsk.lib.bsk_sample_needs_count(op.ctx, C.byref(needs)) == 0 and needs.value == 1
        assert bsk.lib.bsk_sample_set_count(op.ctx, 0) == 0  # an empty input: no division error
        assert bsk.lib.bsk_sample_needs_count(op.ctx, C.byref(needs)) == 0 and needs.value == 0
    with bsk.Operator("Shuffle", "{}", -1) as op:
        assert json.loads(op.opts_json())["Seed"] == 23
        assert bsk.lib.bsk_sample_needs_count(op.ctx, C.byref(needs)) != 0  # not a Sample context
    assert json.loads(bsk.SeqKitSampleOptions().Seed(3).Number(10).Proportion(0.5).to_json()) == {
        "Config": bsk.SeqKitConfig().to_dict(), "Seed": 3, "Number": 10, "Proportion": 0.5}
    assert json.loads(bsk.SeqKitShuffleOptions(seed=5).to_json())["Seed"] == 5


def dry(*args):
    p = subprocess.run([CLI, *args, "--dry-run"], capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()
    out = p.stdout.decode().split("\n")
    return out[0], json.loads(out[1]), [f for f in out[2:] if f]


def test_command_line_flag_tables():
    op, js, files = dry("sample", "x.fq")                                  # bigseqkit-cli/sample.go:43-46
    assert op == "Sample" and files == ["x.fq"] and (js["Seed"], js["Number"], js["Proportion"]) == (11, 0, 0)
    op, js, _ = dry("sample", "-s", "-7", "-n", "100", "-p", "0.3", "-2", "x.fq")
    assert (js["Seed"], js["Number"], js["Proportion"]) == (-7, 100, 0.3) and "TwoPass" not in js
    op, js, _ = dry("sample", "--rand-seed=9223372036854775807", "--number=5", "--proportion=1", "--two-pass")
    assert (js["Seed"], js["Number"], js["Proportion"]) == ((1 << 63) - 1, 5, 1)
    op, js, files = dry("shuffle", "a.fa", "b.fa")                         # bigseqkit-cli/shuffle.go:44-46
    assert op == "Shuffle" and js["Seed"] == 23 and files == ["a.fa", "b.fa"] and set(js) == {"Config", "Seed"}
    assert dry("shuffle", "-s", "24", "-2k", "a.fa")[1]["Seed"] == 24
    assert dry("shuffle", "--keep-temp", "--two-pass", "--rand-seed", "-1")[1]["Seed"] == -1
    for args, msg in ((("sample", "-p", "x"), 'invalid argument "x" for "--proportion" flag'),
                      (("sample", "-n", "1.5"), 'invalid argument "1.5" for "--number" flag'),
                      (("shuffle", "-n", "3"), "unknown shorthand flag: 'n' in -n")):
        p = subprocess.run([CLI, *args, "--dry-run"], capture_output=True, timeout=600)
        assert p.returncode == 1 and msg in p.stderr.decode(), (args, p.stderr)
    # cli/sample.go:11-13, before anything is read; shuffle runs on one device
    p = subprocess.run([CLI, "sample", "-p", "0.5", "a.fq", "b.fq"], capture_output=True, timeout=600)
    assert p.returncode == 1 and "only 1 file needed" in p.stderr.decode()
    p = subprocess.run([CLI, "shuffle", "a.fq", "--devices", "0,0"], capture_output=True, timeout=600)
    assert p.returncode == 1 and "'shuffle' runs on one device" in p.stderr.decode()


@pytest.mark.parametrize("case", range(len(FIX["cases"])))
def test_hand_fixtures(case):
    c = FIX["cases"][case]
    data, fastq = FIX["inputs"][c["name"]].encode(), c["format"] == "fastq"
    recs = R.records(data, fastq)
    assert len(recs) == 8
    row = [int(x, 16) for x in FIX["first8"].get(str(c["seed"]), [])]
    if c["command"] == "sample":
        o = c["options"]
        frac = o["Number"] / 8 if "Number" in o else R.f32(o["Proportion"])
        if row:  # the kept set follows from the pinned draws
            assert [g for g in range(8) if (row[g] >> 11) < R.threshold(frac)] == c["kept"]
        got = R.sample(data, fastq, c["seed"], o.get("Number", 0), o.get("Proportion", 0.0))
    else:
        if row:
            assert sorted(range(8), key=row.__getitem__) == c["order"]
        assert R.shuffle_order(c["seed"], 8) == c["order"]
        got = R.shuffle(data, fastq, c["seed"])
    assert got == c["want"].encode()


def test_record_texts_are_the_elements_range_and_duplicate_print():
    rng = random.Random(5)
    wrap = lambda t, w: "\n".join(t[i:i + w] for i in range(0, len(t), w))
    wrapped = "".join("@w%d\n%s\n+\n%s\n" % (i, wrap("ACGT" * (3 + i), 5), wrap("IIHG" * (3 + i), 7)) for i in range(9)).encode()
    for data, fastq in ((seqgen.random_fasta(rng, 60, 0, 200), False), (seqgen.random_fasta(rng, 40, 0, 90, final_newline=False), False),
                        (seqgen.random_fastq(rng, 60, 0, 120), True), (seqgen.random_fastq(rng, 30, 1, 50, final_newline=False), True),
                        (wrapped, True), (FIX["inputs"]["fasta8"].encode(), False)):
        recs = R.records(data, fastq)
        assert len(recs) == oracle.count_records(data, fastq)
        assert b"".join(r + b"\n" for r in recs) == oracle.duplicate(data, fastq, '{"Times": 1}')
        assert R.sample(data, fastq, proportion=1.0) == oracle.duplicate(data, fastq, '{"Times": 1}')
        k = len(recs) // 2
        assert recs[k] + b"\n" == oracle.range_(data, fastq, json.dumps({"Range": "%d:%d" % (k + 1, k + 1)}))
        assert sorted(R.records(R.shuffle(data, fastq), fastq)) == sorted(recs)
