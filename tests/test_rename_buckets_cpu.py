"""`rename` in buckets of the key without a GPU (PARITY.md RENB): the restated `rename` is the oracle's; the composition the
design rests on -- the ordinals inside every interval of fine bins, put back by global index, are the ordinals of the whole
input -- in plain Python with the reference's XXH64 and the plan of bsk_shuffle_plan; the preconditions of the GPU tests'
inputs; and the compiler's resource report for the kernels."""
import json
import os
import random
import re
import subprocess

import pytest

import bigseqkit_amd as bsk
import oracle
import rename_buckets_ref as N
import rmdup_buckets_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
IDS = lambda o: "+".join(o) or "id"
RENAME_BUCKETS = bsk.RenameBuckets   # what this file restates: without the bucket path of `rename` there is nothing to restate


@pytest.mark.parametrize("name", R.SHAPES)
@pytest.mark.parametrize("o", N.OPTION_SETS, ids=IDS)
def test_restated_rename_is_the_oracles(name, o):
    oj = json.dumps(o)
    data, fastq = R.shape(name)
    recs, subs, hb, hr, ords = N.restated(name, oj)
    assert len(recs) == 500 == sum(hr)
    assert R.parse(N.want_of(name, oj), fastq) == N.py_rename(recs, o)
    assert 73 <= sum(1 for k in ords if k) <= 178                        # between a seventh and a third of the records are renamed
    assert 5 <= max(ords) <= 19                                          # suffixes of one digit; some shapes reach two


def test_two_digit_suffixes_occur():
    assert max(max(N.restated(name, json.dumps(o))[4]) for name in R.SHAPES for o in N.OPTION_SETS) >= 10


def ordinals_by_intervals(subs, bounds):
    """the ordinals computed inside every interval of bins on its own, put back by global index"""
    ords = [None] * len(subs)
    bins = [R.bin_of(s) for s in subs]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        idx = [g for g, b in enumerate(bins) if lo <= b < hi]
        for g, k in zip(idx, N.py_ordinals([subs[g] for g in idx])):
            assert ords[g] is None                                       # a global index belongs to one bucket only
            ords[g] = k
    return ords


@pytest.mark.parametrize("name", R.SHAPES)
@pytest.mark.parametrize("o", N.OPTION_SETS, ids=IDS)
def test_ordinals_of_the_intervals_are_the_ordinals_of_the_input(name, o):
    recs, subs, hb, hr, ords = N.restated(name, json.dumps(o))
    rng = random.Random(5)
    plans = [bsk.ShufflePlan(hb, b) for b in R.budgets_of(hb)]
    plans += [[0] + sorted(rng.sample(range(1, R.BINS), k - 1)) + [R.BINS] for k in range(1, 51)]
    for bounds in plans:
        assert bounds[0] == 0 and bounds[-1] == R.BINS
        assert ordinals_by_intervals(subs, bounds) == ords, len(bounds) - 1


@pytest.mark.parametrize("name", R.SHAPES)
def test_inputs_meet_the_preconditions_of_the_gpu_tests(name):
    data, fastq = R.shape(name)
    spans = oracle.record_spans(data, fastq)
    assert len(spans) == 500
    for o in N.OPTION_SETS:
        recs, subs, hb, hr, ords = N.restated(name, json.dumps(o))
        one, eight, fullest = R.budgets_of(hb)
        assert len(bsk.ShufflePlan(hb, one)) - 1 == 1
        assert eight >= max(hb) and len(bsk.ShufflePlan(hb, eight)) - 1 >= 8   # the 8-bucket budget admits the largest bin
        assert len(bsk.ShufflePlan(hb, fullest)) - 1 >= 8
        with pytest.raises(bsk.BskError):
            bsk.ShufflePlan(hb, fullest - 1)
        for parts in (3, 7):
            cuts = R.cuts_of(data, fastq, parts)
            assert len(cuts) == parts + 1 and cuts == sorted(cuts)
            starts = [s for s, _ in spans]
            shard_of = [max(k for k, c in enumerate(cuts[:-1]) if c <= s and s < cuts[k + 1]) for s in starts]
            first_seen = {}
            spanning = sum(1 for g, s in enumerate(subs) if shard_of[first_seen.setdefault(s, g)] != shard_of[g])
            assert spanning >= 1                                          # a group spans two shards
            assert subs[-1] == subs[0] and ords[-1] >= 1 and shard_of[0] == 0 and shard_of[-1] == max(shard_of)
            if parts == 7:
                assert cuts[3] == cuts[4] and shard_of.count(0) == 1     # an empty shard, a one-record shard


def test_masked_key_input_exercises_the_flagged_ordinals():
    """under 16 bits of the key some IDs share a key group: records are flagged, a flagged text comes two and three times (its
    ordinals 1 and 2 come from the host), and in some group the first text and an intruding text are BOTH repeated -- the
    interleaved case A B A B -> A B A_1 B_1"""
    data = N.masked_key_input()
    subs = [R.subject(r, {}) for r in R.parse(data, True)]
    assert len(subs) == 3600
    flagged, twice, thrice, both = N.masked_groups(subs)
    assert (flagged, twice, thrice, both) == (88, 10, 1, 3)
    assert flagged >= 1 and twice >= 1 and thrice >= 1 and both >= 1
    assert N.masked_groups(subs, 64)[0] == 0                              # whole keys: nothing is flagged


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_use_no_scratch(tmp_path):
    """the compiler's resource report for gfx950: no scratch and no spilled register in any kernel of the file.  The comparison
    kernel holds one word per record of its block (256 / 8 = 32), the block's member count, and behind them, on its own 8-byte
    boundary, the block's base in the member list: 32 * 4 + 4 = 132, padded to 136, + 8 = 144 bytes; nothing else uses LDS"""
    src = os.path.join(ROOT, "bigseqkit_amd", "csrc", "ops_rename_buckets.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", str(tmp_path / "o.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want = ("k_renb_verify", "k_renb_scatter", "k_renb_set")
    assert sorted(re.findall(r"void (k_\w+)\(", open(src).read())) == sorted(want)          # every kernel of the file
    seen = {}
    for b in r.stderr.split("Function Name: ")[1:]:
        sym = b.split(" ", 1)[0]
        for k in want:
            if re.search(r"\d" + k + "E", sym):
                seen[k] = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
                assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, sym
                assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0 and int(re.search(r"SGPRs Spill: (\d+)", b).group(1)) == 0, sym
    assert sorted(seen) == sorted(want), seen
    assert seen["k_renb_verify"] == (256 // 8 + 1) * 4 + 4 + 8
    assert seen["k_renb_scatter"] == 0 and seen["k_renb_set"] == 0
