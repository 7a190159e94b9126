"""`rmdup` in buckets of the key without a GPU (PARITY.md RMDUPB): the composition the design rests on -- the survivors of every
interval of fine bins, joined in file order, are the survivors of the whole input -- restated in plain Python with the
reference's XXH64 and the plan of bsk_shuffle_plan; the preconditions of the GPU tests' inputs; and the compiler's resource
report for the kernels."""
import json
import os
import random
import re
import subprocess

import pytest

import bigseqkit_amd as bsk
import oracle
import rmdup_buckets_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def survivors_by_intervals(subs, bounds):
    """the records with no earlier equal subject among the records of their own interval of bins"""
    keep = [False] * len(subs)
    bins = [R.bin_of(s) for s in subs]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        seen = set()
        for g, (s, b) in enumerate(zip(subs, bins)):
            if lo <= b < hi:
                keep[g] = s not in seen
                seen.add(s)
    return keep


@pytest.mark.parametrize("name", R.SHAPES)
@pytest.mark.parametrize("o", R.OPTION_SETS, ids=lambda o: "+".join(o) or "id")
def test_survivors_of_the_intervals_are_the_survivors_of_the_input(name, o):
    oj = json.dumps(o)
    data, fastq = R.shape(name)
    recs, subs, hb, hr = R.restated(name, oj)
    assert len(recs) == 500 == sum(hr)
    verdict = R.py_verdict(subs)
    assert 50 <= sum(verdict) <= 250                                    # between a tenth and a half of the subjects repeat
    want = R.parse(R.want_of(name, oj), fastq)
    assert want == [r for r, v in zip(recs, verdict) if not v]           # the restated verdict is the oracle's
    rng = random.Random(5)
    plans = [bsk.ShufflePlan(hb, b) for b in R.budgets_of(hb)]
    plans += [[0] + sorted(rng.sample(range(1, R.BINS), k - 1)) + [R.BINS] for k in range(1, 51)]
    for bounds in plans:
        assert bounds[0] == 0 and bounds[-1] == R.BINS
        keep = survivors_by_intervals(subs, bounds)
        assert [r for r, k in zip(recs, keep) if k] == want, len(bounds) - 1


@pytest.mark.parametrize("name", R.SHAPES)
def test_inputs_meet_the_preconditions_of_the_gpu_tests(name):
    data, fastq = R.shape(name)
    spans = oracle.record_spans(data, fastq)
    assert len(spans) == 500
    for o in R.OPTION_SETS:
        recs, subs, hb, hr = R.restated(name, json.dumps(o))
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
            assert spanning >= 1                                          # a duplicate group spans two shards
            assert subs[-1] == subs[0] and shard_of[0] == 0 and shard_of[-1] == max(shard_of)   # survivor first, copy last
            if parts == 7:
                assert cuts[3] == cuts[4] and shard_of.count(0) == 1     # an empty shard, a one-record shard


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_use_no_scratch(tmp_path):
    """the compiler's resource report for gfx950: no scratch and no spilled register in any kernel of the file; the histogram's
    LDS (4096 x (8 + 4) bytes = 48 KiB) lets three blocks share the 160 KB of a CU, the comparison kernel holds one word per
    record of its block and a counter, nothing else uses LDS"""
    src = os.path.join(ROOT, "bigseqkit_amd", "csrc", "ops_rmdup_buckets.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", str(tmp_path / "o.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want = ("k_rdb_hist", "k_rdb_pick", "k_rdb_pack", "k_rdb_pack_long", "k_rdb_verify", "k_rdb_gather", "k_rdb_mark", "k_rdb_apply",
            "k_rdb_narrow")
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
    assert seen["k_rdb_hist"] == 4096 * 12 <= 160 * 1024 // 3
    assert seen["k_rdb_verify"] == (256 // 8 + 1) * 4
    assert all(v == 0 for k, v in seen.items() if k not in ("k_rdb_hist", "k_rdb_verify"))
