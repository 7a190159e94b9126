"""`shuffle` in buckets of the draw without a GPU (PARITY.md SHUF): the plan of buckets (bsk_shuffle_plan, a pure host function)
and the invariant the design rests on -- the per-bucket sorted restatements, concatenated, are the shuffle -- in plain Python
against tests/sample_ref.py."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import bigseqkit_amd as bsk
from bigseqkit_amd import _lib
from bigseqkit_amd._lib import lib
import sample_ref as R
import seqgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS = 4096


def plan(hist, budget):
    return bsk.ShufflePlan(hist, budget)


def check_plan(hist, budget):
    """ascending bounds that cover [0, 4096]; every bucket within the budget; greedy from the left: no bucket would also have
    taken the first non-empty bin behind it"""
    bounds = plan(hist, budget)
    assert bounds[0] == 0 and bounds[-1] == BINS
    assert all(a < b for a, b in zip(bounds[:-1], bounds[1:]))
    sums = [sum(hist[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]
    assert sum(sums) == sum(hist)
    assert all(s <= budget for s in sums), (budget, max(sums))
    for k in range(len(sums) - 1):
        assert sums[k] + sums[k + 1] > budget, (k, sums[k], sums[k + 1], budget)           # neighbours do not fit together
        assert hist[bounds[k + 1]] > 0 and sums[k] + hist[bounds[k + 1]] > budget, k        # a bucket ends only when it must
    assert plan(hist, budget) == bounds                                                     # the same input, the same plan
    return bounds


def test_hand_made_histograms():
    h = [0] * BINS
    assert check_plan(h, 1) == [0, BINS]                      # all empty: one bucket
    assert check_plan(h, 0) == [0, BINS]
    h[5] = 10
    assert check_plan(h, 10) == [0, BINS]                     # one bin that just fits; the empty bins join it
    h[6], h[7], h[4095] = 10, 1, 3
    assert check_plan(h, 10) == [0, 6, 7, BINS]               # 10 | 10 | 1 + 3
    assert check_plan(h, 11) == [0, 6, 4095, BINS]            # 10 | 10 + 1 | 3
    assert check_plan(h, 20) == [0, 7, BINS]
    assert check_plan(h, 24) == [0, BINS]
    full = [7] * BINS
    assert check_plan(full, 7) == list(range(BINS + 1))       # every bin a bucket of its own
    assert check_plan(full, 13) == list(range(BINS + 1))
    assert check_plan(full, 14) == list(range(0, BINS + 1, 2))
    assert check_plan(full, 7 * BINS) == [0, BINS]


@pytest.mark.parametrize("seed", range(6))
def test_random_histograms(seed):
    rng = random.Random(seed)
    density = rng.choice((0.01, 0.3, 1.0))
    hist = [rng.randint(1, 1 << rng.randint(1, 40)) if rng.random() < density else 0 for _ in range(BINS)]
    top = max(hist)
    for budget in (top, top + 1, 2 * top, sum(hist) // 5 + top, sum(hist), (1 << 64) - 1):
        bounds = check_plan(hist, budget)
        if budget >= sum(hist):
            assert bounds == [0, BINS]


def test_a_fine_bin_above_the_budget_is_refused():
    h = [0] * BINS
    h[100], h[2000] = 50, 12345
    with pytest.raises(bsk.BskError) as e:
        plan(h, 12344)
    assert e.value.code == _lib.BSK_ERR_UNSUPPORTED
    assert "12345" in str(e.value) and "12344" in str(e.value) and "2000" in str(e.value)
    assert plan(h, 12345) == [0, 2000, BINS]
    # null arguments are refused, not dereferenced
    assert lib.bsk_shuffle_plan(None, 1, None, None) == _lib.BSK_ERR_INVALID_ARG


def test_the_plan_needs_no_device():
    """a context made for its options alone (device = -1) exists next to it; the plan itself takes no context"""
    with bsk.Operator("Shuffle", "{}", -1):
        h = (C.c_uint64 * BINS)(*([3] * BINS))
        bounds = (C.c_uint64 * (BINS + 1))()
        nb = C.c_int()
        assert lib.bsk_shuffle_plan(h, 3 * 1024, bounds, C.byref(nb)) == 0
        assert nb.value == 4 and list(bounds[:5]) == [0, 1024, 2048, 3072, 4096]


def test_buckets_compose_to_the_shuffle():
    """the invariant without a device: for any cut of the draw range into consecutive intervals, the records of interval 0 in
    ascending order of their draws, then those of interval 1, ... are the shuffle"""
    data = seqgen.random_fastq(random.Random(9), 500, 1, 60)
    recs = R.records(data, True)
    assert len(recs) == 500
    for seed in (23, 0, -1, (1 << 63) - 1):
        want = R.shuffle(data, True, seed)
        draws = [R.draw(seed, g) for g in range(len(recs))]
        assert len(set(draws)) == len(draws)
        for nb in range(1, 51):
            # nb intervals of the 4096 fine bins, as even as integers allow
            bounds = [BINS * k // nb for k in range(nb + 1)]
            got = []
            for lo, hi in zip(bounds[:-1], bounds[1:]):
                inside = [g for g in range(len(recs)) if lo <= (draws[g] >> 52) < hi]
                got += [recs[g] + b"\n" for g in sorted(inside, key=draws.__getitem__)]
            assert b"".join(got) == want, (seed, nb)


HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_use_no_scratch(tmp_path):
    """the compiler's resource report for gfx950: no scratch and no spill in any kernel of `sample` / `shuffle`; the 48 KiB of LDS
    are the histogram's alone"""
    src = os.path.join(ROOT, "bigseqkit_amd", "csrc", "ops_sample.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", str(tmp_path / "o.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want = ("k_sample_size", "k_shuffle_keys", "k_shuffle_segments", "k_shuffle_fix", "k_shuffle_hist", "k_shuffle_append")
    assert sorted(re.findall(r"void (k_\w+)\(", open(src).read())) == sorted(want)          # every kernel of the file
    seen = {}
    for b in r.stderr.split("Function Name: ")[1:]:
        sym = b.split(" ", 1)[0]
        for k in want:
            if k in sym:
                seen[k] = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
                assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, sym
                assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, sym
    assert sorted(seen) == sorted(want), seen
    assert seen.pop("k_shuffle_hist") == 4096 * (8 + 4) and set(seen.values()) == {0}
