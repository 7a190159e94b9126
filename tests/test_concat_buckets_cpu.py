"""`concat` in buckets of the key without a GPU (PARITY.md CONB): the two compositions the design rests on -- the heads decided
inside every interval of fine bins, put back by global index, are the heads of the whole input, and the oracle's `concat` on the
accumulation of every window of any cut of the window bins, joined and followed by the tail, is the oracle's `concat` on the whole
files -- in plain Python with the reference's XXH64 and the plan of bsk_shuffle_plan; that a collected record of file 2 has a mate
in its window; that the cost of a window bounds the bytes of its accumulation; and the compiler's resource report for the
kernels."""
import json
import os
import random
import re
import subprocess

import pytest

import bigseqkit_amd as bsk
import concat_buckets_ref as K
import oracle
import pair_buckets_ref as P
import rmdup_buckets_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CONCAT_BUCKETS = bsk.ConcatBuckets   # what this file restates: without the bucket path of `concat` there is nothing to restate


def three_cuts(hb, seed):
    """three different cuts of 4096 bins: one interval, the plan for about eight parts, a random cut into five"""
    rng = random.Random(seed)
    cuts = [[0, R.BINS], bsk.ShufflePlan(hb, K.budget_of(hb, 1 / 8)), [0] + sorted(rng.sample(range(1, R.BINS), 4)) + [R.BINS]]
    assert len({tuple(c) for c in cuts}) == 3
    return cuts


@pytest.mark.parametrize("full", (False, True), ids=("joined only", "full"))
@pytest.mark.parametrize("variant", P.VARIANTS)
@pytest.mark.parametrize("name", R.SHAPES)
def test_windows_joined_are_the_concat_of_the_files(name, variant, full):
    texts, fastq = P.files_text(name, variant)
    r = K.restated(name, variant)
    subs1, subs2 = r["subs"]
    n1 = len(subs1)
    oj = json.dumps({"Full": full})
    want = K.want_of(name, variant, oj)
    assert want and (full or len(want) < len(K.want_of(name, variant, json.dumps({"Full": True}))))
    for bounds in three_cuts(r["hist"][0], 1):
        assert bounds[0] == 0 and bounds[-1] == R.BINS
        assert K.heads_by_intervals(subs1, subs2, bounds) == r["head"], len(bounds) - 1
    whb = r["whist"][0]
    assert sum(r["whist"][1]) == n1 and K.window_shift(n1) == 0
    t1, t2 = r["costs"]
    for wbounds in three_cuts(whb, 2):
        got, sizes = K.concat_by_windows(texts, fastq, r["head"], wbounds, oj)
        assert got == want, len(wbounds) - 1
        assert sum(a for a, _ in sizes) == n1
        # the cost of a window bounds the bytes of its accumulation
        for lo, hi in zip(wbounds[:-1], wbounds[1:]):
            a, b = K.window_members(r["head"], n1, lo, hi)
            assert sum(whb[lo:hi]) >= sum(t1[i] for i in a) + sum(t2[j] for j in b)
    # the inputs: an ID of several records in file 1 whose mates land in more than one window of the eight-part plan
    plan = bsk.ShufflePlan(whb, K.budget_of(whb, 1 / 8))
    assert len(plan) - 1 >= 3
    picked = [set(K.window_members(r["head"], n1, lo, hi)[1]) for lo, hi in zip(plan[:-1], plan[1:])]
    assert any(x & y for k, x in enumerate(picked) for y in picked[k + 1:])


def test_head_weights_and_costs_by_hand():
    subs1, subs2 = [b"a", b"b", b"a", b"c"], [b"a", b"x", b"a", b"c", b"x"]
    head = K.py_head(subs1, subs2)
    assert head == [0, 1, 0, 3, 0, None, 0, 3, None]
    C, W = K.py_weights(head, 4, [10, 20, 30, 40, 50])
    assert C == [2, 0, 0, 1] and W == [40, 0, 0, 40]
    assert K.py_costs(head, C, W, [7, 7, 7, 7]) == [7 * 3 + 80, 7, 7 * 3 + 80, 7 * 2 + 80]   # the text of file 2 once per record of the ID
    assert K.window_members(head, 4, 0, 1) == ([0], [0, 2]) and K.window_members(head, 4, 1, 2) == ([1], [])
    assert K.window_members(head, 4, 2, 4) == ([2, 3], [0, 2, 3]) and K.tail_members(head, 4) == [1, 4]
    assert [K.window_shift(n) for n in (0, 1, 4096, 4097, 8192, 8193)] == [0, 0, 0, 1, 1, 2]
    hb, hr = K.window_hist([5] * 4097)
    assert hr[:2049] == [2] * 2048 + [1] and hb[2048] == 5 and sum(hr) == 4097


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_use_no_scratch(tmp_path):
    """the compiler's resource report for gfx950: no scratch and no spilled register in any kernel of the file.  LDS: the
    comparison kernel holds one word per record of its block (256 / 8 = 32) and the count of the block's heads, 128 + 4 = 132
    bytes; the window histogram the 48 KiB of bucket_hist; the others none"""
    src = os.path.join(ROOT, "bigseqkit_amd", "csrc", "ops_concat_buckets.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", str(tmp_path / "o.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want = {"k_catb_verify": 132, "k_catb_set": 0, "k_catb_weigh": 0, "k_catb_hist": 4096 * 12, "k_catb_mark": 0, "k_catb_pick": 0,
            "k_catb_tail": 0}
    assert sorted(re.findall(r"void (k_\w+)\(", open(src).read())) == sorted(want)          # every kernel of the file
    seen = {}
    for b in r.stderr.split("Function Name: ")[1:]:
        sym = b.split(" ", 1)[0]
        for k in want:
            if re.search(r"\d" + k + "E", sym):
                seen[k] = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
                assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, sym
                assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0 and int(re.search(r"SGPRs Spill: (\d+)", b).group(1)) == 0, sym
    assert seen == want, seen
