"""`sort` in buckets of the key without a GPU (PARITY.md SORT "Buckets"): the splitters that bsk_sort_pick_splitters -- a pure
host function -- draws from a sample, the invariant the design rests on -- stable sorts per bin, concatenated, are the stable
sort -- in plain Python, and the compiler's resource report for the kernels."""
import bisect
import os
import random
import re
import subprocess

import pytest

import bigseqkit_amd as bsk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
BINS = 4096


def strip0(s):
    """a string without its trailing zero bytes is the same string under the padded comparison (bytes, the shorter string
    zero-padded), and on such strings that comparison is the plain one"""
    return s.rstrip(b"\0")


def bins_of(keys, splitters):
    sp = [strip0(s) for s in splitters]
    return [bisect.bisect_right(sp, strip0(k)) for k in keys]


def check_splitters(keys, max_bins):
    sp = bsk.SortPickSplitters(keys, max_bins)
    assert sp == bsk.SortPickSplitters(keys, max_bins)                                   # the same sample, the same splitters
    s0 = [strip0(s) for s in sp]
    assert all(a < b for a, b in zip(s0[:-1], s0[1:])), "strictly ascending under the padded comparison"
    assert len(sp) <= max_bins - 1
    pool = {strip0(k) for k in keys}
    assert all(s in pool for s in s0)                                                    # a splitter is a sample key
    if not keys:
        assert sp == []
        return sp
    n, bins = len(keys), max_bins
    per_bin, copies = {}, {}
    for k, b in zip(keys, bins_of(keys, sp)):
        per_bin[b] = per_bin.get(b, 0) + 1
        copies[strip0(k)] = copies.get(strip0(k), 0) + 1
    for b, cnt in per_bin.items():
        # a bin spans one quantile step, plus the copies of the key it begins with that lie in front of that step
        most = copies[s0[b - 1]] if b else 0
        assert cnt <= -(-n // bins) + most, (b, cnt, n, bins, most)
    return sp


@pytest.mark.parametrize("seed", range(5))
def test_pick_splitters_random_samples(seed):
    rng = random.Random(seed)
    alphabet = [b"ACGT", b"ab\0", bytes(range(256))][seed % 3]
    n = rng.choice([1, 2, 7, 500, 5000])
    keys = [bytes(rng.choice(alphabet) for _ in range(rng.randint(0, 12))) for _ in range(n)]
    keys += [rng.choice(keys) for _ in range(n // 3)]                                    # copies
    keys += [k + b"\0\0" for k in keys[:n // 5]]                                         # ... and copies under padding
    for max_bins in (1, 2, 3, 16, 4095, 4096):
        check_splitters(keys, max_bins)


def test_pick_splitters_hand_cases():
    assert check_splitters([], 4096) == []                                               # no sample: no splitter, one bin
    assert check_splitters([b"same"] * 1000, 4096) == [b"same"]                          # all equal: duplicates collapse
    assert check_splitters([b"", b"\0", b"\0\0"], 4096) == [b""]
    assert check_splitters([b"b", b"a", b"c", b"d"], 2) == [b"c"]
    assert check_splitters([b"b", b"a", b"c", b"d"], 4) == [b"b", b"c", b"d"]
    assert check_splitters([b"b", b"a", b"c", b"d"], 1) == []
    keys = [b"SRR1234567.%d" % i for i in range(9000)]                                   # a long common prefix
    sp = check_splitters(keys, 4096)
    assert len(sp) == 4095
    with pytest.raises(bsk.BskError):
        bsk.SortPickSplitters([b"a"], 4097)


@pytest.mark.parametrize("seed", range(4))
def test_stable_sorts_per_bin_concatenated_are_the_stable_sort(seed):
    """the invariant in plain Python, in both directions: ties keep input order because a bin receives its records in input
    order; descending, the bins are taken from the last to the first"""
    rng = random.Random(100 + seed)
    recs = [(bytes(rng.choice(b"AC\0") for _ in range(rng.randint(0, 4))), i) for i in range(400)]
    key = lambda r: strip0(r[0])
    pool = sorted({key(r) for r in recs} | {key(r)[:1] for r in recs})
    for k in (0, 1, 3, len(pool)):
        sp = sorted(rng.sample(pool, k))
        b = bins_of([r[0] for r in recs], sp)
        per_bin = [[r for r, x in zip(recs, b) if x == j] for j in range(len(sp) + 1)]
        asc = [r for part in per_bin for r in sorted(part, key=key)]
        assert asc == sorted(recs, key=key)
        desc = [r for part in reversed(per_bin) for r in sorted(part, key=key, reverse=True)]
        assert desc == sorted(recs, key=key, reverse=True)
        # monotone: a larger key never lies in a lower bin; equal keys share one
        order = sorted(range(len(recs)), key=lambda i: key(recs[i]))
        assert all(b[i] <= b[j] for i, j in zip(order[:-1], order[1:]))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_use_no_scratch(tmp_path):
    """the compiler's resource report for gfx950: no scratch and no spilled register in any kernel of the file; the histogram's
    LDS lets three blocks share the 160 KB of a CU"""
    src = os.path.join(ROOT, "bigseqkit_amd", "csrc", "ops_sort_buckets.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", str(tmp_path / "o.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want = ("k_sort_sample_size", "k_sort_sample_keys", "k_sort_bins", "k_sort_hist", "k_sort_pick")
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
    assert 0 < seen["k_sort_hist"] <= 160 * 1024 // 3
    assert all(v == 0 for k, v in seen.items() if k != "k_sort_hist")
