"""`pair` in buckets of the key without a GPU (PARITY.md PAIRB): the restated `pair` is the oracle's; the two compositions the
design rests on -- the pairs decided inside every interval of fine bins, put back by global index, are the pairs of the whole
input, and the order buckets of any cut of the order bins, joined, are paired.2 -- in plain Python with the reference's XXH64
and the plan of bsk_shuffle_plan; the preconditions of the GPU tests' inputs; and the compiler's resource report for the kernels."""
import json
import os
import random
import re
import subprocess

import pytest

import bigseqkit_amd as bsk
import oracle
import pair_buckets_ref as P
import rmdup_buckets_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
PAIR_BUCKETS = bsk.PairBuckets   # what this file restates: without the bucket path of `pair` there is nothing to restate


@pytest.mark.parametrize("variant", P.VARIANTS)
@pytest.mark.parametrize("name", R.SHAPES)
def test_restated_pair_is_the_oracles(name, variant):
    texts, fastq = P.files_text(name, variant)
    r = P.restated(name, variant)
    assert r["recs"] == [list(f) for f in P.files_records(name, variant)]            # the text says what the records say
    widths = (None,) if fastq else (None, 0, 20)
    for unpaired in (True, False):
        for w in widths:
            o = {"SaveUnpaired": unpaired}
            if w is not None:
                o["Config"] = {"LineWidth": w}
            want = P.want_of(name, variant, json.dumps(o))
            got = P.py_outputs(r["recs"][0], r["recs"][1], unpaired)
            # (the oracle computes the unpaired outputs whatever SaveUnpaired says: the operator leaves them empty without it)
            assert tuple(R.parse(t, fastq) for t in want)[:4 if unpaired else 2] == got[:4 if unpaired else 2], (unpaired, w)
            assert unpaired or got[2:] == ([], [])
            if w == 20:
                assert max(len(ln) for ln in want[0].split(b"\n") if not ln.startswith(b">")) == 20
            if w == 0:
                assert want[0].count(b"\n") <= 2 * len(P.py_outputs(r["recs"][0], r["recs"][1])[0])


@pytest.mark.parametrize("variant", P.VARIANTS)
@pytest.mark.parametrize("name", R.SHAPES)
def test_pairs_of_the_intervals_are_the_pairs_of_the_input(name, variant):
    r = P.restated(name, variant)
    subs1, subs2 = r["subs"]
    hb = r["hist"][0]
    paired1, paired2, mate = r["pair"][:3]
    rng = random.Random(5)
    plans = [bsk.ShufflePlan(hb, b) for b in R.budgets_of(hb)]
    plans += [[0] + sorted(rng.sample(range(1, R.BINS), k - 1)) + [R.BINS] for k in range(1, 51)]
    for bounds in plans:
        assert bounds[0] == 0 and bounds[-1] == R.BINS
        assert P.pairs_by_intervals(subs1, subs2, bounds) == (paired1, paired2, mate), len(bounds) - 1


@pytest.mark.parametrize("pairs", (1, 4095, 4096, 4097, 3 * 4096 + 17))
def test_order_buckets_joined_are_paired_2(pairs):
    """every second record of file 2 is paired, their positions a permutation: for cuts of the order bins into runs -- one run,
    every bin its own run, random cuts -- the buckets in ascending pos, joined, are the records of file 2 in ascending pos"""
    rng = random.Random(pairs)
    perm = list(range(pairs))
    rng.shuffle(perm)
    pos2 = [p for q in perm for p in (q, None)]
    want = [j for _, j in sorted((p, j) for j, p in enumerate(pos2) if p is not None)]
    s = P.order_shift(pairs)
    assert (pairs - 1) >> s < P.ORDER_BINS and (s == 0 or (pairs - 1) >> (s - 1) >= P.ORDER_BINS)
    assert {1: 0, 4095: 0, 4096: 0, 4097: 1}.get(pairs, 2) == s
    hb, hr = P.order_hist(pos2, [10] * len(pos2), pairs)
    assert sum(hr) == pairs and sum(hb) == 10 * pairs and max(hr) <= 1 << s
    cuts = [[0, P.ORDER_BINS], list(range(P.ORDER_BINS + 1))]
    cuts += [[0] + sorted(rng.sample(range(1, P.ORDER_BINS), k)) + [P.ORDER_BINS] for k in (1, 2, 7, 100)]
    cuts += [bsk.ShufflePlan(hb, max(max(hb), sum(hb) // 9))]
    for bounds in cuts:
        assert P.order_by_intervals(pos2, pairs, bounds) == want, len(bounds) - 1


@pytest.mark.parametrize("name", R.SHAPES)
def test_inputs_meet_the_preconditions_of_the_gpu_tests(name):
    """asserted with the oracle alone: the texts of the results say which records were printed, and in which order"""
    for variant in P.VARIANTS:
        texts, fastq = P.files_text(name, variant)
        spans = [oracle.record_spans(t, fastq) for t in texts]
        assert [len(s) for s in spans] == [500, 500]
        out = [R.parse(t, fastq) for t in oracle.pair(texts[0], texts[1], fastq, json.dumps({"SaveUnpaired": True}))]
        ids = [[R.subject(r, {}) for r in f] for f in out]
        n_pairs = len(out[0])
        assert 0 < n_pairs < 500 and len(out[1]) == n_pairs and ids[0] == ids[1]
        assert len(out[2]) == 500 - n_pairs and len(out[3]) == 500 - n_pairs
        both = [[R.subject(r, {}) for r in R.parse(t, fastq)] for t in texts]
        assert both[0].count(b"r7") == 2 and both[1].count(b"r7") == 1                # the surplus of file 1 is unpaired
        assert ids[0].count(b"r7") == 1 and [R.subject(r, {}) for r in out[2]].count(b"r7") == 1
        assert both[0].count(b"r11") == 2 and both[1].count(b"r11") == 2 and ids[0].count(b"r11") == 2   # the k-th goes with the k-th
        recs2 = R.parse(texts[1], fastq)
        eleven = [r for r in recs2 if R.subject(r, {}) == b"r11"]
        assert [r for r in out[1] if R.subject(r, {}) == b"r11"] == eleven
        assert both[1].count(b"r13") == 2 and ids[1].count(b"r13") == 1               # the surplus of file 2 is unpaired
        # file 2 is in mate order iff paired.2 is a filter of file 2
        paired2_in_file_order = [r for r in recs2 if r in out[1]]
        assert (out[1] == paired2_in_file_order) == (variant == "ordered")
        assert P.in_mate_order(P.restated(name, variant)["pair"][4]) == (variant == "ordered")
        # a group spans two shards
        for parts in (3, 7):
            for f in (0, 1):
                cuts = R.cuts_of(texts[f], fastq, parts)
                assert len(cuts) == parts + 1 and cuts == sorted(cuts)
                starts = [s for s, _ in spans[f]]
                shard_of = [max(k for k, c in enumerate(cuts[:-1]) if c <= s and s < cuts[k + 1]) for s in starts]
                first_seen = {}
                spanning = sum(1 for g, s in enumerate(both[f]) if shard_of[first_seen.setdefault(s, g)] != shard_of[g])
                assert spanning >= 1 or f == 1
        # the budgets of both phases
        r = P.restated(name, variant)
        for hb in (r["hist"][0], r["order_hist"][0]):
            one, eight, fullest = R.budgets_of(hb)
            assert len(bsk.ShufflePlan(hb, one)) - 1 == 1
            assert eight >= max(hb) and len(bsk.ShufflePlan(hb, eight)) - 1 >= 8     # the 8-bucket budget admits the largest bin
        assert sum(r["order_hist"][1]) == n_pairs == r["pair"][5]


def test_masked_key_input_exercises_the_flagged_path():
    """under 16 bits of the key some IDs share a key group: records are flagged, a flagged text has a mate -- the host has a pair
    to set -- and a flagged text of file 1 has none -- the host has bits to leave clear"""
    files = P.masked_key_files()
    subs = [[R.subject(r, {}) for r in f] for f in files]
    assert [len(s) for s in subs] == [3000, 3000] and len(set(subs[0] + subs[1])) == 4500
    assert P.py_pair(*subs)[5] == 1500
    flagged, flagged_paired, flagged_alone1 = P.masked_groups(*subs)
    assert flagged >= 1 and flagged_paired >= 1 and flagged_alone1 >= 1
    assert P.masked_groups(*subs, bits=64)[0] == 0                                    # whole keys: nothing is flagged


def test_last_byte_collisions_exist():
    """the pairs of the comparison-lane test: equal but for the last byte, equal in the low 16 bits of the key, different keys"""
    for L in P.LANE_LENGTHS:
        pair = P.last_byte_collision(L)
        if L < 2:
            assert pair is None
            continue
        s, t = pair
        assert len(s) == len(t) == L and s[:-1] == t[:-1] and s[-1] != t[-1] and b" " not in s + t
        assert oracle.xxh64(s) != oracle.xxh64(t) and (oracle.xxh64(s) ^ oracle.xxh64(t)) & 0xFFFF == 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_use_no_scratch(tmp_path):
    """the compiler's resource report for gfx950: no scratch and no spilled register in any kernel of the file.  LDS: the
    comparison kernel holds one word per record of its block (256 / 8 = 32), the count of the block's members and the base of
    its places in the list, 128 + 4 + 8 = 140 bytes, which the compiler lays out in 144; the scatter and the rank kernel one
    32-bit count of the block; the count kernel one word per lane, 1024 bytes; the order histogram the 48 KiB of bucket_hist;
    the apply kernel two 64-bit and two 32-bit sums, 24 bytes; the others none"""
    src = os.path.join(ROOT, "bigseqkit_amd", "csrc", "ops_pair_buckets.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", str(tmp_path / "o.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want = {"k_pairb_verify": 144, "k_pairb_scatter": 4, "k_pairb_set": 0, "k_pairb_count": 1024, "k_pairb_rank": 4, "k_pairb_pos": 0,
            "k_pairb_order_hist": 4096 * 12, "k_pairb_order_pick": 0, "k_pairb_order_append": 0, "k_pairb_order_slots": 0,
            "k_pairb_order_offsets": 0, "k_pairb_apply": 24}
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
