"""`common` in buckets of the key without a GPU (PARITY.md COMB): the restated `common` is the oracle's; the composition the design
rests on -- the keep bits decided inside every interval of fine bins, put back by global index, are the keep bits of the whole
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
import common_buckets_ref as M
import rmdup_buckets_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
IDS = lambda o: "+".join(k if v is True else "w%d" % v["LineWidth"] for k, v in o.items()) or "id"
COMMON_BUCKETS = bsk.CommonBuckets   # what this file restates: without the bucket path of `common` there is nothing to restate


@pytest.mark.parametrize("nfiles", (2, 3))
@pytest.mark.parametrize("name", R.SHAPES)
@pytest.mark.parametrize("o", M.OPTION_SETS, ids=IDS)
def test_restated_common_is_the_oracles(name, nfiles, o):
    oj = json.dumps(o)
    texts, fastq = M.files_text(name, nfiles)
    recs, subs, hb, hr, bits, file_records = M.restated(name, nfiles, oj)
    assert file_records == [500] * nfiles and sum(hr) == 500 * nfiles
    assert recs == M.files_records(name, nfiles)                                     # the text says what the records say
    want = M.want_of(name, nfiles, oj)
    assert R.parse(want, fastq) == M.py_common(recs, o) == [r for r, b in zip(recs[0], bits) if b]
    if o.get("Config") and not fastq:
        assert max(len(ln) for ln in want.split(b"\n") if not ln.startswith(b">")) == 20


def bits_by_intervals(subs, file_records, bounds):
    """the keep bits decided inside every interval of bins on its own, put back by global index"""
    bits = [None] * file_records[0]
    bins = [R.bin_of(s) for s in subs]
    full = (1 << len(file_records)) - 1
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        idx = [g for g, b in enumerate(bins) if lo <= b < hi]
        mask, first = {}, {}
        for g in idx:                                                                # (ascending: the bucket receives its records in input order)
            mask[subs[g]] = mask.get(subs[g], 0) | 1 << M.file_of(file_records, g)
            first.setdefault(subs[g], g)
        for g in idx:
            if g < file_records[0]:
                assert bits[g] is None                                               # a global index belongs to one bucket only
                bits[g] = 1 if mask[subs[g]] == full and first[subs[g]] == g else 0
    return bytes(bits)


@pytest.mark.parametrize("nfiles", (2, 3))
@pytest.mark.parametrize("name", R.SHAPES)
@pytest.mark.parametrize("o", M.OPTION_SETS, ids=IDS)
def test_bits_of_the_intervals_are_the_bits_of_the_input(name, nfiles, o):
    recs, subs, hb, hr, bits, file_records = M.restated(name, nfiles, json.dumps(o))
    rng = random.Random(5)
    plans = [bsk.ShufflePlan(hb, b) for b in R.budgets_of(hb)]
    plans += [[0] + sorted(rng.sample(range(1, R.BINS), k - 1)) + [R.BINS] for k in range(1, 51)]
    for bounds in plans:
        assert bounds[0] == 0 and bounds[-1] == R.BINS
        assert bits_by_intervals(subs, file_records, bounds) == bits, len(bounds) - 1


@pytest.mark.parametrize("nfiles", (2, 3))
@pytest.mark.parametrize("name", R.SHAPES)
def test_inputs_meet_the_preconditions_of_the_gpu_tests(name, nfiles):
    """asserted with the oracle alone: the text of the result says which records of file 1 were printed"""
    texts, fastq = M.files_text(name, nfiles)
    parsed = [R.parse(t, fastq) for t in texts]
    spans = oracle.record_spans(texts[0], fastq)
    assert all(len(p) == 500 for p in parsed) and len(spans) == 500
    for o in M.OPTION_SETS:
        so = M.subject_opts(o)
        printed = R.parse(oracle.common(list(texts), fastq, json.dumps(o)), fastq)
        assert 0 < len(printed) < 500                                                # neither empty nor all of file 1
        subs = [[R.subject(r, so) for r in p] for p in parsed]
        printed_subs = [R.subject(r, so) for r in printed]
        assert len(set(printed_subs)) == len(printed_subs)                           # one record per key
        assert any(subs[0].count(s) >= 2 for s in printed_subs[:50])                 # a key comes twice in file 1 and is printed once
        if nfiles == 3:
            sets = [set(s) for s in subs]
            assert any(sum(1 for t in sets if s in t) == 2 for s in subs[0])         # a key of file 1 is missing from exactly one file
        hb = R.py_hist([s for f in subs for s in f])[0]
        one, eight, fullest = R.budgets_of(hb)
        assert len(bsk.ShufflePlan(hb, one)) - 1 == 1
        assert eight >= max(hb) and len(bsk.ShufflePlan(hb, eight)) - 1 >= 8         # the 8-bucket budget admits the largest bin
        assert len(bsk.ShufflePlan(hb, fullest)) - 1 >= 8
        with pytest.raises(bsk.BskError):
            bsk.ShufflePlan(hb, fullest - 1)
        for parts in (3, 7):
            cuts = R.cuts_of(texts[0], fastq, parts)
            assert len(cuts) == parts + 1 and cuts == sorted(cuts)
            starts = [s for s, _ in spans]
            shard_of = [max(k for k, c in enumerate(cuts[:-1]) if c <= s and s < cuts[k + 1]) for s in starts]
            first_seen = {}
            assert sum(1 for g, s in enumerate(subs[0]) if shard_of[first_seen.setdefault(s, g)] != shard_of[g]) >= 1   # a group spans two shards
            if parts == 7:
                assert cuts[3] == cuts[4] and shard_of.count(0) == 1                 # an empty shard, a one-record shard


def test_masked_key_input_exercises_the_flagged_path():
    """under 16 bits of the key some IDs share a key group: records are flagged, and both a kept text and a text of file 1 that
    is not kept share their key group with a foreign text -- so the host has bits to set and bits to leave clear, and the mask
    of a head must not count the files of an intruder"""
    files = M.masked_key_files()
    subs = [R.subject(r, {}) for f in files for r in f]
    file_records = [len(f) for f in files]
    assert file_records == [3000, 3000] and len(set(subs)) == 4500
    assert sum(M.py_bits(subs, file_records)) == 1500
    flagged, kept_shared, dropped_shared = M.masked_groups(subs, file_records)
    assert flagged >= 1 and kept_shared >= 1 and dropped_shared >= 1
    assert M.masked_groups(subs, file_records, 64)[0] == 0                            # whole keys: nothing is flagged


def test_last_byte_collisions_exist():
    """the pairs of the comparison-lane test: equal but for the last byte, equal in the low 16 bits of the key, different keys"""
    for L in M.LANE_LENGTHS:
        pair = M.last_byte_collision(L)
        if L < 2:
            assert pair is None
            continue
        s, t = pair
        assert len(s) == len(t) == L and s[:-1] == t[:-1] and s[-1] != t[-1]
        assert oracle.xxh64(s) != oracle.xxh64(t) and (oracle.xxh64(s) ^ oracle.xxh64(t)) & 0xFFFF == 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_use_no_scratch(tmp_path):
    """the compiler's resource report for gfx950: no scratch and no spilled register in any kernel of the file.  The comparison
    kernel holds the running sums of the records per file (64 * 8 bytes) and one word per record of its block (256 / 8 = 32):
    512 + 128 = 640 bytes; the decide kernel holds the block's count of kept records, 4 bytes; the others use no LDS"""
    src = os.path.join(ROOT, "bigseqkit_amd", "csrc", "ops_common_buckets.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", str(tmp_path / "o.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want = ("k_comb_verify", "k_comb_decide", "k_comb_set", "k_comb_apply")
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
    assert seen["k_comb_verify"] == 64 * 8 + (256 // 8) * 4
    assert seen["k_comb_decide"] == 4
    assert seen["k_comb_set"] == 0 and seen["k_comb_apply"] == 0
