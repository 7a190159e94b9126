"""What tests/test_fuzz_late_commands_gpu.py and tests/test_sample_shuffle_scale_gpu.py take for granted, checked without a
device: the restatements alone answer at least four cases in five for every default seed (so the cap on refusals of the GPU
tests measures the library), the head-genome generator reaches every shared-prefix length and cuts in every place, the edited
FASTQ reading of replace_ref is the oracle's, and the one-block limit of the sort is the installed rocprim's."""
import os
import re

import pytest

import oracle
import head_genome_ref as HG
import replace_ref
import test_fuzz_late_commands_gpu as T
from test_sample_shuffle_scale_gpu import ONE_BLOCK_SORT

SEEDS = range(6)   # (BSK_FUZZ_SEEDS = 24, the default, // 4)


def answered(c):
    try:
        T.reference(c)
        return True
    except T.REF_ERRORS:
        return False


@pytest.mark.parametrize("tiny", [False, True], ids=["ordinary", "tiny"])
@pytest.mark.parametrize("seed", SEEDS)
def test_the_restatements_answer_four_cases_in_five(seed, tiny):
    cases = T.cases_of(seed, tiny)
    assert len(cases) == (120 if tiny else 60) and {c["op"] for c in cases} == set(T.OPS)
    assert sum(answered(c) for c in cases) >= 0.8 * len(cases)


def test_head_genome_cases_reach_every_prefix_length_and_cut():
    n_words, n_1, cuts, outcomes, ms = set(), set(), set(), set(), set()
    for seed in SEEDS:
        for c in T.cases_of(seed, False) + T.cases_of(seed, True):
            if c["op"] != "head-genome":
                continue
            descs = [d for _, _, d in HG.heads(c["data"], c["fastq"])]
            n_words |= {len(HG.words(d)) for d in descs}
            if len(descs) > 1 and descs[0] and descs[1]:
                n_1.add(HG.shared(HG.words(descs[1]), HG.words(descs[0])))
            cut, bad = HG.verdicts(descs, c["m"])
            if bad is not None:
                outcomes.add("no description, first" if bad == 0 else "no description, later")
            elif cut == len(descs):
                outcomes.add("no cut")
            else:
                outcomes.add("cut")
                cuts.add(min(cut, 50))
                if n_1 and cut > 1:
                    ms.add(c["m"])
    assert n_words == set(range(6)), n_words                 # descriptions of 0 - 5 words
    assert n_1 == set(range(6)), n_1                         # every count of shared words for the first compared record
    assert {1, 2, 3} <= cuts and max(cuts) >= 8, cuts        # the cut at record 1 (n_1 < m) and far behind it (n_i != n_1)
    assert ms == {1, 2, 3}, ms                               # ... under every m
    assert outcomes == {"cut", "no cut", "no description, first", "no description, later"}, outcomes


def test_replace_ref_reads_a_fastq_without_its_last_newline_like_the_oracle():
    """an empty last quality line whose newline is missing is a record; a missing quality line is not made up"""
    for data in (b"@r\n\n+", b"@a d\nAC\n+\nII\n@r\n\n+"):
        assert len(oracle.record_spans(data, True)) == data.count(b"@")
        want = oracle.seq(data, True, "{}")
        assert want.endswith(b"@r\n\n+\n\n")
        recs = replace_ref.parse(data, True)
        assert b"".join(replace_ref.fmt(n, s, q, 0, True) for n, s, q in recs) == want
        assert replace_ref.replace_records(data, True, {"Pattern": "nomatch", "Replacement": "z"}) == want
    with pytest.raises(IndexError):
        replace_ref.parse(b"@a\nACGT\n+", True)


def test_the_one_block_limit_of_the_sort_is_rocprims():
    """rocprim::radix_sort_pairs sorts in one block up to min(256, block_size) * min(4, items_per_thread) items, block_size and
    items_per_thread those of radix_sort_block_sort_config_base for max(sizeof(key), sizeof(value)) = 8 bytes"""
    inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include", "rocprim", "device")
    sort = open(os.path.join(inc, "device_radix_sort.hpp")).read()
    helper = open(os.path.join(inc, "detail", "device_config_helper.hpp")).read()
    m = re.search(r"kernel_config<rocprim::min\((\d+)u, default_radix_sort_block_sort_config::block_size\),\s*"
                  r"rocprim::min\((\d+)u, default_radix_sort_block_sort_config::items_per_thread\)>", sort)
    assert m, "the single-block configuration of radix_sort_pairs is not where it was"
    cap_threads, cap_items = int(m.group(1)), int(m.group(2))

    def step(name, scale):   # the first `if(item_scale <= X) return Y` of the constexpr function that holds for `scale`
        body = helper[helper.index("constexpr unsigned int %s(" % name):]
        for bound, value in re.findall(r"item_scale <= (\d+)\)\s*\{\s*return (\d+);", body[:body.index("\n}\n")]):
            if scale <= int(bound):
                return int(value)
        raise AssertionError(name)

    assert "block_size = merge_sort_block_size(item_scale) * 2" in helper
    assert "= rocprim::min(4u, merge_sort_items_per_thread(item_scale))" in helper
    block_size = step("merge_sort_block_size", 8) * 2
    items = min(4, step("merge_sort_items_per_thread", 8))
    assert min(cap_threads, block_size) * min(cap_items, items) == ONE_BLOCK_SORT
