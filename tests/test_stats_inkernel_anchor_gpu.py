"""FASTQ `stats` without k_prep: the waves of k_stats find the range behind a queue ticket themselves (the default), against
the older order -- k_prep writes anchors[], k_stats reads them -- that the switch stats_prep=pass keeps.  The two must give
identical maps, identical error codes and identical error texts, and the maps must be the CPU oracle's."""
import ctypes as C
import json
import random

import pytest

import oracle
import seqgen
import bigseqkit_amd as bsk
from bigseqkit_amd._lib import BSK_ERR_FORMAT, BSK_ERR_UNSUPPORTED, BskError, check, lib

pytestmark = pytest.mark.gpu


def dev(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def run(data, switches, all_=False, steps=1):
    """(map, None) or (None, (code, text)) of `steps` reset -> run -> collect rounds on one context (the last one counts)"""
    op = bsk.Operator("Stats", json.dumps({"All": all_}), 0)
    try:
        for k, v in switches.items():
            check(lib.bsk_ctx_set(op.ctx, k.encode(), str(v).encode()), op.ctx)
        t = dev(data)
        m = None
        for _ in range(steps):
            check(lib.bsk_stats_reset(op.ctx, None), op.ctx)
            check(lib.bsk_stats_run(op.ctx, C.c_void_p(t.data_ptr()), len(data), 1, bsk.FORMAT_FASTQ, 0, None, None), op.ctx)
            m = bsk.api._collect_map(op)
        return m, None
    except BskError as e:
        return None, (e.code, str(e))
    finally:
        op.close()


def forced_ranges(n, switches):
    """How many ranges a shard of n bytes is cut into when the switches pin the count (ranges_per_wave = 1), at least:
    pick_nranges (ctx.hpp) gives min(resident waves, n / min_range_bytes), and the persistent grid has at least one block
    of four waves per compute unit.  Without ranges_per_wave, min_range_bytes only caps a count that is n / 128 KiB anyway."""
    import torch
    assert switches.get("ranges_per_wave") == 1
    return min(4 * torch.cuda.get_device_properties(0).multi_processor_count, n // int(switches["min_range_bytes"]))


def both_paths(data, switches=None, all_=False, steps=1, must_raise=False, paths_only=False, want_ranges=0):
    switches = dict(switches or {})
    if want_ranges and "ranges_per_wave" in switches:
        # the shard really is cut as finely as the test means it to be
        assert forced_ranges(len(data), switches) >= want_ranges[int(switches["min_range_bytes"])], (len(data), switches)
    new = run(data, switches, all_, steps)
    old = run(data, dict(switches, stats_prep="pass"), all_, steps)
    assert new == old, (new, old, switches, data[:120])
    if paths_only:
        return new
    if must_raise:
        # (a shard that ends inside a header or a bases line: the reference's reader -- the oracle -- takes what is there
        # for a record, the strict 4-line reader of the HIP path refuses it, with k_prep and without: an error, whatever
        # the oracle says)
        assert new[0] is None and new[1] is not None, (new, data[-120:])
        return new
    try:
        want = oracle.stats_map(data, True, json.dumps({"All": all_}))
    except oracle.OracleError:
        want = None
    if want is None:
        assert new[0] is None and new[1] is not None, (new, data[:120])
    else:
        assert new[0] == want, (new, switches, data[:120])
    return new


def fixed_fastq(lengths, tag=b"r"):
    out = []
    for i, L in enumerate(lengths):
        out.append(b"@" + tag + str(i).encode() + b"\n" + b"ACGT" * (L // 4) + b"N" * (L % 4) + b"\n+\n" + b"I" * L + b"\n")
    return b"".join(out)


# Ranges of 256 bytes (min_range_bytes at its minimum, the count pinned to one per wave so that the minimum is what
# decides: a boundary every 256 bytes up to the number of resident waves, many of them inside one record), of 4 KiB,
# and the default geometry (>= 128 KiB).  The tests pass the number of ranges they count on as want_ranges.
RANGES = [{"min_range_bytes": 256, "ranges_per_wave": 1}, {"min_range_bytes": 4096, "ranges_per_wave": 1}, {}]


@pytest.mark.parametrize("sw", RANGES)
@pytest.mark.parametrize("seed", range(3))
def test_clean_fastq_of_mixed_lengths(seed, sw):
    rng = random.Random(700 + seed)
    data = seqgen.random_fastq(rng, 3000, 0, [40, 300, 3000][seed], final_newline=seed != 1, trailing_blank=seed)
    both_paths(data, sw, want_ranges={256: 500, 4096: 30})


@pytest.mark.parametrize("sw", RANGES)
def test_at_and_plus_open_every_quality_line(sw):
    rng = random.Random(11)
    recs = []
    for i in range(4000):
        L = rng.randint(1, 120)
        q = rng.choice("@+") + "".join(chr(rng.randint(33, 126)) for _ in range(L - 1))
        recs.append("@r%d\n%s\n+\n%s\n" % (i, "".join(rng.choice("ACGT") for _ in range(L)), q))
    both_paths("".join(recs).encode(), sw, want_ranges={256: 1000, 4096: 100})


@pytest.mark.parametrize("sw", RANGES)
def test_no_final_line_feed_and_empty_reads(sw):
    rng = random.Random(12)
    lengths = [rng.choice([0, 0, 1, 7, 150]) for _ in range(5000)]
    data = fixed_fastq(lengths)
    both_paths(data[:-1], sw, want_ranges={256: 1000, 4096: 80})
    both_paths(data + b"\n\n", sw, want_ranges={256: 1000, 4096: 80})
    both_paths(data + b"\n" * 5000, sw, want_ranges={256: 1000, 4096: 80})   # (the effective end, found 64 bytes per step)
    both_paths(fixed_fastq([0] * 3000), sw, want_ranges={256: 100, 4096: 6})


@pytest.mark.parametrize("sw", RANGES)
def test_one_record_longer_than_a_range(sw):
    data = fixed_fastq([100] * 300) + fixed_fastq([300000], b"long") + fixed_fastq([100] * 300, b"s")
    # (256: one range per resident wave, at most 720 bytes each -- the two lines of the long record hold 800 boundaries)
    both_paths(data, sw, want_ranges={256: 1000, 4096: 150})


def test_shards_smaller_than_a_range_and_of_one_record():
    both_paths(fixed_fastq([150] * 10))
    both_paths(fixed_fastq([150]))
    both_paths(fixed_fastq([150])[:-1])
    both_paths(fixed_fastq([0]))
    both_paths(b"@a\nA\n+\nI")
    both_paths(fixed_fastq([150]), {"min_range_bytes": 256, "ranges_per_wave": 1})
    both_paths(fixed_fastq([70000]), {"min_range_bytes": 256, "ranges_per_wave": 1}, want_ranges={256: 500})


@pytest.mark.parametrize("tail", ["uniform", "4096", None])
def test_ranges_that_shrink_towards_the_end(tail):
    """2.5 MB with min_range_bytes = 4096: 16 and more nominal ranges whose last sixteenth goes out in quarter chunks when
    the floor for those is lowered to 4 KiB (stats_tail=4096; uniform: one size; unset: the floor of 192 KiB, one size
    here); several steps on one context -- the range queue must be back at zero after a kernel"""
    rng = random.Random(13)
    data = seqgen.random_fastq(rng, 14000, 50, 250)
    assert len(data) > 2 << 20
    sw = {"min_range_bytes": 4096}
    if tail:
        sw["stats_tail"] = tail
    both_paths(data, sw, steps=3)
    both_paths(data, dict(sw, ranges_per_wave=1), steps=2)


def test_two_runs_between_resets_add_up():
    data = fixed_fastq([150] * 2000)
    op = bsk.Operator("Stats", json.dumps({}), 0)
    try:
        check(lib.bsk_ctx_set(op.ctx, b"min_range_bytes", b"1024"), op.ctx)
        t = dev(data)
        for pid in range(2):
            check(lib.bsk_stats_run(op.ctx, C.c_void_p(t.data_ptr()), len(data), 1, bsk.FORMAT_FASTQ, pid, None, None), op.ctx)
        m = bsk.api._collect_map(op)
    finally:
        op.close()
    assert m[150] == 4000


MALFORMED = {
    "truncated_in_header": lambda d, k: d[:k + 3],
    "truncated_in_bases": lambda d, k: d[:d.index(b"\n", k) + 5],
    "truncated_after_plus": lambda d, k: d[:d.index(b"\n+\n", k) + 3],
    "missing_plus": lambda d, k: d[:d.index(b"\n+\n", k) + 1] + b"-" + d[d.index(b"\n+\n", k) + 2:],
    "quality_shorter": lambda d, k: d[:d.index(b"\n+\n", k) + 3] + d[d.index(b"\n+\n", k) + 5:],
    "quality_longer": lambda d, k: d[:d.index(b"\n+\n", k) + 3] + b"II" + d[d.index(b"\n+\n", k) + 3:],
}
# What the strict 4-line reader of the HIP path has to answer, from its rules (include/bsk.h, capi.cpp describe_kernel_errors),
# not from what either order of kernels gives: a shard whose line count is no multiple of four ends inside a record (the
# reference's Call() error class); a third line without '+' is a layout the HIP path does not take; four lines with
# qualities of another length than the bases are the reference's own "unmatched length" error -- and so is a shard that
# ends right behind the line feed of its last '+' line: the last line of a file need not end with a line feed, so what
# follows is a quality line of length 0 (tests/test_stats_gpu.py HAND: `@a\n\n+\n` is a whole record), which the oracle
# reports with the same words.
EXPECTED_ERROR = {
    "truncated_in_bases": (BSK_ERR_FORMAT, "FASTQ ends inside a record"),
    "truncated_after_plus": (BSK_ERR_FORMAT, "unmatched length of sequence and quality"),
    "missing_plus": (BSK_ERR_UNSUPPORTED, "third line must start with '+'"),
    "quality_shorter": (BSK_ERR_FORMAT, "unmatched length of sequence and quality"),
    "quality_longer": (BSK_ERR_FORMAT, "unmatched length of sequence and quality"),
}


@pytest.mark.parametrize("sw", RANGES)
@pytest.mark.parametrize("kind", sorted(MALFORMED))
def test_malformed_shards_raise_the_same_error(kind, sw):
    rng = random.Random(14)
    data = fixed_fastq([rng.randint(20, 200) for _ in range(6000)])   # 1.4 MB
    for frac in (0.001, 0.37, 0.5, 0.93):
        k = data.index(b"\n@", int(len(data) * frac)) + 1
        bad = MALFORMED[kind](data, k)
        # A header cut off before its line feed, behind whole records, is no line to the HIP reader: k_stats sees no event
        # for it and answers with the map of the records in front of it, where the oracle counts one more, empty, record.
        # That is the reader's business, before this change as after it; what is held here is that the two orders agree
        # and that the records in front of the fragment are all counted.
        if kind == "truncated_in_header":
            got = both_paths(bad, sw, paths_only=True)
            want = oracle.stats_map(bad[:k], True, "{}")
            assert got[0] == want, (frac, got)
            continue
        got = both_paths(bad, sw, must_raise=True, want_ranges={256: 2, 4096: 0} if frac < 0.01 else {256: 1000, 4096: 100})
        code, text = EXPECTED_ERROR[kind]
        assert got[1][0] == code and text in got[1][1], (kind, frac, got)


@pytest.mark.parametrize("sw", RANGES)
def test_text_that_is_not_fastq(sw):
    rng = random.Random(15)
    fasta = seqgen.random_fasta(rng, 800, 50, 400)
    got = both_paths(fasta, sw, want_ranges={256: 500, 4096: 30})
    assert got[0] is None
