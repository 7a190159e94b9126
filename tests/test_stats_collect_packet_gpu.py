"""bsk_stats_collect brings the status words, the header slots and the first 4 096 bins of the histogram to the host with one
kernel and one copy, and the bins beyond them -- long reads -- with a second copy.  With the context's own vector and with a
caller-owned one, with a histogram that ends below and above the packet, with and without lengths beyond the histogram
(the overflow list): the map is the CPU oracle's."""
import ctypes as C
import json

import pytest

import oracle
import bigseqkit_amd as bsk
from bigseqkit_amd._lib import check, lib

pytestmark = pytest.mark.gpu

PACK_BINS = 4096   # ctx.hpp
HIST_CAP = 65536


def fastq(lengths):
    out = []
    for i, L in enumerate(lengths):
        out.append(b"@r%d\n" % i + b"ACGT" * (L // 4) + b"N" * (L % 4) + b"\n+\n" + b"I" * L + b"\n")
    return b"".join(out)


SHORT = [150] * 500 + [0, 1, 36, 2047, 2048, PACK_BINS - 1]           # extent == PACK_BINS: the packet alone
LONG = [PACK_BINS, PACK_BINS + 1, 30000, HIST_CAP - 1]                 # extent up to the whole histogram: the second copy
OVER = [HIST_CAP, HIST_CAP + 1, 200000, 200000]                        # not in the histogram at all: the overflow list
CASES = {"below": SHORT, "at_edge": SHORT + [PACK_BINS], "above": SHORT + LONG, "below_overflow": SHORT + OVER,
         "above_overflow": SHORT + LONG + OVER, "only_overflow": OVER, "only_long": [HIST_CAP - 1]}


@pytest.mark.parametrize("own_vector", [False, True])
@pytest.mark.parametrize("all_", [False, True])
@pytest.mark.parametrize("case", sorted(CASES))
def test_collect_packet(case, all_, own_vector):
    import torch
    data = fastq(CASES[case])
    want = oracle.stats_map(data, True, json.dumps({"All": all_}))
    op = bsk.Operator("Stats", json.dumps({"All": all_}), 0)
    try:
        assert lib.bsk_stats_vector_len(op.ctx) == 8 + HIST_CAP
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        vec = torch.zeros(lib.bsk_stats_vector_len(op.ctx), dtype=torch.int64, device="cuda") if own_vector else None
        dv = C.c_void_p(vec.data_ptr()) if own_vector else None
        for step in range(2):   # (the second step: what a reset leaves behind must not show)
            if own_vector:
                vec.zero_()
            check(lib.bsk_stats_reset(op.ctx, None), op.ctx)
            check(lib.bsk_stats_run(op.ctx, C.c_void_p(t.data_ptr()), len(data), 1, bsk.FORMAT_FASTQ, 0, dv, None), op.ctx)
            got = bsk.api._collect_map(op, dv)
            assert got == want, (case, step)
            total = C.c_uint64()
            check(lib.bsk_stats_overflow_total(op.ctx, C.byref(total)), op.ctx)
            assert total.value == sum(1 for L in CASES[case] if L >= HIST_CAP)
    finally:
        op.close()


def test_own_and_caller_vectors_take_turns():
    """a context that runs on its own vector, then on the caller's, then on its own again: every reset leaves both clean"""
    import torch
    data = fastq([150] * 100 + [5000])
    want = oracle.stats_map(data, True, "{}")
    op = bsk.Operator("Stats", "{}", 0)
    try:
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        vec = torch.zeros(lib.bsk_stats_vector_len(op.ctx), dtype=torch.int64, device="cuda")
        for dv in (None, C.c_void_p(vec.data_ptr()), C.c_void_p(vec.data_ptr()), None, None):
            vec.zero_()
            check(lib.bsk_stats_reset(op.ctx, None), op.ctx)
            check(lib.bsk_stats_run(op.ctx, C.c_void_p(t.data_ptr()), len(data), 1, bsk.FORMAT_FASTQ, 0, dv, None), op.ctx)
            assert bsk.api._collect_map(op, dv) == want
    finally:
        op.close()
