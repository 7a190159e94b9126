"""The tile grid of stream_range (stream_core_dev.hpp) begins on a 128-byte line of memory -- by absolute address -- instead
of on `range start & ~15`, pieces of a tile that lie outside the range are not loaded, and interior tiles are loaded without
per-lane bounds tests.  None of that may show in a result: every pass built on the skeleton (`stats`, `stats -a` by line roles
and on the dense path, `seq -n`, `grep -s -p`, `subseq -r`, `rmdup -s`) is held against the CPU oracle on inputs whose range
starts take every residue mod 128 (ranges pinned at 256 bytes and 4 KiB: a few kilobytes hold hundreds of range starts), on
device views at odd byte offsets into one allocation (with a guard pattern in front and another shard's bytes behind, on
neither of which the result may depend), and on shards that end in every awkward way."""
import ctypes as C
import json
import random

import pytest

import oracle
import bigseqkit_amd as bsk
from bigseqkit_amd import _lib
from bigseqkit_amd._lib import BskError, check, lib

pytestmark = pytest.mark.gpu

RANGES = [{"min_range_bytes": 256, "ranges_per_wave": 1}, {"min_range_bytes": 4096, "ranges_per_wave": 1}]
IDS = ["ranges256", "ranges4k"]


def fastq(lengths, seed):
    """records with 12-byte headers: a read of 150 bases is 317 bytes, an odd number -- record starts walk through all residues
    mod 128; every tenth read repeats an earlier one (rmdup -s), every seventh carries the pattern of the grep case"""
    rng = random.Random(seed)
    out, seqs = [], []
    for i, L in enumerate(lengths):
        s = "".join(rng.choice("ACGTN") for _ in range(L))
        if i % 7 == 3 and L >= 40:
            k = rng.randrange(L - 12)
            s = s[:k] + "ACGTTGCAAGCT" + s[k + 12:]
        if i % 10 == 9 and seqs:
            s = rng.choice(seqs)
            L = len(s)
        seqs.append(s)
        if L and i % 13 == 5:
            s = s[:L // 2] + "-" + s[L // 2 + 1:]
        q = "".join(chr(rng.randint(33, 74)) for _ in range(L))
        if L and i % 3 == 0:
            q = "@+"[i % 2] + q[1:]
        out.append("@r%010d\n%s\n+\n%s\n" % (i, s, q))
    return "".join(out).encode()


FIXED = fastq([150] * 300, 1)
_rng = random.Random(2)
VARIABLE = fastq([_rng.choice([0, 0, 1, 15, 16, 17]) if _rng.random() < 0.2 else _rng.randint(1, 300) for _ in range(300)], 3)
assert len(FIXED) == 300 * 317 and {(317 * i) % 128 for i in range(300)} == set(range(128))
INPUTS = {"fixed": FIXED, "variable": VARIABLE}

# pass -> (operator, options, entry point, After() hook, oracle call)
RECORD_OPS = {
    "seq -n": ("SeqTransform", {"Name": True}, "bsk_seq_run", None, oracle.seq),
    "grep -s -p": ("Grep", {"BySeq": True, "Pattern": ["ACGTTGCAAGCT"]}, "bsk_grep_run", None, oracle.grep),
    "subseq -r": ("SubseqTransform", {"Region": "1:50"}, "bsk_subseq_run", None, oracle.subseq),
    "rmdup -s": ("RmDup", {"BySeq": True}, "bsk_rmdup_run", "bsk_rmdup_finish", oracle.rmdup),
}
STATS_OPS = {
    "stats": ({"All": False}, {}),
    "stats -a": ({"All": True}, {}),
    "stats -a dense": ({"All": True}, {"stats_a": "dense"}),
}
ALL_OPS = sorted(STATS_OPS) + sorted(RECORD_OPS)

_want = {}


def want(opname, data):
    """the oracle's answer, computed once per (pass, input): ("ok", map or bytes) or ("error",)"""
    key = (opname, data)
    if key not in _want:
        try:
            if opname in STATS_OPS:
                _want[key] = ("ok", oracle.stats_map(data, True, json.dumps(STATS_OPS[opname][0])))
            else:
                _want[key] = ("ok", RECORD_OPS[opname][4](data, True, json.dumps(RECORD_OPS[opname][1])))
        except oracle.OracleError:
            _want[key] = ("error",)
    return _want[key]


def run_ptr(opname, ptr, n, switches):
    """one pass over the n device bytes at ptr: ("ok", map or bytes) or ("error",)"""
    if opname in STATS_OPS:
        opts, extra = STATS_OPS[opname]
        name = "Stats"
    else:
        name, opts, entry, finish, _ = RECORD_OPS[opname]
        extra = {}
    op = bsk.Operator(name, json.dumps(opts), 0)
    try:
        for k, v in dict(switches, **extra).items():
            check(lib.bsk_ctx_set(op.ctx, k.encode(), str(v).encode()), op.ctx)
        if opname in STATS_OPS:
            check(lib.bsk_stats_reset(op.ctx, None), op.ctx)
            check(lib.bsk_stats_run(op.ctx, C.c_void_p(ptr), n, 1, bsk.FORMAT_FASTQ, 0, None, None), op.ctx)
            return ("ok", bsk.api._collect_map(op))
        out = _lib.Out()
        check(getattr(lib, entry)(op.ctx, C.c_void_p(ptr), n, 1, bsk.FORMAT_FASTQ, 0, None, C.byref(out)), op.ctx)
        buf = C.create_string_buffer(max(1, out.len))
        check(lib.bsk_out_to_host(op.ctx, C.byref(out), buf, out.len), op.ctx)
        if finish:
            check(getattr(lib, finish)(op.ctx), op.ctx)
        return ("ok", buf.raw[:out.len])
    except BskError:
        return ("error",)
    finally:
        op.close()


def view(data, offset, guard=b"\n@x\n+\n", behind=b"@next\nACGT\n+\nIIII\n"):
    """`data` in device memory at an address that is `offset` bytes behind a 128-byte line, the guard pattern in front of it
    (down to the start of the allocation) and the bytes of another shard behind it; returns (tensor to keep alive, pointer)"""
    import torch
    front = 256 + offset
    blob = (guard * (front // len(guard) + 1))[:front] + data + (behind * 40)
    t = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    assert t.data_ptr() % 128 == 0
    return t, t.data_ptr() + front


@pytest.mark.parametrize("sw", RANGES, ids=IDS)
@pytest.mark.parametrize("opname", ALL_OPS)
@pytest.mark.parametrize("which", sorted(INPUTS))
def test_every_residue_of_a_range_start(which, opname, sw):
    data = INPUTS[which]
    t, ptr = view(data, 0)
    got = run_ptr(opname, ptr, len(data), sw)
    assert got == want(opname, data), (which, opname, sw)
    assert got[0] == "ok"


OFFSETS = [0, 1, 15, 16, 17, 64, 112, 127, 128, 129]


@pytest.mark.parametrize("opname", ALL_OPS)
def test_views_at_odd_byte_offsets(opname):
    """The first range of a view that does not begin on a line has no line of its own to begin on: the grid keeps
    `rs & ~15` there and reads nothing in front of the pointer.  Two guards and two neighbours: the result depends on neither."""
    data = FIXED[:317 * 60]
    for off in OFFSETS:
        for guard, behind in ((b"\n@x\n+\n", b"@next\nACGT\n+\nIIII\n"), (b"\xff", b"\nACGTTGCAAGCT\n")):
            t, ptr = view(data, off, guard, behind)
            assert ptr % 128 == off % 128
            for sw in RANGES:
                assert run_ptr(opname, ptr, len(data), sw) == want(opname, data), (opname, off, guard, sw)


ENDS = {
    "n_not_a_multiple_of_16": FIXED[:317 * 37],                    # 11 729 bytes, whole records
    "no_final_newline": FIXED[:317 * 40 - 1],
    "stops_inside_a_quality_line": FIXED[:317 * 40 - 60],
    "shorter_than_a_line": fastq([40], 5),                          # 97 bytes
    "shorter_than_a_line_no_newline": fastq([40], 5)[:-1],
    "shorter_than_a_tile": FIXED[:317 * 9],                         # 2 853 bytes
    "a_tile_and_a_bit": FIXED[:317 * 13 - 1],                       # 4 120 bytes
    "variable_no_final_newline": VARIABLE[:-1],
}
assert len(ENDS["n_not_a_multiple_of_16"]) % 16 and len(ENDS["shorter_than_a_line"]) < 128 and len(ENDS["shorter_than_a_tile"]) < 4096


@pytest.mark.parametrize("opname", sorted(STATS_OPS))
@pytest.mark.parametrize("end", sorted(ENDS))
def test_ends_of_a_shard(end, opname):
    """the three `stats` passes (the error flags are theirs): the map, or that the shard is refused, is the oracle's -- at offsets
    0 and 17 and for every range size"""
    data = ENDS[end]
    for off in (0, 17):
        t, ptr = view(data, off)
        for sw in RANGES + [{}]:
            assert run_ptr(opname, ptr, len(data), sw) == want(opname, data), (end, opname, off, sw)


@pytest.mark.parametrize("sw", RANGES, ids=IDS)
def test_anchors_in_the_kernel_against_the_anchor_pass(sw):
    t, ptr = view(FIXED, 0)
    a = run_ptr("stats", ptr, len(FIXED), sw)
    b = run_ptr("stats", ptr, len(FIXED), dict(sw, stats_prep="pass"))
    assert a == b == want("stats", FIXED)
