"""`pair` in buckets of the key on the GPU (PARITY.md PAIRB; include/bsk.h bsk_pair_hist_run .. bsk_pair_order_bucket_finish): the
four outputs are those of the one-call bsk.Pair and of the oracle whatever the budget, the cut of the files into shards and the
order of file 2; both histograms, the pairs and the positions against the restatement in pair_buckets_ref.py; the smallest
shapes, the lanes of the comparison, a launch of many blocks, distinct subjects under one key, global indices past 2^32, empty
sides, wrapped input; misuse; the command line."""
import ctypes as C
import json
import os
import subprocess

import pytest

import bigseqkit_amd as bsk
from bigseqkit_amd import _lib
from bigseqkit_amd._lib import lib, check
import oracle
import pair_buckets_ref as P
import rmdup_buckets_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")
BINS = R.BINS
RANK_RECORDS = 32 * 256          # PAIRB_RANK_RECORDS (ops_pair_buckets.hpp): the records of one block of the rank's prefix counts
UNPAIRED = json.dumps({"SaveUnpaired": True})


class Opts:
    def __init__(self, d):
        self.d = dict(d)

    def to_json(self):
        return json.dumps(self.d)


def frame(data, fastq, parts=1):
    """`data` as 1, 3 or 7 shards that begin on record starts (7: a one-record shard and an empty one among them)"""
    fmt = bsk.FORMAT_FASTQ if fastq else bsk.FORMAT_FASTA
    cuts = R.cuts_of(data, fastq, parts)
    return bsk.SeqFrame(fmt, [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])])


def dev(data):
    import torch
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8) if len(data) else torch.empty(0, dtype=torch.uint8)
    return t.cuda()


def one_call_of(texts, fastq, o):
    fmt = bsk.FORMAT_FASTQ if fastq else bsk.FORMAT_FASTA
    return bsk.Pair(bsk.SeqFrame(fmt, [dev(texts[0])]), bsk.SeqFrame(fmt, [dev(texts[1])]), Opts(o))


def budget_of(hb, which):
    """which = 0, 1, 2: the three budgets of rmdup_buckets_ref; a number: that fraction of the whole, the fullest bin at least"""
    if isinstance(which, int):
        return R.budgets_of(hb)[which]
    return max(max(hb), int(sum(hb) * which) + 1)


def run(fa, fb, o, which=0, order="auto"):
    """the passes of bsk.PairBuckets, step by step, the budget of either phase taken from its own histogram"""
    res = {}
    with bsk.Operator("Pair", json.dumps(o), 0) as op:
        if order == "buckets":
            check(lib.bsk_ctx_set(op.ctx, b"pair_order", b"buckets"), op.ctx)
        bsk.PairHistReset(op)
        counts = bsk.PairHistRun(op, [fa, fb])
        res["hist"] = bsk.PairHistGet(op)
        n1, n2 = sum(counts[0]), sum(counts[1])
        bounds = bsk.ShufflePlan(res["hist"][0], budget_of(res["hist"][0], which)) if n1 + n2 else [0, BINS]
        bsk.PairVerdictBegin(op, [n1, n2])
        found = flagged = 0
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            k, fl = bsk.PairBucket(op, [fa, fb], counts, lo, hi)
            found, flagged = found + k, flagged + fl
        pairs, ordered = bsk.PairOrderBegin(op)
        assert found == pairs
        res.update(buckets=len(bounds) - 1, pairs=pairs, flagged=flagged, ordered=ordered, pos=bsk.PairVerdictGet(op, 0, n1 + n2))
        paired1, unpaired1, none = bsk.PairEmit(op, fa, counts[0], 0)
        none2, unpaired2, paired2 = bsk.PairEmit(op, fb, counts[1], n1)
        assert none == b"" and none2 == b""
        res["order_buckets"] = 0
        if pairs and (order == "buckets" or not ordered):
            assert paired2 == b""
            bsk.PairOrderHistRun(op, fb, counts[1], n1)
            res["order_hist"] = bsk.PairOrderHistGet(op)
            ob = bsk.ShufflePlan(res["order_hist"][0], budget_of(res["order_hist"][0], which))
            paired2 = b"".join(bsk.PairOrderBucket(op, fb, counts[1], n1, lo, hi) for lo, hi in zip(ob[:-1], ob[1:]))
            res["order_buckets"] = len(ob) - 1
        res["out"] = (paired1, paired2, unpaired1, unpaired2)
    return res


def expect(want, unpaired):
    return want if unpaired else want[:2] + (b"", b"")


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("mode", ("ordered auto", "ordered buckets", "shuffled auto"))
@pytest.mark.parametrize("unpaired", (True, False), ids=("unpaired", "pairs only"))
@pytest.mark.parametrize("name", R.SHAPES)
def test_buckets_equal_the_one_call_and_the_oracle(name, unpaired, mode):
    variant, order = mode.split()
    o = {"SaveUnpaired": unpaired}
    texts, fastq = P.files_text(name, variant)
    want = expect(P.want_of(name, variant, UNPAIRED), unpaired)
    assert one_call_of(texts, fastq, o) == want
    r = P.restated(name, variant)
    pair = r["pair"]
    for which, least in zip((0, 1, 2), (1, 8, 8)):
        for parts in (1, 3, 7):
            got = run(frame(texts[0], fastq, parts), frame(texts[1], fastq, parts), o, which, order)
            assert got["out"] == want, (which, parts)
            assert got["buckets"] >= least and (least > 1 or got["buckets"] == 1)
            assert got["flagged"] == 0 and got["pairs"] == pair[5]
            assert got["pos"] == P.pos_list(pair)
            assert got["hist"] == r["hist"]
            assert got["ordered"] == (variant == "ordered")
            if mode == "ordered auto":
                assert got["order_buckets"] == 0
            else:
                assert got["order_hist"] == r["order_hist"]
                assert got["order_buckets"] >= least and (least > 1 or got["order_buckets"] == 1)
    budget = R.budgets_of(r["hist"][0])[1]
    assert bsk.PairBuckets(frame(texts[0], fastq, 3), frame(texts[1], fastq, 3), Opts(o), budget_bytes=budget, order=order) == want


def test_line_width_and_id_rule():
    """LineWidth on FASTA, and the ID rule of the context: under --id-regexp the ID is what the expression captures"""
    texts, fastq = P.files_text("fasta 60", "shuffled")
    for o in ({"SaveUnpaired": True, "Config": {"LineWidth": 20}}, {"SaveUnpaired": True, "Config": {"LineWidth": 0}},
              {"SaveUnpaired": True, "Config": {"IDRegexp": "^(\\w\\d?)"}}):                         # (a few hundred records per ID)
        want = oracle.pair(texts[0], texts[1], fastq, json.dumps(o))
        got = run(frame(texts[0], fastq, 3), frame(texts[1], fastq, 3), o, 1)
        assert got["out"] == want == one_call_of(texts, fastq, o), o
        assert got["buckets"] >= 2 and got["flagged"] == 0


# ------------------------------------------------------------------ the smallest shapes
PATTERNS = ("file 2 equals file 1", "file 2 reversed", "file 2 holds every other ID", "one ID everywhere", "file 2 repeats one ID more often")


def pattern_ids(n, pattern):
    if pattern == "file 2 equals file 1":
        return list(range(n)), list(range(n))
    if pattern == "file 2 reversed":
        return list(range(n)), list(range(n))[::-1]
    if pattern == "file 2 holds every other ID":
        return list(range(n)), list(range(0, n, 2))
    if pattern == "one ID everywhere":
        return [0] * n, [0] * n
    return list(range(n)), [0] + list(range(n)) + [0]


@pytest.mark.parametrize("n", (1, 31, 32, 33, 2047, 2048, 2049, 4097, RANK_RECORDS + 1))
def test_smallest_shapes(n):
    """the records of a block of the 8-lane kernel (32), the bits of a word of the verdict (32), the tile of the scans (2048) and
    the block of the rank's prefix counts (RANK_RECORDS)"""
    for pattern in PATTERNS:
        ids = pattern_ids(n, pattern)
        files = [[(b"r%d" % i, seq) for i in f] for f, seq in zip(ids, (b"ACGT", b"TTGCA"))]
        pair = P.py_pair(*([h for h, _ in f] for f in files))
        for fastq, parts, which, order in ((True, 1, 0, "auto"), (False, 3, 0.25, "buckets")):
            texts = [P.tiny_text(f, fastq) for f in files]
            got = run(frame(texts[0], fastq, parts), frame(texts[1], fastq, parts), {"SaveUnpaired": True}, which, order)
            assert got["pos"] == P.pos_list(pair) and got["pairs"] == pair[5] and got["flagged"] == 0, (pattern, fastq)
            assert got["out"] == tuple(P.tiny_text(f, fastq) for f in P.py_outputs(*files)) == oracle.pair(texts[0], texts[1], fastq, UNPAIRED), (pattern, fastq)
            assert got["ordered"] == P.in_mate_order(pair[4])
            if pattern == "file 2 equals file 1":
                assert got["out"] == (texts[0], texts[1], b"", b"") and got["ordered"]
            if pattern == "file 2 reversed" and n > 1:
                assert not got["ordered"] and got["order_buckets"] >= 1
            if pattern == "one ID everywhere":
                assert got["pairs"] == n and got["out"][:2] == (texts[0], texts[1])
            if order == "buckets" and n >= 32:
                assert got["order_buckets"] >= 3 and (got["buckets"] >= 3 or pattern == "one ID everywhere")   # (one ID: one fine bin)


# ------------------------------------------------------------------ the lanes of the comparison
def test_comparison_lanes(monkeypatch):
    """IDs of 0 .. 257 bytes: 16 bytes per lane and step, 8 lanes, the bytes behind the last whole 16"""
    o = {"SaveUnpaired": True}
    lengths = P.LANE_LENGTHS
    head = lambda ident, tag: ident + tag if ident else b""                            # (an empty ID is an empty header)
    a = [(head(P.lane_id(L, L, b"A"), b" one"), b"ACGT") for L in lengths]
    same = [(head(P.lane_id(L, L, b"A"), b" two"), b"TTG") for L in lengths]
    last = [(head(P.lane_id(L, L, b"C"), b" two"), b"TTG") for L in lengths]         # (the empty ID has no last byte: equal)
    for other, n_pairs in ((same, len(lengths)), (last, 1)):
        texts = [R.fasta_text(a, 1000), R.fasta_text(other, 1000)]
        assert P.py_pair(*([R.subject(r, {}) for r in f] for f in (a, other)))[5] == n_pairs
        got = run(frame(texts[0], False), frame(texts[1], False), o)
        assert got["pairs"] == n_pairs and got["flagged"] == 0                         # a last byte that differs is another key
        assert got["out"] == oracle.pair(texts[0], texts[1], False, UNPAIRED) == one_call_of(texts, False, o)
    # under 16 bits of the key a pair that differs in its last byte only shares a key group: the comparison tells it apart
    pairs = [P.last_byte_collision(L) for L in lengths if L >= 2]
    a = [(b"", b"ACGT"), (b"G one", b"ACGT")] + [(s + b" one", b"ACGT") for s, t in pairs]
    b = [(b"", b"TTG"), (b"G two", b"TTG")] + [(t + b" two", b"TTG") for s, t in pairs]
    texts = [R.fasta_text(a, 1000), R.fasta_text(b, 1000)]
    want = oracle.pair(texts[0], texts[1], False, UNPAIRED)
    assert R.parse(want[0], False) == a[:2] and R.parse(want[3], False) == b[2:]
    monkeypatch.setenv("BSK_RMDUP_K1_BITS", "16")
    got = run(frame(texts[0], False), frame(texts[1], False), o)
    assert got["buckets"] == 1 and got["flagged"] == len(pairs) == 9                   # every t differs from the s in front of it
    assert got["pairs"] == 2 and got["out"] == want


# ------------------------------------------------------------------ distinct subjects under one key
def test_distinct_subjects_under_one_key_are_kept_apart(monkeypatch):
    files = P.masked_key_files()
    texts = [P.tiny_text(f, True) for f in files]
    want = oracle.pair(texts[0], texts[1], True, UNPAIRED)
    pair = P.py_pair(*([h for h, _ in f] for f in files))
    o = {"SaveUnpaired": True}
    plain = run(frame(texts[0], True, 3), frame(texts[1], True, 3), o, 0.34)
    assert plain["out"] == want and plain["flagged"] == 0 and plain["pos"] == P.pos_list(pair) and plain["pairs"] == 1500
    monkeypatch.setenv("BSK_RMDUP_K1_BITS", "16")                                    # 4500 subjects under 65 536 keys: some pairs collide
    got = run(frame(texts[0], True, 3), frame(texts[1], True, 3), o, 0.34)
    assert got["out"] == want and got["pos"] == plain["pos"]
    assert got["flagged"] > 0 and got["pairs"] == 1500
    assert got["hist"] == plain["hist"] and got["buckets"] == plain["buckets"] >= 3   # the bins come from the whole k1
    assert got["order_hist"] == plain["order_hist"] and got["order_buckets"] == plain["order_buckets"]


# ------------------------------------------------------------------ past one launch of many blocks
def test_many_blocks():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 3 * cus * 256 + 1234
    a = b"".join(b">%x\nA\n" % i for i in range(n))
    ids_b = list(range(0, n, 3))[::-1]
    b = b"".join(b">%x\nC\n" % i for i in ids_b)
    subs = [b"%x" % i for i in range(n)], [b"%x" % i for i in ids_b]
    pair = P.py_pair(*subs)
    got = run(frame(a, False), frame(b, False), {"SaveUnpaired": True}, 0.25)
    assert got["hist"] == R.py_hist(subs[0] + subs[1]) and got["buckets"] >= 4 and got["flagged"] == 0
    assert got["pairs"] == len(ids_b) == pair[5] and not got["ordered"] and got["pos"] == P.pos_list(pair)
    assert got["order_hist"] == P.order_hist(pair[4], [len(s) + 4 for s in subs[1]], pair[5]) and got["order_buckets"] >= 4
    assert got["out"] == oracle.pair(a, b, False, UNPAIRED)


# ------------------------------------------------------------------ global indices past 2^32
def test_indices_past_2_to_32():
    """the bits of 2^32 + 8 records of file 1 take 512 MB; the mate words hold indices past 2^32"""
    ids_a, ids_b = [1, 2, 3, 1, 4, 5, 2, 6], [7, 1, 8, 6, 6, 9, 3, 10]
    recs_a, recs_b = ([(b"r%d" % i, seq) for i in ids] for ids, seq in ((ids_a, b"ACGT"), (ids_b, b"TTG")))
    a, b = P.tiny_text(recs_a, True), P.tiny_text(recs_b, True)
    first_a, first_b = (1 << 32) - 3, (1 << 32) + 8
    pair = P.py_pair([b"r%d" % i for i in ids_a], [b"r%d" % i for i in ids_b])
    assert pair[3] == [0, None, 1, None, None, None, None, 2] and pair[4] == [None, 0, None, 2, None, None, 1, None]
    want = oracle.pair(a, b, True, UNPAIRED)

    def outs_of(op, text, first):
        outs = (_lib.Out * 3)()
        check(lib.bsk_pair_emit_run(op.ctx, text, len(text), 0, bsk.FORMAT_FASTQ, 0, first, None, outs), op.ctx)
        return [bsk.api._out_bytes(op, outs[k]) for k in range(3)]

    with bsk.Operator("Pair", UNPAIRED, 0) as op:
        bsk.PairVerdictBegin(op, [(1 << 32) + 8, 8])
        check(lib.bsk_pair_bucket_begin(op.ctx, 0, BINS), op.ctx)
        for text, first in ((a, first_a), (b, first_b)):
            check(lib.bsk_pair_bucket_add(op.ctx, text, len(text), 0, bsk.FORMAT_FASTQ, 0, first, None), op.ctx)
        found, flagged = C.c_uint64(), C.c_uint64()
        check(lib.bsk_pair_bucket_finish(op.ctx, None, C.byref(found), C.byref(flagged)), op.ctx)
        assert (found.value, flagged.value) == (3, 0)
        assert bsk.PairOrderBegin(op) == (3, False)
        assert bsk.PairVerdictGet(op, first_a - 5, 5 + 8 + 3) == [None] * 5 + pair[3] + [None] * 3
        assert bsk.PairVerdictGet(op, first_b, 8) == pair[4]
        assert bsk.PairVerdictGet(op, 0, 40) == [None] * 40                           # nothing wrapped round to the low indices
        assert outs_of(op, a, first_a) == [want[0], want[2], b""]
        assert outs_of(op, b, first_b) == [b"", want[3], b""]
        frame_b = bsk.SeqFrame(bsk.FORMAT_FASTQ, [b])
        bsk.PairOrderHistRun(op, frame_b, [8], first_b)
        assert sum(bsk.PairOrderHistGet(op)[1]) == 3
        assert bsk.PairOrderBucket(op, frame_b, [8], first_b, 0, BINS) == want[1] == P.tiny_text([recs_b[1], recs_b[6], recs_b[3]], True)


# ------------------------------------------------------------------ empty sides, wrapped input
def test_empty_sides():
    a = P.tiny_text([(b"r%d" % i, b"ACGT") for i in range(40)], True)
    b = P.tiny_text([(b"r%d" % i, b"TTG") for i in range(39, -1, -1)], True)
    fmt = bsk.FORMAT_FASTQ
    o = Opts({"SaveUnpaired": True})
    for x, y in ((b"", b), (a, b""), (b"", b"")):
        want = oracle.pair(x, y, True, UNPAIRED)
        assert want == (b"", b"", x, y)
        for order in ("auto", "buckets"):
            assert bsk.PairBuckets(frame(x, True), frame(y, True), o, budget_bytes=1 << 20, order=order) == want
        got = run(frame(x, True), frame(y, True), o.d)
        assert got["pairs"] == 0 and got["pos"] == [None] * ((x + y).count(b"\n") // 4)
    assert bsk.PairBuckets(bsk.SeqFrame(fmt, []), bsk.SeqFrame(fmt, [b]), o) == (b"", b"", b"", b)   # (a frame without a shard)
    assert bsk.PairBuckets(bsk.SeqFrame(fmt, [a]), bsk.SeqFrame(fmt, []), o) == (b"", b"", a, b"")
    with pytest.raises(ValueError):
        bsk.PairBuckets(bsk.SeqFrame(fmt, [a]), bsk.SeqFrame(bsk.FORMAT_FASTA, [b">x\nA\n"]))
    with pytest.raises(ValueError):
        bsk.PairBuckets(frame(a, True), frame(b, True), order="sorted")


def test_wrapped_input():
    """a wrapped FASTQ file 2 against a 4-line file 1: the multi-line reader in every pass over file 2; a FASTA file 1 without
    its final newline"""
    recs = P.files_records("fastq", "shuffled")
    rng = __import__("random").Random(1)
    a, b = R.fastq_text(rng, recs[0], 0), R.fastq_text(rng, recs[1], 7)
    o = {"SaveUnpaired": True}
    want = oracle.pair(a, b, True, UNPAIRED)
    for order in ("auto", "buckets"):
        got = run(frame(a, True, 3), frame(b, True, 3), o, 1, order)
        assert got["out"] == want and got["order_buckets"] >= 8 and got["buckets"] >= 8
        assert got["order_hist"] == P.order_hist(P.py_pair(*([R.subject(r, {}) for r in f] for f in recs))[4], [P.text_cost(r, True) for r in recs[1]], got["pairs"])
    texts, fastq = P.files_text("fasta 7", "shuffled")
    a = texts[0][:-1]
    want = oracle.pair(a, texts[1], False, UNPAIRED)
    assert want == P.want_of("fasta 7", "shuffled", UNPAIRED)
    assert run(frame(a, False, 3), frame(texts[1], False, 3), o, 1)["out"] == want


# ------------------------------------------------------------------ misuse and refusals
def test_refusals_and_misuse():
    texts, fastq = P.files_text("fastq", "shuffled")
    fa, fb = frame(texts[0], fastq), frame(texts[1], fastq)
    (pid, ptr, n, on_dev, keep), = fa.partitions()
    (pid2, ptr2, n2, on_dev2, keep2), = fb.partitions()
    fmt = fa.format
    err = lambda op: lib.bsk_last_error(op.ctx).decode()
    INV, UNS = _lib.BSK_ERR_INVALID_ARG, _lib.BSK_ERR_UNSUPPORTED
    k, r, fl, io = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
    want = P.want_of("fastq", "shuffled", UNPAIRED)
    hb = P.restated("fastq", "shuffled")["hist"][0]
    both = texts[0] + texts[1]

    with bsk.Operator("Pair", UNPAIRED, 0) as op:
        outs, out = (_lib.Out * 3)(), _lib.Out()
        word = (C.c_uint64 * 1)()
        assert lib.bsk_pair_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 0, None) == INV and "bsk_pair_bucket_add: no bucket is open" in err(op)
        assert lib.bsk_pair_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)) == INV and "no bucket is open" in err(op)
        assert lib.bsk_pair_bucket_begin(op.ctx, 0, BINS) == INV and "bsk_pair_verdict_begin first" in err(op)
        assert lib.bsk_pair_emit_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, outs) == INV and "bsk_pair_verdict_begin" in err(op)
        assert lib.bsk_pair_order_begin(op.ctx, None, C.byref(r), C.byref(io)) == INV and "no verdict" in err(op)
        assert lib.bsk_pair_verdict_get(op.ctx, 0, 1, word) == INV and "no verdict" in err(op)
        assert lib.bsk_pair_verdict_begin(op.ctx, None) == INV and "null argument" in err(op)
        assert lib.bsk_pair_bucket_begin(op.ctx, 5, 5) == INV and lib.bsk_pair_bucket_begin(op.ctx, 0, BINS + 1) == INV
        # the order calls before bsk_pair_order_begin
        for rc in (lib.bsk_pair_order_hist_run(op.ctx, ptr2, n2, 0, fmt, 0, 500, None, C.byref(k)), lib.bsk_pair_order_hist_get(op.ctx, None, None),
                   lib.bsk_pair_order_bucket_begin(op.ctx, 0, BINS), lib.bsk_pair_order_bucket_add(op.ctx, ptr2, n2, 0, fmt, 0, 500, None),
                   lib.bsk_pair_order_bucket_finish(op.ctx, None, C.byref(out))):
            assert rc == INV and "bsk_pair_order_begin first" in err(op)
        check(lib.bsk_pair_hist_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(k)), op.ctx)
        n_a = k.value
        check(lib.bsk_pair_hist_run(op.ctx, ptr2, n2, 0, fmt, 1, n_a, None, C.byref(k)), op.ctx)
        n_b = k.value
        assert (n_a, n_b) == (500, 500)
        bsk.PairVerdictBegin(op, [n_a, n_b])
        assert lib.bsk_pair_verdict_get(op.ctx, 0, 1, word) == INV and "bsk_pair_order_begin first" in err(op)
        check(lib.bsk_pair_bucket_begin(op.ctx, 0, 2048), op.ctx)
        assert lib.bsk_pair_bucket_begin(op.ctx, 2048, BINS) == INV and "a bucket is open" in err(op)
        assert lib.bsk_pair_verdict_begin(op.ctx, (C.c_uint64 * 2)(n_a, n_b)) == INV and "a bucket is open" in err(op)
        assert lib.bsk_pair_order_begin(op.ctx, None, C.byref(r), C.byref(io)) == INV and "a bucket is open" in err(op)
        # an add that is refused before it runs leaves the bucket usable
        assert lib.bsk_pair_bucket_add(op.ctx, ptr, n, 0, 99, 0, 0, None) == INV and "format" in err(op)
        assert lib.bsk_pair_bucket_add(op.ctx, None, n, 0, fmt, 0, 0, None) == INV and "null shard" in err(op)
        check(lib.bsk_pair_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 0, None), op.ctx)
        check(lib.bsk_pair_bucket_add(op.ctx, ptr2, n2, 0, fmt, 1, n_a, None), op.ctx)
        check(lib.bsk_pair_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)), op.ctx)
        # half of the bins are decided: the rank step and the emit name the first one that is not
        assert lib.bsk_pair_order_begin(op.ctx, None, C.byref(r), C.byref(io)) == INV and "bsk_pair_order_begin: fine bin 2048 has not been decided" in err(op)
        assert lib.bsk_pair_emit_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, outs) == INV and "fine bin 2048 has not been decided" in err(op)
        # the shards of a bucket arrive in input order: a first_record that goes backwards closes the bucket
        check(lib.bsk_pair_bucket_begin(op.ctx, 2048, BINS), op.ctx)
        half = R.cuts_of(texts[0], fastq, 3)[1]
        check(lib.bsk_pair_bucket_add(op.ctx, texts[0][:half], half, 0, fmt, 0, 100, None), op.ctx)
        assert lib.bsk_pair_bucket_add(op.ctx, texts[0][:half], half, 0, fmt, 0, 99, None) == INV and "goes backwards" in err(op)
        assert lib.bsk_pair_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)) == INV and "no bucket is open" in err(op)
        # a shard that reaches past the sum of file_records, and one that straddles the two files
        check(lib.bsk_pair_bucket_begin(op.ctx, 2048, BINS), op.ctx)
        assert lib.bsk_pair_bucket_add(op.ctx, ptr2, n2, 0, fmt, 0, n_a + 1, None) == INV
        assert "bsk_pair_bucket_add" in err(op) and "reach past the total_records = %d of bsk_pair_verdict_begin" % (n_a + n_b) in err(op)
        assert lib.bsk_pair_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)) == INV                          # ... has closed the bucket
        check(lib.bsk_pair_bucket_begin(op.ctx, 2048, BINS), op.ctx)
        assert lib.bsk_pair_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 1, None) == INV and "straddle the two files" in err(op)
        assert lib.bsk_pair_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)) == INV
        check(lib.bsk_pair_bucket_begin(op.ctx, 2048, BINS), op.ctx)                                             # (a bucket that was never finished wrote nothing)
        check(lib.bsk_pair_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 0, None), op.ctx)
        check(lib.bsk_pair_bucket_add(op.ctx, ptr2, n2, 0, fmt, 1, n_a, None), op.ctx)
        check(lib.bsk_pair_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)), op.ctx)
        # an emit before the rank step
        assert lib.bsk_pair_emit_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, outs) == INV and "bsk_pair_emit_run" in err(op) and "bsk_pair_order_begin first" in err(op)
        assert bsk.PairOrderBegin(op) == (len(R.parse(want[0], True)), False) == bsk.PairOrderBegin(op)         # (a second call reports the same)
        assert lib.bsk_pair_bucket_begin(op.ctx, 0, BINS) == INV and "has its positions already" in err(op)
        # shards of the emit: past the sum, astride the files
        assert lib.bsk_pair_emit_run(op.ctx, ptr2, n2, 0, fmt, 0, n_a + 1, None, outs) == INV and "reach past the sum of file_records = 1000" in err(op)
        assert lib.bsk_pair_emit_run(op.ctx, ptr, n, 0, fmt, 0, 1, None, outs) == INV and "straddle the two files" in err(op)
        assert lib.bsk_pair_verdict_get(op.ctx, n_a + n_b, 1, word) == INV and "reach past" in err(op)
        assert lib.bsk_pair_verdict_get(op.ctx, 0, 1, None) == INV and "null argument" in err(op)
        # the order phase: a shard of file 1, a first_record that goes backwards, a bucket that did not get every shard
        assert lib.bsk_pair_order_hist_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(k)) == INV and "lies in file 1" in err(op)
        assert lib.bsk_pair_order_bucket_add(op.ctx, ptr2, n2, 0, fmt, 0, n_a, None) == INV and "bsk_pair_order_bucket_add: no bucket is open" in err(op)
        assert lib.bsk_pair_order_bucket_finish(op.ctx, None, C.byref(out)) == INV and "no bucket is open" in err(op)
        assert lib.bsk_pair_order_bucket_finish(op.ctx, None, None) == INV
        assert lib.bsk_pair_order_bucket_begin(op.ctx, 7, 7) == INV and "0 <= lo < hi <= 4096" in err(op)
        check(lib.bsk_pair_order_bucket_begin(op.ctx, 0, BINS), op.ctx)
        assert lib.bsk_pair_order_bucket_begin(op.ctx, 0, BINS) == INV and "a bucket is open" in err(op)
        cut = R.cuts_of(texts[1], fastq, 3)[1]
        check(lib.bsk_pair_order_bucket_add(op.ctx, texts[1][cut:], len(texts[1]) - cut, 0, fmt, 0, n_a + 166, None), op.ctx)
        assert lib.bsk_pair_order_bucket_add(op.ctx, texts[1][:cut], cut, 0, fmt, 0, n_a, None) == INV and "bsk_pair_order_bucket_add" in err(op) and "goes backwards" in err(op)
        assert lib.bsk_pair_order_bucket_finish(op.ctx, None, C.byref(out)) == INV and "no bucket is open" in err(op)
        check(lib.bsk_pair_order_bucket_begin(op.ctx, 0, BINS), op.ctx)
        check(lib.bsk_pair_order_bucket_add(op.ctx, texts[1][cut:], len(texts[1]) - cut, 0, fmt, 0, n_a + 166, None), op.ctx)
        assert lib.bsk_pair_order_bucket_finish(op.ctx, None, C.byref(out)) == INV and "records of paired.2 whose positions lie in its bins" in err(op)
        # the context is whole after all that
        bsk.PairOrderHistRun(op, fb, [n_b], n_a)
        p1, u1, none = bsk.PairEmit(op, fa, [n_a], 0)
        none2, u2, p2 = bsk.PairEmit(op, fb, [n_b], n_a)
        assert (p1, bsk.PairOrderBucket(op, fb, [n_b], n_a, 0, BINS), u1, u2) == want and none == none2 == p2 == b""
        assert bsk.PairVerdictGet(op, 0, n_a + n_b) == P.pos_list(P.restated("fastq", "shuffled")["pair"])
        bsk.PairVerdictBegin(op, [n_a, n_b])                                                                     # a new verdict forgets the decided bins
        assert lib.bsk_pair_emit_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, outs) == INV and "fine bin 0 has not been decided" in err(op)
        # the one call still runs on a context that has been through the buckets
        outs4 = (_lib.Out * 4)()
        check(lib.bsk_pair_run(op.ctx, both, len(both), len(texts[0]), 0, fmt, None, outs4), op.ctx)
        assert tuple(bsk.api._out_bytes(op, outs4[j]) for j in range(4)) == want
    # a single bin above the budget: the plan's refusal
    with pytest.raises(bsk.BskError) as e:
        bsk.PairBuckets(fa, fb, budget_bytes=max(hb) - 1)
    assert e.value.code == UNS and "budget of %d bytes" % (max(hb) - 1) in str(e.value)
    # out=slices on the emit is refused; the one call is what it was
    os.environ["BSK_OUT"] = "slices"
    try:
        assert one_call_of(texts, fastq, {"SaveUnpaired": True}) == want
        with pytest.raises(bsk.BskError) as e:
            bsk.PairBuckets(fa, fb, budget_bytes=R.budgets_of(hb)[1])
        assert e.value.code == UNS and "bsk_pair_emit_run: out=slices" in str(e.value)
    finally:
        del os.environ["BSK_OUT"]
    # every entry point on a context of another operator -- and the siblings' on a Pair context
    arr = (C.c_uint64 * 2)(10, 10)
    for other in ("Shuffle", "RmDup", "Rename", "Common"):
        with bsk.Operator(other, "{}", 0) as op:
            out, outs = _lib.Out(), (_lib.Out * 3)()
            for rc in (lib.bsk_pair_hist_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(k)),
                       lib.bsk_pair_hist_get(op.ctx, None, None),
                       lib.bsk_pair_hist_reset(op.ctx),
                       lib.bsk_pair_verdict_begin(op.ctx, arr),
                       lib.bsk_pair_verdict_get(op.ctx, 0, 1, (C.c_uint64 * 1)()),
                       lib.bsk_pair_bucket_begin(op.ctx, 0, BINS),
                       lib.bsk_pair_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 0, None),
                       lib.bsk_pair_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)),
                       lib.bsk_pair_order_begin(op.ctx, None, C.byref(r), C.byref(io)),
                       lib.bsk_pair_emit_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, outs),
                       lib.bsk_pair_order_hist_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(k)),
                       lib.bsk_pair_order_hist_get(op.ctx, None, None),
                       lib.bsk_pair_order_bucket_begin(op.ctx, 0, BINS),
                       lib.bsk_pair_order_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 0, None),
                       lib.bsk_pair_order_bucket_finish(op.ctx, None, C.byref(out))):
                assert rc == INV and "not a Pair context" in err(op)
    with bsk.Operator("Pair", "{}", 0) as op:
        out = _lib.Out()
        for prefix, message, word in (("bsk_rmdup", "not an RmDup context", C.c_uint8), ("bsk_rename", "not a Rename context", C.c_uint32),
                                      ("bsk_common", "not a Common context", C.c_uint8)):
            fn = lambda name: getattr(lib, prefix + "_" + name)
            for rc in (fn("hist_run")(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(k)),
                       fn("hist_get")(op.ctx, None, None),
                       fn("hist_reset")(op.ctx),
                       fn("verdict_begin")(op.ctx, arr, 2) if prefix == "bsk_common" else fn("verdict_begin")(op.ctx, 10),
                       fn("verdict_get")(op.ctx, 0, 1, (word * 1)()),
                       fn("bucket_begin")(op.ctx, 0, BINS),
                       fn("bucket_add")(op.ctx, ptr, n, 0, fmt, 0, 0, None),
                       fn("bucket_finish")(op.ctx, None, C.byref(r), C.byref(fl)),
                       fn("emit_run")(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(out))):
                assert rc == INV and message in err(op)


# ------------------------------------------------------------------ the command line
@pytest.mark.parametrize("variant", P.VARIANTS)
def test_cli_pair_in_buckets(tmp_path, variant):
    texts, fastq = P.files_text("fastq", variant)
    r = P.restated("fastq", variant)
    paths = [str(tmp_path / x) for x in ("reads_1.fq", "reads_2.fq")]
    for path, text in zip(paths, texts):
        open(path, "wb").write(text)
    names = ("paired.1", "paired.2", "unpaired.1", "unpaired.2")

    def files_of(d):
        return tuple(open(os.path.join(d, x), "rb").read() if os.path.exists(os.path.join(d, x)) else None for x in names)

    budget = max(max(r["hist"][0]), sum(r["hist"][0]) // 4, max(r["order_hist"][0]))
    assert len(bsk.ShufflePlan(r["hist"][0], budget)) - 1 >= 3 and len(bsk.ShufflePlan(r["order_hist"][0], budget)) - 1 >= 3
    for flags, unpaired in (([], False), (["-u"], True)):
        want = expect(P.want_of("fastq", variant, UNPAIRED), unpaired)
        plain, bucketed = str(tmp_path / ("plain%d" % unpaired)), str(tmp_path / ("buckets%d" % unpaired))
        p = subprocess.run([CLI, "pair", *paths, "-O", plain, *flags], capture_output=True, timeout=900, env=dict(os.environ, BSK_CLI_TIMING="1"))
        assert p.returncode == 0 and "k_rdb_hist" not in p.stderr.decode(), p.stderr.decode()   # the whole-file run, as before
        env = dict(os.environ, BSK_CLI_TIMING="1", BSK_STREAM_PIECE_BYTES="4096", BSK_PAIR_BUDGET_BYTES=str(budget))
        p = subprocess.run([CLI, "pair", *paths, "-O", bucketed, *flags], capture_output=True, timeout=900, env=env)
        assert p.returncode == 0, p.stderr.decode()
        got = files_of(bucketed)
        assert got == files_of(plain), flags
        assert got[:2] == want[:2] and (not unpaired or got[2:] == want[2:])
        err = p.stderr.decode()
        assert all(s in err for s in ("k_rdb_hist", "k_rdb_pick", "k_pairb_verify", "k_pairb_rank", "k_pairb_apply")), err[-800:]
        assert ("k_pairb_order_pick" in err) == (variant == "shuffled")
        assert "pair: %d pair(s), 0 flagged" % r["pair"][5] in err
    p = subprocess.run([CLI, "pair", *paths], capture_output=True, timeout=900, env=dict(os.environ, BSK_PAIR_BUDGET_BYTES=str(budget)))
    assert p.returncode != 0 and "out-dir required" in p.stderr.decode()
    p = subprocess.run([CLI, "pair", paths[0], "-O", str(tmp_path / "x")], capture_output=True, timeout=900, env=dict(os.environ, BSK_PAIR_BUDGET_BYTES=str(budget)))
    assert p.returncode != 0 and "2 files needed" in p.stderr.decode()
