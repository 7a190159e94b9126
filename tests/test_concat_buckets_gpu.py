"""`concat` in buckets of the key on the GPU (PARITY.md CONB; include/bsk.h bsk_concat_hist_run .. bsk_concat_tail_run): the output
is that of the one-call bsk.Concat and of the oracle whatever the budget, the cut of the files into shards and the order of file
2; both histograms and the heads against the restatement in concat_buckets_ref.py; the smallest shapes, an ID in several windows,
Full and empty sides, distinct subjects under one key, the lanes of the comparison, wrapped input, global indices past 2^32;
misuse; the command line."""
import ctypes as C
import json
import os
import subprocess

import pytest

import bigseqkit_amd as bsk
from bigseqkit_amd import _lib
from bigseqkit_amd._lib import lib, check
import concat_buckets_ref as K
import oracle
import pair_buckets_ref as P
import rmdup_buckets_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")
BINS = R.BINS
FULL = json.dumps({"Full": True})


class Opts:
    def __init__(self, d):
        self.d = dict(d)

    def to_json(self):
        return json.dumps(self.d)


def fmt_of(fastq):
    return bsk.FORMAT_FASTQ if fastq else bsk.FORMAT_FASTA


def frame(data, fastq, parts=1):
    """`data` as 1, 3 or 7 shards that begin on record starts (7: a one-record shard and an empty one among them)"""
    cuts = R.cuts_of(data, fastq, parts)
    return bsk.SeqFrame(fmt_of(fastq), [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])])


def frame_of_pieces(data, fastq, piece=4096):
    """`data` as shards of whole records, a new one as soon as the running one has reached `piece` bytes"""
    starts = [s for s, _ in oracle.record_spans(data, fastq)] + [len(data)]
    cuts = [0]
    for s in starts[1:]:
        if s - cuts[-1] >= piece or s == len(data):
            cuts.append(s)
    return bsk.SeqFrame(fmt_of(fastq), [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])])


def dev(data):
    import torch
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8) if len(data) else torch.empty(0, dtype=torch.uint8)
    return t.cuda()


def one_call_of(texts, fastq, o):
    fmt = fmt_of(fastq)
    return bsk.Concat(bsk.SeqFrame(fmt, [dev(texts[0])]), bsk.SeqFrame(fmt, [dev(texts[1])]), Opts(o))


def run(fa, fb, o, fraction=1.0):
    """the passes of bsk.ConcatBuckets, step by step, the budget of either phase taken from its own histogram: about 1 / fraction
    buckets and windows"""
    res = {}
    with bsk.Operator("Concat", json.dumps(o), 0) as op:
        bsk.ConcatHistReset(op)
        counts = bsk.ConcatHistRun(op, [fa, fb])
        res["hist"] = bsk.ConcatHistGet(op)
        n1, n2 = sum(counts[0]), sum(counts[1])
        bounds = bsk.ShufflePlan(res["hist"][0], K.budget_of(res["hist"][0], fraction)) if n1 + n2 else [0, BINS]
        bsk.ConcatVerdictBegin(op, [n1, n2])
        matched = flagged = 0
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            k, fl = bsk.ConcatBucket(op, [fa, fb], counts, lo, hi)
            matched, flagged = matched + k, flagged + fl
        bsk.ConcatJoinBegin(op)
        res.update(buckets=len(bounds) - 1, matched=matched, flagged=flagged, head=bsk.ConcatVerdictGet(op, 0, n1 + n2), n1=n1)
        bsk.ConcatWeighRun(op, fb, counts[1], n1)
        bsk.ConcatWindowHistRun(op, fa, counts[0])
        res["whist"] = bsk.ConcatWindowHistGet(op)
        wb = bsk.ShufflePlan(res["whist"][0], K.budget_of(res["whist"][0], fraction)) if n1 else [0, BINS]
        res["shares"] = [bsk.ConcatWindow(op, [fa, fb], counts, lo, hi) for lo, hi in zip(wb[:-1], wb[1:])]
        res["wbounds"] = wb
        res["windows"] = len(wb) - 1
        res["tail"] = bsk.ConcatTail(op, fb, counts[1], n1)
        res["out"] = b"".join(res["shares"]) + res["tail"]
    return res


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("full", (False, True), ids=("joined only", "full"))
@pytest.mark.parametrize("variant", P.VARIANTS)
@pytest.mark.parametrize("name", R.SHAPES)
def test_buckets_equal_the_one_call_and_the_oracle(name, variant, full):
    o = {"Full": full}
    texts, fastq = P.files_text(name, variant)
    want = K.want_of(name, variant, json.dumps(o))
    assert one_call_of(texts, fastq, o) == want and want
    r = K.restated(name, variant)
    for fraction, parts in ((1.0, 1), (0.25, 3), (0.1, 7)):
        got = run(frame(texts[0], fastq, parts), frame(texts[1], fastq, parts), o, fraction)
        assert got["out"] == want, (fraction, parts)
        assert got["head"] == r["head"] and got["flagged"] == 0
        assert got["matched"] == sum(1 for h in r["head"] if h is not None)
        assert got["hist"] == r["hist"] and got["whist"] == r["whist"]
        if fraction < 1:
            assert got["buckets"] >= 3 and got["windows"] >= 3
        else:
            assert got["buckets"] == 1 and got["windows"] == 1
        if not full:
            assert got["tail"] == b""
    budget = max(max(r["hist"][0]), max(r["whist"][0]), sum(r["hist"][0]) // 4)      # one budget plans both phases
    assert len(bsk.ShufflePlan(r["hist"][0], budget)) - 1 >= 3 and len(bsk.ShufflePlan(r["whist"][0], budget)) - 1 >= 3
    assert bsk.ConcatBuckets(frame(texts[0], fastq, 3), frame(texts[1], fastq, 3), Opts(o), budget_bytes=budget) == want


def test_line_width_and_id_rule():
    """LineWidth on FASTA, and the ID rule of the context: under --id-regexp the ID is what the expression captures"""
    texts, fastq = P.files_text("fasta 60", "shuffled")
    for o in ({"Full": True, "Config": {"LineWidth": 0}}, {"Full": True, "Config": {"LineWidth": 13}}, {"Full": False, "Config": {"LineWidth": 60}},
              {"Full": True, "Config": {"IDRegexp": "^(\\w\\d?)"}}):                                 # (a few dozen records per ID)
        want = oracle.concat(texts[0], texts[1], fastq, json.dumps(o))
        got = run(frame(texts[0], fastq, 3), frame(texts[1], fastq, 3), o, 0.25)
        assert got["out"] == want == one_call_of(texts, fastq, o), o
        assert got["flagged"] == 0 and got["windows"] >= 3 and (got["buckets"] >= 3 or "IDRegexp" in o["Config"])


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


@pytest.mark.parametrize("n", (1, 31, 32, 33, 2047, 2048, 2049, 4097, 8193))
def test_smallest_shapes(n):
    """the records of a block of the 8-lane kernel (32), the bits of a word of the marks (32), the tile of the scans (2048) and
    the shifts 1 and 2 of the window bins (4097, 8193 records in file 1)"""
    assert K.window_shift(n) == {4097: 1, 8193: 2}.get(n, 0)
    for pattern in PATTERNS:
        if pattern == "one ID everywhere" and n > 33:                                 # (the product stays at 33 * 33 elements)
            continue
        ids = pattern_ids(n, pattern)
        files = [[(b"r%d" % i, seq) for i in f] for f, seq in zip(ids, (b"ACGT", b"TTGCA"))]
        subs = [[h for h, _ in f] for f in files]
        head = K.py_head(*subs)
        for fastq, parts, fraction, full in ((True, 1, 1.0, True), (False, 3, 0.25, False)):
            texts = [P.tiny_text(f, fastq) for f in files]
            costs = [[P.text_cost(r, fastq) for r in f] for f in files]
            Cw, Ww = K.py_weights(head, n, costs[1])
            got = run(frame(texts[0], fastq, parts), frame(texts[1], fastq, parts), {"Full": full}, fraction)
            assert got["head"] == head and got["flagged"] == 0, (pattern, fastq)
            assert got["hist"] == R.py_hist(subs[0] + subs[1]), (pattern, fastq)
            assert got["whist"] == K.window_hist(K.py_costs(head, Cw, Ww, costs[0])), (pattern, fastq)
            assert got["out"] == one_call_of(texts, fastq, {"Full": full}), (pattern, fastq)
            if n <= 33:
                assert got["out"] == oracle.concat(texts[0], texts[1], fastq, json.dumps({"Full": full}))
            if pattern == "one ID everywhere":
                assert got["out"].count(b"\n") == (4 if fastq else 2) * n * n
            if fraction < 1 and n >= 32:
                assert got["windows"] >= 3 and (got["buckets"] >= 3 or pattern == "one ID everywhere")   # (one ID: one fine bin)


# ------------------------------------------------------------------ an ID in several windows
def test_an_id_that_occurs_in_several_windows():
    """the same ID at the first and the last record of file 1, windows cut between them: its mates of file 2 appear in both
    shares and in no other"""
    ids_a, ids_b = [0, 1, 2, 3, 4, 0], [5, 0, 2, 0, 4]
    recs_a, recs_b = [(b"r%d" % i, b"ACGT") for i in ids_a], [(b"r%d" % i, b"TT" + b"G" * k) for k, i in enumerate(ids_b)]
    for fastq in (True, False):
        a, b = P.tiny_text(recs_a, fastq), P.tiny_text(recs_b, fastq)
        head = K.py_head([h for h, _ in recs_a], [h for h, _ in recs_b])
        fa, fb = frame(a, fastq), frame(b, fastq)
        with bsk.Operator("Concat", FULL, 0) as op:
            counts = bsk.ConcatHistRun(op, [fa, fb])
            bsk.ConcatVerdictBegin(op, [6, 5])
            assert bsk.ConcatBucket(op, [fa, fb], counts, 0, BINS) == (6 + 4, 0)
            bsk.ConcatJoinBegin(op)
            assert bsk.ConcatVerdictGet(op, 0, 11) == head == [0, 1, 2, 3, 4, 0, None, 0, 2, 0, 4]
            bsk.ConcatWeighRun(op, fb, counts[1], 6)
            bsk.ConcatWindowHistRun(op, fa, counts[0])
            shares = [bsk.ConcatWindow(op, [fa, fb], counts, lo, hi) for lo, hi in ((0, 2), (2, 5), (5, BINS))]
            tail = bsk.ConcatTail(op, fb, counts[1], 6)
        one, two = K.record_texts(a, fastq), K.record_texts(b, fastq)
        for share, (lo, hi) in zip(shares, ((0, 2), (2, 5), (5, BINS))):
            ia, ib = K.window_members(head, 6, lo, hi)
            assert share == oracle.concat(b"".join(one[i] for i in ia), b"".join(two[j] for j in ib), fastq, FULL)
        mark = b"@r0\n" if fastq else b">r0\n"
        assert [s.count(mark) for s in shares] == [2, 0, 2]                           # r0 x (b[1], b[3]) in the first and the last share
        assert b"".join(shares) + tail == oracle.concat(a, b, fastq, FULL) == one_call_of((a, b), fastq, {"Full": True})
        assert tail == two[0]


# ------------------------------------------------------------------ Full, empty sides
def test_full_and_empty_sides():
    recs_a = [(b"r%d left" % i, b"ACGT") for i in range(40)]
    recs_b = [(b"r%d right" % i, b"TTG") for i in range(78, -1, -2)]                 # r0 .. r38 have a mate, r40 .. r78 have none
    a, b = P.tiny_text(recs_a, True), P.tiny_text(recs_b, True)
    got = run(frame(a, True, 3), frame(b, True, 3), {"Full": True}, 0.2)
    assert got["windows"] >= 3 and got["out"] == oracle.concat(a, b, True, FULL) == one_call_of((a, b), True, {"Full": True})
    # the unmatched records of file 1 in place, those of file 2 in the tail only
    assert got["tail"] == P.tiny_text(recs_b[:20], True) and all(b"right" not in s for s in got["shares"])
    heads = [ln for ln in b"".join(got["shares"]).split(b"\n") if ln.startswith(b"@")]
    assert heads == [b"@r%d" % i if i % 2 == 0 else b"@r%d left" % i for i in range(40)]
    plain = run(frame(a, True, 3), frame(b, True, 3), {"Full": False}, 0.2)
    assert plain["tail"] == b"" and plain["out"] == oracle.concat(a, b, True, "{}") and plain["out"].count(b"@") == 20
    fmt = bsk.FORMAT_FASTQ
    for x, y in ((b"", b), (a, b""), (b"", b"")):
        for full in (True, False):
            want = oracle.concat(x, y, True, json.dumps({"Full": full})) if x + y else b""
            assert want == ((x + y) if full else b"")
            assert bsk.ConcatBuckets(frame(x, True), frame(y, True), Opts({"Full": full}), budget_bytes=1 << 20) == want
            got = run(frame(x, True), frame(y, True), {"Full": full})
            assert got["out"] == want and got["matched"] == x.count(b"\n") // 4
    assert bsk.ConcatBuckets(bsk.SeqFrame(fmt, []), bsk.SeqFrame(fmt, [b]), Opts({"Full": True})) == b   # (a frame without a shard)
    assert bsk.ConcatBuckets(bsk.SeqFrame(fmt, [a]), bsk.SeqFrame(fmt, []), Opts({"Full": True})) == a
    with pytest.raises(ValueError):
        bsk.ConcatBuckets(bsk.SeqFrame(fmt, [a]), bsk.SeqFrame(bsk.FORMAT_FASTA, [b">x\nA\n"]))


# ------------------------------------------------------------------ distinct subjects under one key
def test_distinct_subjects_under_one_key_are_kept_apart(monkeypatch):
    files = P.masked_key_files()
    texts = [P.tiny_text(f, True) for f in files]
    subs = [[h for h, _ in f] for f in files]
    want = oracle.concat(texts[0], texts[1], True, FULL)
    head = K.py_head(*subs)
    plain = run(frame(texts[0], True, 3), frame(texts[1], True, 3), {"Full": True}, 0.34)
    assert plain["out"] == want and plain["flagged"] == 0 and plain["head"] == head and plain["matched"] == 3000 + 1500
    monkeypatch.setenv("BSK_RMDUP_K1_BITS", "16")                                    # 4500 subjects under 65 536 keys: some collide
    got = run(frame(texts[0], True, 3), frame(texts[1], True, 3), {"Full": True}, 0.34)
    # one bucket sees every key group: the flagged records are the restatement's
    whole = run(frame(texts[0], True), frame(texts[1], True), {"Full": True})
    assert whole["buckets"] == 1 and whole["flagged"] == P.masked_groups(*subs)[0] > 0
    assert got["flagged"] > 0 and got["head"] == whole["head"] == head and got["matched"] == whole["matched"] == plain["matched"]
    assert got["out"] == whole["out"] == want
    assert got["hist"] == plain["hist"] and got["buckets"] == plain["buckets"] >= 3   # the bins come from the whole k1
    assert got["whist"] == plain["whist"] and got["windows"] == plain["windows"] >= 3


# ------------------------------------------------------------------ the lanes of the comparison
def test_comparison_lanes(monkeypatch):
    """IDs of 0 .. 257 bytes: 16 bytes per lane and step, 8 lanes, the bytes behind the last whole 16"""
    lengths = P.LANE_LENGTHS
    head = lambda ident, tag: ident + tag if ident else b""                            # (an empty ID is an empty header)
    a = [(head(P.lane_id(L, L, b"A"), b" one"), b"ACGT") for L in lengths]
    same = [(head(P.lane_id(L, L, b"A"), b" two"), b"TTG") for L in lengths]
    last = [(head(P.lane_id(L, L, b"C"), b" two"), b"TTG") for L in lengths]         # (the empty ID has no last byte: equal)
    for other, joined in ((same, len(lengths)), (last, 1)):
        texts = [R.fasta_text(a, 1000), R.fasta_text(other, 1000)]
        got = run(frame(texts[0], False), frame(texts[1], False), {"Full": True})
        assert got["flagged"] == 0 and got["matched"] == len(lengths) + joined      # a last byte that differs is another key
        assert got["out"] == oracle.concat(texts[0], texts[1], False, FULL) == one_call_of(texts, False, {"Full": True})
    # under 16 bits of the key a pair that differs in its last byte only shares a key group: the comparison tells it apart
    pairs = [P.last_byte_collision(L) for L in lengths if L >= 2]
    a = [(b"", b"ACGT"), (b"G one", b"ACGT")] + [(s + b" one", b"ACGT") for s, t in pairs]
    b = [(b"", b"TTG"), (b"G two", b"TTG")] + [(t + b" two", b"TTG") for s, t in pairs]
    texts = [R.fasta_text(a, 1000), R.fasta_text(b, 1000)]
    want = oracle.concat(texts[0], texts[1], False, FULL)
    assert R.parse(want, False) == [(b"", b"ACGTTTG"), (b"G", b"ACGTTTG")] + a[2:] + b[2:]   # not joined
    monkeypatch.setenv("BSK_RMDUP_K1_BITS", "16")
    got = run(frame(texts[0], False), frame(texts[1], False), {"Full": True})
    assert got["buckets"] == 1 and got["flagged"] == len(pairs) == 9                   # every t differs from the s in front of it
    assert got["matched"] == len(a) + 2 and got["out"] == want
    assert got["head"] == list(range(len(a))) + [0, 1] + [None] * len(pairs)


# ------------------------------------------------------------------ wrapped input in small shards
@pytest.mark.parametrize("name", ("fastq wrapped", "fasta 7"))
def test_wrapped_input_in_4k_shards(name):
    texts, fastq = P.files_text(name, "shuffled")
    r = K.restated(name, "shuffled")
    fa, fb = (frame_of_pieces(t, fastq, 4096) for t in texts)
    assert len(fa.shards) >= 5 and len(fb.shards) >= 5
    for full in (True, False):
        got = run(fa, fb, {"Full": full}, 0.2)
        assert got["out"] == K.want_of(name, "shuffled", json.dumps({"Full": full}))
        assert got["head"] == r["head"] and got["whist"] == r["whist"] and got["windows"] >= 3 and got["buckets"] >= 3
    # a FASTA file 1 without its final newline
    if not fastq:
        a = texts[0][:-1]
        assert run(frame(a, False, 3), frame(texts[1], False, 3), {"Full": True}, 0.25)["out"] == K.want_of(name, "shuffled", FULL)


# ------------------------------------------------------------------ global indices past 2^32
def test_indices_past_2_to_32():
    """the heads of 2^32 + 16 records take 32 GiB, the weights of file 1 twice as much: the words hold indices past 2^32, the
    shift of the window bins is 21 and the shard of file 1 lies astride two bins"""
    ids_a, ids_b = [1, 2, 3, 1, 4, 5, 2, 6], [7, 1, 8, 6, 6, 9, 3, 10]
    recs_a, recs_b = ([(b"r%d" % i, seq) for i in ids] for ids, seq in ((ids_a, b"ACGT"), (ids_b, b"TTG")))
    a, b = P.tiny_text(recs_a, True), P.tiny_text(recs_b, True)
    first_a, n1 = (1 << 32) - 3, (1 << 32) + 8
    small = K.py_head([h for h, _ in recs_a], [h for h, _ in recs_b])
    assert small == [0, 1, 2, 0, 4, 5, 1, 7, None, 0, None, 7, 7, None, 2, None]
    head = [None if h is None else first_a + h for h in small]
    assert K.window_shift(n1) == 21 and first_a >> 21 == 2047 and (first_a + 3) >> 21 == 2048
    want = oracle.concat(a, b, True, FULL)
    fmt = bsk.FORMAT_FASTQ
    fa, fb = bsk.SeqFrame(fmt, [a]), bsk.SeqFrame(fmt, [b])
    with bsk.Operator("Concat", FULL, 0) as op:
        bsk.ConcatVerdictBegin(op, [n1, 8])
        check(lib.bsk_concat_bucket_begin(op.ctx, 0, BINS), op.ctx)
        for text, first in ((a, first_a), (b, n1)):
            check(lib.bsk_concat_bucket_add(op.ctx, text, len(text), 0, fmt, 0, first, None), op.ctx)
        matched, flagged = C.c_uint64(), C.c_uint64()
        check(lib.bsk_concat_bucket_finish(op.ctx, None, C.byref(matched), C.byref(flagged)), op.ctx)
        assert (matched.value, flagged.value) == (8 + 4, 0)
        bsk.ConcatJoinBegin(op)
        assert bsk.ConcatVerdictGet(op, first_a - 5, 5 + 8 + 3) == [None] * 5 + head[:8] + [None] * 3
        assert bsk.ConcatVerdictGet(op, n1, 8) == head[8:]
        assert bsk.ConcatVerdictGet(op, 0, 40) == [None] * 40                         # nothing wrapped round to the low indices
        bsk.ConcatWeighRun(op, fb, [8], n1)
        k = C.c_uint64()
        check(lib.bsk_concat_window_hist_run(op.ctx, a, len(a), 0, fmt, 0, first_a, None, C.byref(k)), op.ctx)
        hb, hr = bsk.ConcatWindowHistGet(op)
        assert hr[2047] == 3 and hr[2048] == 5 and sum(hr) == 8
        costs = [[P.text_cost(r, True) for r in f] for f in (recs_a, recs_b)]
        Cw, Ww = K.py_weights(small, 8, costs[1])
        cost = K.py_costs(small, Cw, Ww, costs[0])
        assert (hb[2047], hb[2048]) == (sum(cost[:3]), sum(cost[3:])) and sum(hb) == sum(cost)
        shares = []
        for lo, hi in ((0, 2048), (2048, BINS)):
            check(lib.bsk_concat_window_begin(op.ctx, lo, hi), op.ctx)
            for text, first in ((a, first_a), (b, n1)):
                check(lib.bsk_concat_window_add(op.ctx, text, len(text), 0, fmt, 0, first, None), op.ctx)
            out = _lib.Out()
            check(lib.bsk_concat_window_finish(op.ctx, None, C.byref(out)), op.ctx)
            shares.append(bsk.api._out_bytes(op, out))
        assert all(shares) and b"".join(shares) + bsk.ConcatTail(op, fb, [8], n1) == want


# ------------------------------------------------------------------ misuse and refusals
def test_refusals_and_misuse():
    texts, fastq = P.files_text("fastq", "shuffled")
    fa, fb = frame(texts[0], fastq), frame(texts[1], fastq)
    (pid, ptr, n, on_dev, keep), = fa.partitions()
    (pid2, ptr2, n2, on_dev2, keep2), = fb.partitions()
    fmt = fa.format
    err = lambda op: lib.bsk_last_error(op.ctx).decode()
    INV, UNS = _lib.BSK_ERR_INVALID_ARG, _lib.BSK_ERR_UNSUPPORTED
    k, r, fl = C.c_uint64(), C.c_uint64(), C.c_uint64()
    want = K.want_of("fastq", "shuffled", FULL)
    rs = K.restated("fastq", "shuffled")
    both = texts[0] + texts[1]

    with bsk.Operator("Concat", FULL, 0) as op:
        out = _lib.Out()
        word = (C.c_uint64 * 1)()
        # no verdict yet
        assert lib.bsk_concat_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 0, None) == INV and "bsk_concat_bucket_add: no bucket is open" in err(op)
        assert lib.bsk_concat_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)) == INV and "no bucket is open" in err(op)
        assert lib.bsk_concat_bucket_begin(op.ctx, 0, BINS) == INV and "bsk_concat_verdict_begin first" in err(op)
        assert lib.bsk_concat_join_begin(op.ctx, None) == INV and "bsk_concat_join_begin: no verdict" in err(op)
        assert lib.bsk_concat_verdict_get(op.ctx, 0, 1, word) == INV and "no verdict" in err(op)
        assert lib.bsk_concat_tail_run(op.ctx, ptr2, n2, 0, fmt, 0, 500, None, C.byref(out)) == INV and "no verdict" in err(op)
        assert lib.bsk_concat_verdict_begin(op.ctx, None) == INV and "null argument" in err(op)
        assert lib.bsk_concat_bucket_begin(op.ctx, 5, 5) == INV and lib.bsk_concat_bucket_begin(op.ctx, 0, BINS + 1) == INV
        check(lib.bsk_concat_hist_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(k)), op.ctx)
        n_a = k.value
        check(lib.bsk_concat_hist_run(op.ctx, ptr2, n2, 0, fmt, 1, n_a, None, C.byref(k)), op.ctx)
        n_b = k.value
        assert (n_a, n_b) == (500, 500)
        bsk.ConcatVerdictBegin(op, [n_a, n_b])
        # the join calls before bsk_concat_join_begin
        for rc in (lib.bsk_concat_weigh_run(op.ctx, ptr2, n2, 0, fmt, 0, n_a, None, C.byref(k)),
                   lib.bsk_concat_window_hist_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(k)),
                   lib.bsk_concat_window_hist_get(op.ctx, None, None),
                   lib.bsk_concat_window_begin(op.ctx, 0, BINS),
                   lib.bsk_concat_window_add(op.ctx, ptr, n, 0, fmt, 0, 0, None),
                   lib.bsk_concat_window_finish(op.ctx, None, C.byref(out)),
                   lib.bsk_concat_tail_run(op.ctx, ptr2, n2, 0, fmt, 0, n_a, None, C.byref(out))):
            assert rc == INV and "bsk_concat_join_begin first" in err(op)
        assert lib.bsk_concat_join_begin(op.ctx, None) == INV and "bsk_concat_join_begin: fine bin 0 has not been decided" in err(op)
        # a bucket in the wrong state
        check(lib.bsk_concat_bucket_begin(op.ctx, 0, 2048), op.ctx)
        assert lib.bsk_concat_bucket_begin(op.ctx, 2048, BINS) == INV and "a bucket is open" in err(op)
        assert lib.bsk_concat_verdict_begin(op.ctx, (C.c_uint64 * 2)(n_a, n_b)) == INV and "a bucket is open" in err(op)
        assert lib.bsk_concat_join_begin(op.ctx, None) == INV and "a bucket is open" in err(op)
        # an add that is refused before it runs leaves the bucket usable
        assert lib.bsk_concat_bucket_add(op.ctx, ptr, n, 0, 99, 0, 0, None) == INV and "format" in err(op)
        assert lib.bsk_concat_bucket_add(op.ctx, None, n, 0, fmt, 0, 0, None) == INV and "null shard" in err(op)
        check(lib.bsk_concat_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 0, None), op.ctx)
        check(lib.bsk_concat_bucket_add(op.ctx, ptr2, n2, 0, fmt, 1, n_a, None), op.ctx)
        check(lib.bsk_concat_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)), op.ctx)
        assert lib.bsk_concat_join_begin(op.ctx, None) == INV and "fine bin 2048 has not been decided" in err(op)
        # first_record going backwards closes the bucket
        check(lib.bsk_concat_bucket_begin(op.ctx, 2048, BINS), op.ctx)
        half = R.cuts_of(texts[0], fastq, 3)[1]
        check(lib.bsk_concat_bucket_add(op.ctx, texts[0][:half], half, 0, fmt, 0, 100, None), op.ctx)
        assert lib.bsk_concat_bucket_add(op.ctx, texts[0][:half], half, 0, fmt, 0, 99, None) == INV and "goes backwards" in err(op)
        assert lib.bsk_concat_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)) == INV and "no bucket is open" in err(op)
        # a shard past n1 + n2, and one astride the files
        check(lib.bsk_concat_bucket_begin(op.ctx, 2048, BINS), op.ctx)
        assert lib.bsk_concat_bucket_add(op.ctx, ptr2, n2, 0, fmt, 0, n_a + 1, None) == INV
        assert "bsk_concat_bucket_add" in err(op) and "reach past the total_records = %d of bsk_concat_verdict_begin" % (n_a + n_b) in err(op)
        assert lib.bsk_concat_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)) == INV                        # ... has closed the bucket
        check(lib.bsk_concat_bucket_begin(op.ctx, 2048, BINS), op.ctx)
        assert lib.bsk_concat_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 1, None) == INV and "straddle the two files" in err(op)
        assert lib.bsk_concat_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)) == INV
        check(lib.bsk_concat_bucket_begin(op.ctx, 2048, BINS), op.ctx)                                           # (a bucket that was never finished decided nothing)
        check(lib.bsk_concat_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 0, None), op.ctx)
        check(lib.bsk_concat_bucket_add(op.ctx, ptr2, n2, 0, fmt, 1, n_a, None), op.ctx)
        check(lib.bsk_concat_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)), op.ctx)
        bsk.ConcatJoinBegin(op)
        # a match bucket after the join has begun
        assert lib.bsk_concat_bucket_begin(op.ctx, 0, BINS) == INV and "the join phase has begun" in err(op)
        assert bsk.ConcatVerdictGet(op, 0, n_a + n_b) == rs["head"]
        assert lib.bsk_concat_verdict_get(op.ctx, n_a + n_b, 1, word) == INV and "reach past" in err(op)
        assert lib.bsk_concat_verdict_get(op.ctx, 0, 1, None) == INV and "null argument" in err(op)
        # the window histogram before every record of file 2 is weighed; a shard of the wrong file
        assert lib.bsk_concat_window_hist_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(k)) == INV and "0 records have been weighed, file 2 has 500" in err(op)
        assert lib.bsk_concat_weigh_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(k)) == INV and "lie in file 1" in err(op)
        assert lib.bsk_concat_weigh_run(op.ctx, ptr2, n2, 0, fmt, 0, n_a + 1, None, C.byref(k)) == INV and "reach past the sum of file_records = 1000" in err(op)
        bsk.ConcatWeighRun(op, fb, [n_b], n_a)
        assert lib.bsk_concat_window_hist_run(op.ctx, ptr2, n2, 0, fmt, 0, n_a, None, C.byref(k)) == INV and "lie in file 2" in err(op)
        assert lib.bsk_concat_window_hist_run(op.ctx, ptr, n, 0, fmt, 0, 1, None, C.byref(k)) == INV and "straddle the two files" in err(op)
        bsk.ConcatWindowHistRun(op, fa, [n_a])
        assert bsk.ConcatWindowHistGet(op) == rs["whist"]
        # a window in the wrong state
        assert lib.bsk_concat_window_add(op.ctx, ptr, n, 0, fmt, 0, 0, None) == INV and "bsk_concat_window_add: no window is open" in err(op)
        assert lib.bsk_concat_window_finish(op.ctx, None, C.byref(out)) == INV and "no window is open" in err(op)
        assert lib.bsk_concat_window_finish(op.ctx, None, None) == INV
        assert lib.bsk_concat_window_begin(op.ctx, 7, 7) == INV and "0 <= lo < hi <= 4096" in err(op)
        check(lib.bsk_concat_window_begin(op.ctx, 0, BINS), op.ctx)
        assert lib.bsk_concat_window_begin(op.ctx, 0, BINS) == INV and "a window is open" in err(op)
        assert lib.bsk_concat_verdict_begin(op.ctx, (C.c_uint64 * 2)(n_a, n_b)) == INV and "a window is open" in err(op)
        assert lib.bsk_concat_join_begin(op.ctx, None) == INV and "a window is open" in err(op)
        # first_record going backwards closes the window
        cut = R.cuts_of(texts[0], fastq, 3)[1]
        check(lib.bsk_concat_window_add(op.ctx, texts[0][cut:], len(texts[0]) - cut, 0, fmt, 0, 166, None), op.ctx)
        assert lib.bsk_concat_window_add(op.ctx, texts[0][:cut], cut, 0, fmt, 0, 0, None) == INV and "bsk_concat_window_add" in err(op) and "goes backwards" in err(op)
        assert lib.bsk_concat_window_finish(op.ctx, None, C.byref(out)) == INV and "no window is open" in err(op)
        # a shard of file 1 after a shard of file 2
        check(lib.bsk_concat_window_begin(op.ctx, 0, BINS), op.ctx)
        check(lib.bsk_concat_window_add(op.ctx, ptr2, n2, 0, fmt, 0, n_a, None), op.ctx)
        assert lib.bsk_concat_window_add(op.ctx, ptr, n, 0, fmt, 0, 0, None) == INV and "a shard of file 1 (first_record 0) after a shard of file 2" in err(op)
        check(lib.bsk_concat_window_begin(op.ctx, 0, BINS), op.ctx)
        assert lib.bsk_concat_window_add(op.ctx, ptr, n, 0, fmt, 0, 1, None) == INV and "straddle the two files" in err(op)
        check(lib.bsk_concat_window_begin(op.ctx, 0, BINS), op.ctx)
        assert lib.bsk_concat_window_add(op.ctx, ptr2, n2, 0, fmt, 0, n_a + 1, None) == INV and "reach past the sum of file_records" in err(op)
        # a window that did not get its records of file 1, and one that has not seen file 2
        check(lib.bsk_concat_window_begin(op.ctx, 0, BINS), op.ctx)
        check(lib.bsk_concat_window_add(op.ctx, texts[0][cut:], len(texts[0]) - cut, 0, fmt, 0, 166, None), op.ctx)
        check(lib.bsk_concat_window_add(op.ctx, ptr2, n2, 0, fmt, 0, n_a, None), op.ctx)
        assert lib.bsk_concat_window_finish(op.ctx, None, C.byref(out)) == INV and "the window holds 334 records of file 1, the window histogram has 500" in err(op)
        check(lib.bsk_concat_window_begin(op.ctx, 0, BINS), op.ctx)
        check(lib.bsk_concat_window_add(op.ctx, ptr, n, 0, fmt, 0, 0, None), op.ctx)
        assert lib.bsk_concat_window_finish(op.ctx, None, C.byref(out)) == INV and "has seen 0 of the 500 records of file 2" in err(op)
        # the tail: a shard of file 1
        assert lib.bsk_concat_tail_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(out)) == INV and "lie in file 1" in err(op)
        # the context is whole after all that
        assert bsk.ConcatWindow(op, [fa, fb], [[n_a], [n_b]], 0, BINS) + bsk.ConcatTail(op, fb, [n_b], n_a) == want
        bsk.ConcatVerdictBegin(op, [n_a, n_b])                                                                   # a new verdict forgets the decided bins
        assert lib.bsk_concat_window_begin(op.ctx, 0, BINS) == INV and "bsk_concat_join_begin first" in err(op)
        assert lib.bsk_concat_join_begin(op.ctx, None) == INV and "fine bin 0 has not been decided" in err(op)
        # the one call still runs on a context that has been through the buckets
        check(lib.bsk_concat_run(op.ctx, both, len(both), len(texts[0]), 0, fmt, None, C.byref(out)), op.ctx)
        assert bsk.api._out_bytes(op, out) == want
    # a fine bin above the budget: the plan's refusal
    hb = rs["hist"][0]
    with pytest.raises(bsk.BskError) as e:
        bsk.ConcatBuckets(fa, fb, budget_bytes=max(hb) - 1)
    assert e.value.code == UNS and "budget of %d bytes" % (max(hb) - 1) in str(e.value)
    # a heavy ID: 30 records of one ID in either file, a budget below its one window bin -- refused, the bytes named
    heavy = [[(b"big", b"ACGT" * 50)] * 30 + [(b"r%d" % i, b"ACGT") for i in range(30)], [(b"big", b"TTG" * 60)] * 30]
    ht = [P.tiny_text(f, True) for f in heavy]
    costs = [[P.text_cost(x, True) for x in f] for f in heavy]
    hh = K.py_head([h for h, _ in heavy[0]], [h for h, _ in heavy[1]])
    whb = K.window_hist(K.py_costs(hh, *K.py_weights(hh, 60, costs[1]), costs[0]))[0]
    assert max(whb) == whb[0] == costs[0][0] * 31 + 2 * sum(costs[1]) > max(R.py_hist([b"big"] * 60 + [b"r%d" % i for i in range(30)])[0])
    with pytest.raises(bsk.BskError) as e:
        bsk.ConcatBuckets(frame(ht[0], True), frame(ht[1], True), Opts({"Full": True}), budget_bytes=max(whb) - 1)
    assert e.value.code == UNS and "holds %d bytes, more than the budget of %d bytes" % (max(whb), max(whb) - 1) in str(e.value)
    assert bsk.ConcatBuckets(frame(ht[0], True), frame(ht[1], True), Opts({"Full": True}), budget_bytes=max(whb)) == oracle.concat(ht[0], ht[1], True, FULL)
    # out=slices on the window finish and the tail is refused; the one call is what it was
    os.environ["BSK_OUT"] = "slices"
    try:
        assert one_call_of(texts, fastq, {"Full": True}) == want
        with pytest.raises(bsk.BskError) as e:
            bsk.ConcatBuckets(fa, fb, Opts({"Full": True}), budget_bytes=K.budget_of(rs["whist"][0], 0.25))
        assert e.value.code == UNS and "bsk_concat_window_finish: out=slices" in str(e.value)
        with bsk.Operator("Concat", FULL, 0) as op:
            counts = bsk.ConcatHistRun(op, [fa, fb])
            bsk.ConcatVerdictBegin(op, [500, 500])
            bsk.ConcatBucket(op, [fa, fb], counts, 0, BINS)
            bsk.ConcatJoinBegin(op)
            out = _lib.Out()
            assert lib.bsk_concat_tail_run(op.ctx, ptr2, n2, 0, fmt, 0, 500, None, C.byref(out)) == UNS and "bsk_concat_tail_run: out=slices" in err(op)
    finally:
        del os.environ["BSK_OUT"]
    # every entry point on a context of another operator -- and the siblings' on a Concat context
    arr = (C.c_uint64 * 2)(10, 10)
    for other in ("Shuffle", "RmDup", "Rename", "Common", "Pair"):
        with bsk.Operator(other, "{}", 0) as op:
            out = _lib.Out()
            for rc in (lib.bsk_concat_hist_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(k)),
                       lib.bsk_concat_hist_get(op.ctx, None, None),
                       lib.bsk_concat_hist_reset(op.ctx),
                       lib.bsk_concat_verdict_begin(op.ctx, arr),
                       lib.bsk_concat_verdict_get(op.ctx, 0, 1, (C.c_uint64 * 1)()),
                       lib.bsk_concat_bucket_begin(op.ctx, 0, BINS),
                       lib.bsk_concat_bucket_add(op.ctx, ptr, n, 0, fmt, 0, 0, None),
                       lib.bsk_concat_bucket_finish(op.ctx, None, C.byref(r), C.byref(fl)),
                       lib.bsk_concat_join_begin(op.ctx, None),
                       lib.bsk_concat_weigh_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(k)),
                       lib.bsk_concat_window_hist_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(k)),
                       lib.bsk_concat_window_hist_get(op.ctx, None, None),
                       lib.bsk_concat_window_begin(op.ctx, 0, BINS),
                       lib.bsk_concat_window_add(op.ctx, ptr, n, 0, fmt, 0, 0, None),
                       lib.bsk_concat_window_finish(op.ctx, None, C.byref(out)),
                       lib.bsk_concat_tail_run(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(out))):
                assert rc == INV and "not a Concat context" in err(op)
    with bsk.Operator("Concat", "{}", 0) as op:
        out = _lib.Out()
        for prefix, message, word in (("bsk_rmdup", "not an RmDup context", C.c_uint8), ("bsk_rename", "not a Rename context", C.c_uint32),
                                      ("bsk_common", "not a Common context", C.c_uint8), ("bsk_pair", "not a Pair context", C.c_uint64)):
            fn = lambda name: getattr(lib, prefix + "_" + name)
            outs = (_lib.Out * 3)()
            for rc in (fn("hist_run")(op.ctx, ptr, n, 0, fmt, 0, 0, None, C.byref(k)),
                       fn("hist_get")(op.ctx, None, None),
                       fn("hist_reset")(op.ctx),
                       fn("verdict_begin")(op.ctx, arr, 2) if prefix == "bsk_common" else fn("verdict_begin")(op.ctx, arr) if prefix == "bsk_pair"
                       else fn("verdict_begin")(op.ctx, 10),
                       fn("verdict_get")(op.ctx, 0, 1, (word * 1)()),
                       fn("bucket_begin")(op.ctx, 0, BINS),
                       fn("bucket_add")(op.ctx, ptr, n, 0, fmt, 0, 0, None),
                       fn("bucket_finish")(op.ctx, None, C.byref(r), C.byref(fl)),
                       fn("emit_run")(op.ctx, ptr, n, 0, fmt, 0, 0, None, outs if prefix == "bsk_pair" else C.byref(out))):
                assert rc == INV and message in err(op)


# ------------------------------------------------------------------ the command line
@pytest.mark.parametrize("variant", P.VARIANTS)
def test_cli_concat_in_buckets(tmp_path, variant):
    texts, fastq = P.files_text("fastq", variant)
    r = K.restated("fastq", variant)
    paths = [str(tmp_path / x) for x in ("reads_1.fq", "reads_2.fq")]
    for path, text in zip(paths, texts):
        open(path, "wb").write(text)
    budget = max(max(r["hist"][0]), max(r["whist"][0]), sum(r["hist"][0]) // 4)
    assert len(bsk.ShufflePlan(r["hist"][0], budget)) - 1 >= 3 and len(bsk.ShufflePlan(r["whist"][0], budget)) - 1 >= 3
    assert budget < len(texts[0]) + len(texts[1])
    for flags, full in (([], False), (["-f"], True)):
        want = K.want_of("fastq", variant, json.dumps({"Full": full}))
        plain, bucketed = str(tmp_path / ("plain%d" % full)), str(tmp_path / ("buckets%d" % full))
        p = subprocess.run([CLI, "concat", *paths, "-o", plain, "--merge", *flags], capture_output=True, timeout=900, env=dict(os.environ, BSK_CLI_TIMING="1"))
        assert p.returncode == 0 and "k_rdb_hist" not in p.stderr.decode(), p.stderr.decode()   # the whole-file run, as before
        env = dict(os.environ, BSK_CLI_TIMING="1", BSK_STREAM_PIECE_BYTES="65536", BSK_CONCAT_BUDGET_BYTES=str(budget))
        p = subprocess.run([CLI, "concat", *paths, "-o", bucketed, "--merge", *flags], capture_output=True, timeout=900, env=env)
        assert p.returncode == 0, p.stderr.decode()
        assert open(bucketed, "rb").read() == open(plain, "rb").read() == want, flags
        err = p.stderr.decode()
        assert all(s in err for s in ("k_rdb_hist", "k_rdb_pick", "k_catb_verify", "k_catb_weigh", "k_catb_hist", "k_catb_pick", "concat_window")), err[-800:]
        assert ("k_catb_tail" in err) == full
        assert "concat: %d record(s) with a head, 0 flagged" % sum(1 for h in r["head"] if h is not None) in err
    # the standard output receives the shares too; a directory of part files is cut from the whole result
    env = dict(os.environ, BSK_STREAM_PIECE_BYTES="65536", BSK_CONCAT_BUDGET_BYTES=str(budget))
    p = subprocess.run([CLI, "concat", *paths, "-o", "-", "-f"], capture_output=True, timeout=900, env=env)
    assert p.returncode == 0 and p.stdout == want, p.stderr.decode()
    p = subprocess.run([CLI, "concat", *paths, "-o", str(tmp_path / "parts"), "-f"], capture_output=True, timeout=900, env=env)
    assert p.returncode == 0 and open(str(tmp_path / "parts" / "part00000"), "rb").read() == want, p.stderr.decode()
    p = subprocess.run([CLI, "concat", paths[0], "-o", str(tmp_path / "x")], capture_output=True, timeout=900, env=dict(os.environ, BSK_CONCAT_BUDGET_BYTES=str(budget)))
    assert p.returncode != 0 and "2 files needed" in p.stderr.decode()
    # a budget below the fullest window bin: the refusal names the bytes
    p = subprocess.run([CLI, "concat", *paths, "-o", str(tmp_path / "y"), "--merge"], capture_output=True, timeout=900,
                       env=dict(os.environ, BSK_CONCAT_BUDGET_BYTES=str(max(r["whist"][0]) - 1)))
    assert p.returncode != 0 and "holds %d bytes, more than the budget of %d bytes" % (max(r["whist"][0]), max(r["whist"][0]) - 1) in p.stderr.decode()
    assert "concat: a window bin" in p.stderr.decode()
