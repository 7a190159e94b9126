"""`sort` in buckets of the key on the GPU (PARITY.md SORT "Buckets"; include/bsk.h bsk_sort_sample_run .. bsk_sort_bucket_finish):
the bytes are those of the one-pass bsk.Sort and of the oracle whatever the splitters, the number of buckets and the cut of the
input into shards; the fine bins against a restatement of the canonical key and the padded comparison; the sample; the smallest
shapes; misuse; the command line."""
import bisect
import ctypes as C
import functools
import json
import os
import random
import subprocess

import pytest

import bigseqkit_amd as bsk
from bigseqkit_amd import _lib
from bigseqkit_amd._lib import lib, check
import oracle
import sample_ref as R
from test_sample_gpu import frame, wrap
from test_sort_gpu import OPTS, make

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")
BINS = 4096
SAMPLE_SEED = 0x534F5254   # ops_sort_buckets.hpp SORT_SAMPLE_SEED
KEY_CUT = 256              # ... SORT_SAMPLE_KEY_BYTES


class Opts:
    def __init__(self, d):
        self.d = dict(d)

    def to_json(self):
        return json.dumps(self.d)


# ------------------------------------------------------------------ the restatement: records, canonical keys, bins, histogram
def parse(data, fastq):
    """[(bytes of text + newline, header without its marker, sequence)] of 4-line FASTQ / FASTA without blank lines"""
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    recs = []
    if fastq:
        for k in range(0, len(lines), 4):
            h, s, p, q = lines[k:k + 4]
            recs.append((len(h) + len(s) + len(p) + len(q) + 4, h[1:], s))
        return recs
    for ln in lines:
        if ln.startswith(b">"):
            recs.append([len(ln) + 1, ln[1:], b""])
        else:
            recs[-1][0] += len(ln) + 1
            recs[-1][2] += ln
    return [tuple(r) for r in recs]


def natural_key(k, fold):
    """natural_key of sort_key_dev.hpp: digit run -> '0', number of significant digits, the digits; other run -> its bytes, 0"""
    out, i = bytearray(), 0
    while i < len(k):
        if 48 <= k[i] <= 57:
            j = i
            while j < len(k) and 48 <= k[j] <= 57:
                j += 1
            z = i
            while z + 1 < j and k[z] == 48:
                z += 1
            out += b"0" + bytes([min(j - z, 255)]) + k[z:j]
            i = j
        else:
            while i < len(k) and not 48 <= k[i] <= 57:
                out.append(k[i] + 32 if fold and 65 <= k[i] <= 90 else k[i])
                i += 1
            out.append(0)
    return bytes(out)


def key_of(rec, o):
    """the canonical key of PARITY SORT"""
    _, head, seq = rec
    if o.get("ByBases"):
        gaps = o.get("GapLetters", "- \t.").encode()
        return (len(seq) - sum(seq.count(bytes([g])) for g in set(gaps))).to_bytes(4, "big")
    if o.get("ByLength"):
        return len(seq).to_bytes(4, "big")
    if o.get("BySeq"):
        L = o.get("SeqPrefixLength", 10000)
        k = seq if L == 0 else seq[:L]
        return k.lower() if o.get("IgnoreCase") else k
    k = head
    if not o.get("ByName"):
        sp = head.find(b" ")
        if sp <= 0:
            sp = head.find(b"\t")
        k = head[:sp] if sp > 0 else head
    if o.get("InNaturalOrder"):
        return natural_key(k, bool(o.get("IgnoreCase")))
    return k.lower() if o.get("IgnoreCase") else k


def strip0(s):
    """a string without its trailing zero bytes is the same string under the padded comparison, and on such strings that
    comparison is the plain one"""
    return s.rstrip(b"\0")


def bins_of(keys, splitters):
    sp = [strip0(s) for s in splitters]
    assert all(a < b for a, b in zip(sp[:-1], sp[1:]))
    return [bisect.bisect_right(sp, strip0(k)) for k in keys]


def py_hist(recs, keys, splitters):
    hb, hr = [0] * BINS, [0] * BINS
    for r, b in zip(recs, bins_of(keys, splitters)):
        hb[b] += r[0]
        hr[b] += 1
    return hb, hr


def py_plan(hb, budget):
    bounds, s = [0], 0
    for b, v in enumerate(hb):
        if s + v > budget:
            bounds.append(b)
            s = 0
        s += v
    return bounds + [BINS]


def py_sample(keys, cap=1 << 18, rate=1.0):
    """the sample restated: record g is in it when (draw >> 11) < T; above the cap T halves"""
    draws = [R.draw(SAMPLE_SEED, g) >> 11 for g in range(len(keys))]
    T = min(1 << 53, -int(-rate * (1 << 53) // 1))
    while sum(1 for d in draws if d < T) > cap:
        T >>= 1
    return [k[:KEY_CUT] for k, d in zip(keys, draws) if d < T]


def default_rate(n):
    return min(1.0, 32 * BINS / max(1, n))


def run(f, o, budget, splitters=None, rate=None):
    """bsk.SortBuckets, step by step: (bytes, number of buckets)"""
    op_o = Opts(o)
    with bsk.Operator("Sort", op_o.to_json(), 0) as op:
        buckets, counts = bsk.SortBucketsPlan(op, f, op_o, budget, splitters, rate)
        return b"".join(bsk.SortBucket(op, f, counts, lo, hi) for lo, hi in buckets), len(buckets)


HAND = b"".join(b"@%s\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in
                ((b"abc", b"ACGT"), (b"abcd x", b""), (b"abc", b"ACG"), (b"ab", b"ACGTA"), (b"abc y", b""), (b"abcd", b"ACGT")))


@functools.lru_cache(maxsize=None)
def shape(name):
    """ties, a 31-byte common prefix, empty keys (-s), keys that are proper prefixes of others"""
    if name == "fastq":
        return make(random.Random(41), 600, True) + HAND, True
    data = make(random.Random(42), 600, False, 7)
    return data + b">abc\nACGT\n>abcd x\n>abc\nACG\n>ab\nACGTA\n", False


@functools.lru_cache(maxsize=None)
def restated(name, oj):
    """(records, keys, splitters of the default sample, histogram bytes) of a shape under options `oj` (JSON)"""
    data, fastq = shape(name)
    o = json.loads(oj)
    recs = parse(data, fastq)
    keys = [key_of(r, o) for r in recs]
    sp = bsk.SortPickSplitters(py_sample(keys, rate=default_rate(len(keys))))
    return recs, keys, sp, py_hist(recs, keys, sp)[0]


@functools.lru_cache(maxsize=None)
def want_of(name, oj):
    data, fastq = shape(name)
    return oracle.sort(data, fastq, oj)


# ------------------------------------------------------------------ bytes
@pytest.mark.parametrize("name", ["fastq", "fasta wrapped at 7"])
def test_every_option_gives_the_bytes_of_sort(name):
    data, fastq = shape(name)
    for o in OPTS:
        oj = json.dumps(o)
        want = want_of(name, oj)
        assert bsk.Sort(frame(data, fastq), Opts(o)) == want, o
        got, nb = run(frame(data, fastq, 3), o, len(data) // 5)
        assert got == want, (o, nb)
        assert nb >= 3, (o, nb)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("o", [{}, {"BySeq": True, "IgnoreCase": True}, {"ByLength": True, "Reverse": True}], ids=["id", "seq -i", "length -r"])
@pytest.mark.parametrize("name", ["fastq", "fasta wrapped at 7"])
def test_shards_budgets_and_bucket_counts(name, o, device):
    data, fastq = shape(name)
    oj = json.dumps(o)
    recs, keys, sp, hb = restated(name, oj)
    T, m = sum(hb), max(hb)
    budgets = [(T, 1), (T // 2 + m, 2), (m, None)]
    counts = [len(py_plan(hb, b)) - 1 for b, _ in budgets]
    assert counts[0] == 1 and counts[1] == 2 and counts[2] >= 3, counts
    want = want_of(name, oj)
    for parts in (1, 3, 7):
        f = frame(data, fastq, parts, device)
        for (budget, _), nb_want in zip(budgets, counts):
            got, nb = run(f, o, budget)
            assert nb == nb_want, (parts, budget, nb, nb_want)
            assert got == want, (parts, budget)


# ------------------------------------------------------------------ bins against the restatement, hand-set splitters
P256 = bytes(random.Random(7).choice(b"ACGT") for _ in range(256))


@functools.lru_cache(maxsize=None)
def bins_input():
    """FASTA (wrapped at 60): the records of `make`, and sequences that agree on 256 bytes and differ behind them"""
    data = make(random.Random(43), 300, False)
    for k, tail in enumerate((b"A", b"", b"C", b"AC", b"A", b"T" * 700)):
        s = P256 + tail
        data += b">long%d\n" % k + wrap(s.decode(), 60).encode() + b"\n"
    data += b">short\n" + wrap(P256[:100].decode(), 60).encode() + b"\n"
    return data


def splitter_sets(keys):
    """hand-set splitters: k = 0, 1, 2, 4094, 4095; one equal to a key, one a proper prefix of keys, a key plus a zero byte, the
    empty string, the 256-byte cut of a longer key"""
    ks = sorted({strip0(k) for k in keys})
    pool = set(ks)
    for k in ks:
        pool.update(k[:m] for m in range(len(k)))
        pool.add(k + b"!")
    pool.update(b"zz%05d" % j for j in range(5000))
    pool.update(bytes([a, b]) for a in range(1, 256, 3) for b in range(1, 256, 5))
    pool = sorted({strip0(p) for p in pool})
    out = [[], [ks[len(ks) // 2]], [b"", ks[len(ks) // 3] + b"\0"]]
    for k in (4094, 4095):
        assert len(pool) >= k
        out.append([pool[len(pool) * j // k] for j in range(k)])
    long_keys = [k for k in ks if len(k) > 1]
    out.append(sorted({strip0(x) for x in (long_keys[0][:1], long_keys[len(long_keys) // 2], long_keys[-1][:-1])}))
    if any(len(k) > KEY_CUT for k in keys):
        out.append([P256[:100], P256])
    return out


@pytest.mark.parametrize("o", [{}, {"ByName": True, "IgnoreCase": True}, {"BySeq": True, "SeqPrefixLength": 5}, {"BySeq": True, "SeqPrefixLength": 0},
                               {"ByLength": True}, {"InNaturalOrder": True}], ids=["id", "-n -i", "-s -L 5", "-s", "-l", "-N"])
def test_histogram_equals_its_restatement(o):
    data = bins_input()
    recs = parse(data, False)
    keys = [key_of(r, o) for r in recs]
    with bsk.Operator("Sort", json.dumps(o), 0) as op:
        for sp in splitter_sets(keys):
            for parts in (1, 3):
                bsk.SortSplittersSet(op, sp)
                assert bsk.SortSplittersGet(op) == sp
                bsk.SortHistReset(op)
                counts = bsk.SortHistRun(op, frame(data, False, parts))
                assert sum(counts) == len(recs)
                assert bsk.SortHistGet(op) == py_hist(recs, keys, sp), (o, len(sp), parts)


def test_a_key_longer_than_its_splitter_is_decided_behind_it():
    """the records that agree on the 256 bytes of the splitter and differ behind them share its bin, whatever follows"""
    data = bins_input()
    o = {"BySeq": True, "SeqPrefixLength": 0}
    recs = parse(data, False)
    keys = [key_of(r, o) for r in recs]
    b = bins_of(keys, [P256[:100], P256])
    assert b[-7:] == [2, 2, 2, 2, 2, 2, 1]               # long0 .. long5 at or above the cut, `short` equal to the first splitter
    with bsk.Operator("Sort", json.dumps(o), 0) as op:
        bsk.SortSplittersSet(op, [P256[:100], P256])
        bsk.SortHistRun(op, frame(data, False))
        assert bsk.SortHistGet(op)[1][:3] == [b.count(0), b.count(1), b.count(2)] and sum(bsk.SortHistGet(op)[1][3:]) == 0


# ------------------------------------------------------------------ any splitters, the same bytes
@pytest.mark.parametrize("o", [{}, {"BySeq": True, "Reverse": True}, {"ByBases": True}, {"InNaturalOrder": True, "IgnoreCase": True}],
                         ids=["id", "seq -r", "bases", "-N -i"])
def test_any_splitters_give_the_bytes_of_sort(o):
    data, fastq = shape("fastq")
    oj = json.dumps(o)
    want = want_of("fastq", oj)
    recs, keys, _, _ = restated("fastq", oj)
    rng = random.Random(9)
    pool = sorted({strip0(k[:rng.randint(0, len(k))]) for k in keys} | {strip0(k) for k in keys})
    sets = [[], [b""], pool, pool[::7], sorted(rng.sample(pool, min(5, len(pool))))]
    for sp in sets:
        hb = py_hist(recs, keys, sp)[0]
        for budget in (sum(hb), max(max(hb), sum(hb) // 4)):
            got, nb = run(frame(data, fastq, 3), o, budget, splitters=sp)
            assert got == want, (o, len(sp), budget, nb)


def test_all_records_in_one_bin_run_into_the_refusal():
    data, fastq = shape("fastq")
    sp = [b"zz%05d" % j for j in range(4095)]           # above every ID: 4095 splitters, one bin in use
    recs, keys, _, _ = restated("fastq", "{}")
    hb = py_hist(recs, keys, sp)[0]
    assert hb[0] == sum(hb) == len(data)
    assert run(frame(data, fastq, 3), {}, len(data), splitters=sp) == (want_of("fastq", "{}"), 1)
    with pytest.raises(bsk.BskError) as e:
        run(frame(data, fastq, 3), {}, len(data) - 1, splitters=sp)
    assert e.value.code == _lib.BSK_ERR_UNSUPPORTED and str(len(data)) in str(e.value) and "budget of %d bytes" % (len(data) - 1) in str(e.value)


# ------------------------------------------------------------------ the sample
def built_splitters(f, o, rate):
    with bsk.Operator("Sort", json.dumps(o), 0) as op:
        bsk.SortSampleRun(op, f, rate)
        n = bsk.SortSampleCount(op)
        nbins = bsk.SortSplittersBuild(op)
        sp = bsk.SortSplittersGet(op)
        assert nbins == len(sp) + 1
        return n, sp


@pytest.mark.parametrize("cap", [None, 100], ids=["all", "thinned"])
def test_the_sample_does_not_depend_on_the_cut(cap, monkeypatch):
    if cap:
        monkeypatch.setenv("BSK_SORT_SAMPLE_CAP", str(cap))
    data, fastq = shape("fastq")
    for o, rate in (({}, 1.0), ({"BySeq": True}, 1.0), ({"ByLength": True}, 0.5)):
        recs, keys, _, _ = restated("fastq", json.dumps(o))
        sample = py_sample(keys, cap or 1 << 18, rate)
        assert 0 < len(sample) <= (cap or len(keys)) and (len(sample) < len(keys) if cap or rate < 1 else len(sample) == len(keys))
        want = bsk.SortPickSplitters(sample)
        for parts, device in ((1, False), (3, False), (7, False), (3, True)):
            assert built_splitters(frame(data, fastq, parts, device), o, rate) == (len(sample), want), (o, parts, device)
    # ... and neither do the bytes
    for o in ({}, {"BySeq": True, "Reverse": True}):
        for parts in (1, 7):
            assert run(frame(data, fastq, parts), o, len(data) // 4, rate=1.0)[0] == want_of("fastq", json.dumps(o))


# ------------------------------------------------------------------ edges
@pytest.mark.parametrize("fastq", [True, False])
def test_smallest_shapes(fastq):
    one = b"@r\nACGT\n+\nIIII\n" if fastq else b">r d\nACGT\n"
    two = (b"@s x\nAC\n+\nII\n" if fastq else b">s x\nAC\n") + one
    for data in (b"", one, one[:-1]):
        for budget in (1 << 30, len(one)):
            assert run(frame(data, fastq), {}, budget) == (one if data else b"", 1)
    # two records in two buckets: the budget holds the larger one alone
    want = oracle.sort(two, fastq)
    assert want == one + two[:-len(one)]
    for parts in (1, 2):
        for o in ({}, {"Reverse": True}):
            assert run(frame(two, fastq, parts), o, len(one)) == (oracle.sort(two, fastq, json.dumps(o)), 2), (parts, o)


def test_all_keys_equal():
    data = b"".join(b"@same %d\n%s\n+\n%s\n" % (i, b"ACGT" * (i % 5), b"IIII" * (i % 5)) for i in range(300))
    for parts in (1, 3):
        assert run(frame(data, True, parts), {}, len(data)) == (data, 1)        # ties keep file order
        assert run(frame(data, True, parts), {"Reverse": True}, len(data)) == (data, 1)
    with pytest.raises(bsk.BskError) as e:
        run(frame(data, True, 3), {}, len(data) // 2)
    assert e.value.code == _lib.BSK_ERR_UNSUPPORTED


def test_a_shard_of_one_record_between_two_larger_ones():
    data = make(random.Random(32), 201, True)
    starts = [s for s, _ in oracle.record_spans(data, True)]
    cuts = [0, starts[100], starts[101], len(data)]
    f = bsk.SeqFrame(bsk.FORMAT_FASTQ, [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])])
    for o in ({}, {"BySeq": True}):
        got, nb = run(f, o, len(data) // 4)
        assert got == oracle.sort(data, True, json.dumps(o)) and nb >= 3, (o, nb)


@pytest.mark.parametrize("parts", [1, 3])
def test_past_the_grid_stride_of_the_histogram(parts):
    """more records than the lanes of the histogram's grid (three blocks per CU), few bytes each; the last record has no newline
    and lands inside the output.  One shard: a launch takes a second stride of the grid; three: every launch stays below it"""
    import torch
    n = 3 * torch.cuda.get_device_properties(0).multi_processor_count * 256 + 77
    ids = list(range(n))
    random.Random(5).shuffle(ids)
    ids.append(ids.pop(ids.index(5)))                      # "5" last in the file, in the middle of the order
    data = b"".join(b">%d\nA\n" % i for i in ids)[:-1]
    want = oracle.sort(data, False)
    assert want.index(b">5\nA\n") not in (0, len(want) - 5)
    recs = parse(data, False)
    keys = [r[1] for r in recs]
    sp = bsk.SortPickSplitters(py_sample(keys, rate=default_rate(n)))
    hb, hr = py_hist(recs, keys, sp)
    f = frame(data, False, parts)
    with bsk.Operator("Sort", "{}", 0) as op:
        buckets, counts = bsk.SortBucketsPlan(op, f, Opts({}), sum(hb) // 3 + max(hb))
        assert bsk.SortSplittersGet(op) == sp and bsk.SortHistGet(op) == (hb, hr)
        assert len(buckets) == len(py_plan(hb, sum(hb) // 3 + max(hb))) - 1 and 2 <= len(buckets) <= 3
        got = b"".join(bsk.SortBucket(op, f, counts, lo, hi) for lo, hi in buckets)
    assert got == want


@pytest.mark.parametrize("segcopy", ["off", "force"])
def test_copy_paths(segcopy, monkeypatch):
    """the byte-wise copy that stands in for the segmented copy (switch segcopy), a last record without its newline included"""
    monkeypatch.setenv("BSK_SEGCOPY", segcopy)
    for fastq in (True, False):
        data = make(random.Random(33), 150, fastq, 60, final_newline=False)
        for o in ({}, {"BySeq": True, "Reverse": True}):
            got, nb = run(frame(data, fastq, 3), o, len(data) // 3)
            assert got == oracle.sort(data, fastq, json.dumps(o)) and nb >= 2, (fastq, o, nb)


def test_fastq_wrapped_at_7():
    """a wrapped FASTQ shard is accumulated as the 4-line text of the multi-line reader; the output is Format text either way"""
    rng = random.Random(71)
    recs = []
    for i in range(250):
        L = rng.randint(1, 90)
        s = "".join(rng.choice("ACGT") for _ in range(L))
        q = "".join(rng.choice("ABCDEFGHI") for _ in range(L))
        recs.append("@w%d x\n%s\n+\n%s\n" % (rng.randrange(120), wrap(s, 7), wrap(q, 7)))
    data = "".join(recs).encode()
    for o in ({}, {"BySeq": True}, {"ByLength": True, "Reverse": True}):
        want = oracle.sort(data, True, json.dumps(o))
        assert bsk.Sort(frame(data, True), Opts(o)) == want
        for parts in (1, 3):
            got, nb = run(frame(data, True, parts), o, len(want) // 3)
            assert got == want and nb >= 2, (o, parts, nb)


# ------------------------------------------------------------------ misuse, refusals, stage names
def test_refusals_and_misuse():
    data, fastq = shape("fastq")
    f = frame(data, fastq)
    with pytest.raises(bsk.BskError) as e:
        bsk.SortBuckets(f, Opts({}), 1)
    msg = str(e.value)
    assert e.value.code == _lib.BSK_ERR_UNSUPPORTED and "budget of 1 bytes" in msg
    hb = restated("fastq", "{}")[3]
    assert "holds %d bytes" % next(v for v in hb if v > 1) in msg          # the first bin above the budget, by its bytes
    (pid, ptr, n, on_dev, keep), = f.partitions()
    err = lambda op: lib.bsk_last_error(op.ctx).decode()
    with bsk.Operator("Sort", "{}", 0) as op:
        out = _lib.Out()
        assert lib.bsk_sort_bucket_add(op.ctx, ptr, n, 0, f.format, 0, 0, None) == _lib.BSK_ERR_INVALID_ARG and "bsk_sort_bucket_add" in err(op)
        assert lib.bsk_sort_bucket_finish(op.ctx, None, C.byref(out)) == _lib.BSK_ERR_INVALID_ARG and "bsk_sort_bucket_finish" in err(op)
        check(lib.bsk_sort_bucket_begin(op.ctx, 0, BINS), op.ctx)
        assert lib.bsk_sort_bucket_begin(op.ctx, 0, BINS) == _lib.BSK_ERR_INVALID_ARG and "bsk_sort_bucket_begin" in err(op)
        assert lib.bsk_sort_bucket_begin(op.ctx, 7, 7) == _lib.BSK_ERR_INVALID_ARG                    # an empty bin range
        assert lib.bsk_sort_bucket_begin(op.ctx, 0, BINS + 1) == _lib.BSK_ERR_INVALID_ARG
        # the open bucket is still good: the whole range is the one-pass sort
        check(lib.bsk_sort_bucket_add(op.ctx, ptr, n, 0, f.format, 0, 0, None), op.ctx)
        check(lib.bsk_sort_bucket_finish(op.ctx, None, C.byref(out)), op.ctx)
        buf = C.create_string_buffer(out.len)
        check(lib.bsk_out_to_host(op.ctx, C.byref(out), buf, out.len), op.ctx)
        assert buf.raw[:out.len] == want_of("fastq", "{}") and out.records == len(parse(data, fastq))
        assert lib.bsk_sort_bucket_finish(op.ctx, None, C.byref(out)) == _lib.BSK_ERR_INVALID_ARG        # finished: closed again
        # the shards of a bucket arrive in input order: a first_record that goes backwards closes the bucket
        check(lib.bsk_sort_bucket_begin(op.ctx, 0, BINS), op.ctx)
        check(lib.bsk_sort_bucket_add(op.ctx, ptr, n, 0, f.format, 0, 100, None), op.ctx)
        assert lib.bsk_sort_bucket_add(op.ctx, ptr, n, 0, f.format, 0, 99, None) == _lib.BSK_ERR_INVALID_ARG and "goes backwards" in err(op)
        assert lib.bsk_sort_bucket_finish(op.ctx, None, C.byref(out)) == _lib.BSK_ERR_INVALID_ARG
        # splitters that are not strictly ascending under the padded comparison
        for sp in ([b"b", b"a"], [b"a", b"a"], [b"a", b"a\0"], [b"", b"\0\0"]):
            with pytest.raises(bsk.BskError) as e:
                bsk.SortSplittersSet(op, sp)
            assert e.value.code == _lib.BSK_ERR_INVALID_ARG and "not strictly ascending" in str(e.value), sp
        with pytest.raises(bsk.BskError):
            bsk.SortSplittersSet(op, [b"%05d" % j for j in range(4096)])
        assert bsk.SortSplittersGet(op) == []                                                            # a refused list installs nothing
    with bsk.Operator("Shuffle", "{}", 0) as op:
        k, k32 = C.c_uint64(), C.c_uint32()
        offs = (C.c_uint64 * 2)(0, 1)
        for rc in (lib.bsk_sort_sample_run(op.ctx, ptr, n, 0, f.format, 0, 0, 1.0, None, C.byref(k)),
                   lib.bsk_sort_sample_reset(op.ctx),
                   lib.bsk_sort_sample_count(op.ctx, C.byref(k)),
                   lib.bsk_sort_splitters_build(op.ctx, BINS, C.byref(k32)),
                   lib.bsk_sort_splitters_set(op.ctx, b"a", offs, 1),
                   lib.bsk_sort_splitters_get(op.ctx, None, 0, None, C.byref(k32), C.byref(k)),
                   lib.bsk_sort_hist_run(op.ctx, ptr, n, 0, f.format, 0, 0, None, C.byref(k)),
                   lib.bsk_sort_hist_get(op.ctx, None, None),
                   lib.bsk_sort_hist_reset(op.ctx),
                   lib.bsk_sort_bucket_begin(op.ctx, 0, BINS),
                   lib.bsk_sort_bucket_add(op.ctx, ptr, n, 0, f.format, 0, 0, None),
                   lib.bsk_sort_bucket_finish(op.ctx, None, C.byref(_lib.Out()))):
            assert rc == _lib.BSK_ERR_INVALID_ARG and "not a Sort context" in err(op)


def profile_of(op):
    buf = C.create_string_buffer(1 << 16)
    check(lib.bsk_profile_dump(op.ctx, buf, len(buf)), op.ctx)
    return dict(x.split("=") for x in buf.value.decode().split(";") if x)


def test_stage_names_of_the_bucket_path():
    data, fastq = shape("fastq")
    f = frame(data, fastq, 3)
    with bsk.Operator("Sort", "{}", 0) as op:
        check(lib.bsk_profile_enable(op.ctx, 1), op.ctx)
        buckets, counts = bsk.SortBucketsPlan(op, f, Opts({}), len(data))
        got = b"".join(bsk.SortBucket(op, f, counts, lo, hi) for lo, hi in buckets)
        stages = profile_of(op)
    for s in ("k_sort_sample_keys", "k_sort_bins", "k_sort_hist", "k_sort_pick", "sort_bucket_sort"):
        assert s in stages, stages
    assert stages["k_sort_sample_keys"].endswith("/3") and stages["k_sort_bins"].endswith("/6") and stages["k_sort_pick"].endswith("/3")
    assert got == want_of("fastq", "{}")
    with bsk.Operator("Sort", "{}", 0) as op:
        check(lib.bsk_profile_enable(op.ctx, 1), op.ctx)
        (pid, ptr, n, on_dev, keep), = frame(data, fastq).partitions()
        out = _lib.Out()
        check(lib.bsk_sort_run(op.ctx, ptr, n, 0, bsk.FORMAT_FASTQ, 0, None, C.byref(out)), op.ctx)
        assert "k_sort_bins" not in profile_of(op)           # a plain Sort does not search


# ------------------------------------------------------------------ the command line
def cli(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([CLI, *args], capture_output=True, timeout=900, env=e)
    assert p.returncode == 0, p.stderr.decode()
    return p


def test_cli_sort_in_buckets(tmp_path):
    """two files, the first one without its final newline, unioned in order"""
    a, b = make(random.Random(50), 500, True), make(random.Random(51), 200, True, final_newline=False)
    fa, fb = str(tmp_path / "a.fq"), str(tmp_path / "b.fq")
    open(fa, "wb").write(a)
    open(fb, "wb").write(b)
    union = b + b"\n" + a
    out = str(tmp_path / "o")
    args = ["sort", fb, fa, "-o", out, "--merge"]
    want = oracle.sort(union, True)
    p = cli(args, {"BSK_CLI_TIMING": "1"})
    assert open(out, "rb").read() == want and "k_sort_bins" not in p.stderr.decode()              # one pass, as before
    os.remove(out)
    streamed = {"BSK_SORT_BUDGET_BYTES": "20000", "BSK_STREAM_PIECE_BYTES": "30000", "BSK_STAGE_BYTES": "4096"}
    p = cli(args, dict(streamed, BSK_CLI_TIMING="1"))
    assert open(out, "rb").read() == want
    err = p.stderr.decode()
    assert "k_sort_bins" in err and "k_sort_sample_keys" in err and "k_sort_pick" in err and "sort_bucket_sort" in err, err[-800:]
    assert int(err.split("sort in ")[1].split(" bucket")[0]) >= 3
    os.remove(out)
    for flags in (["-r"], ["-s", "-i", "-r"], ["-l"]):
        o = {"Reverse": "-r" in flags, "BySeq": "-s" in flags, "IgnoreCase": "-i" in flags, "ByLength": "-l" in flags}
        cli(args + flags, streamed)
        assert open(out, "rb").read() == oracle.sort(union, True, json.dumps(o)), flags
        os.remove(out)
    # an input that fits the budget but cannot be loaded whole goes through the buckets too
    p = cli(args, {"BSK_SORT_BUDGET_BYTES": str(1 << 30), "BSK_SHARD_FAIL_ALLOC": "1", "BSK_CLI_TIMING": "1"})
    assert open(out, "rb").read() == want and "sort in 1 bucket(s)" in p.stderr.decode()
    os.remove(out)
    # ... and without the switch it is told about it
    p = subprocess.run([CLI, *args], capture_output=True, timeout=900, env=dict(os.environ, BSK_SHARD_FAIL_ALLOC="1"))
    assert p.returncode != 0 and "BSK_SORT_BUDGET_BYTES" in p.stderr.decode()
    p = subprocess.run([CLI, "sort", fa, "--devices", "0-1", "-o", out], capture_output=True, timeout=900, env=dict(os.environ, **streamed))
    assert p.returncode != 0 and "runs on one device" in p.stderr.decode()
