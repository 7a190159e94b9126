"""`pair` in buckets of the key (PARITY.md PAIRB) restated in plain Python, and the inputs of its tests.  Records, subjects, fine
bins, the histogram, the cuts and the budgets are those of rmdup_buckets_ref.py -- the subject of `pair` is the ID, rmdup's under
its default options.  What is `pair`'s own: the ordinal of a record inside its file, the pairs, the output position `pos`, the
order bins with their shift, and the composition of both bucket phases by intervals."""
import functools
import random

import oracle
import rmdup_buckets_ref as R

N_PER_FILE = 500
ORDER_BINS = R.BINS


# ------------------------------------------------------------------ the definition
def py_pair(subs1, subs2):
    """(paired1[i], paired2[j], mate[j] = index in file 1 of the mate of record j of file 2 or None, pos1[i], pos2[j], P):
    the k-th record of a subject in file 1 goes with the k-th of file 2; pos of a paired record of file 1 = the paired records
    of file 1 in front of it, pos of a record of file 2 = the pos of its mate; None: unpaired"""
    where1 = {}
    for i, s in enumerate(subs1):
        where1.setdefault(s, []).append(i)
    seen2, mate = {}, []
    for s in subs2:
        k = seen2.get(s, 0)
        seen2[s] = k + 1
        mate.append(where1[s][k] if k < len(where1.get(s, ())) else None)
    paired1 = [False] * len(subs1)
    for i in mate:
        if i is not None:
            paired1[i] = True
    pos1, p = [], 0
    for f in paired1:
        pos1.append(p if f else None)
        p += 1 if f else 0
    pos2 = [None if i is None else pos1[i] for i in mate]
    return paired1, [i is not None for i in mate], mate, pos1, pos2, p


def in_mate_order(pos2):
    """file 2 is in mate order iff pos of every paired record equals the paired records of file 2 in front of it"""
    return [p for p in pos2 if p is not None] == list(range(sum(1 for p in pos2 if p is not None)))


def py_outputs(recs1, recs2, save_unpaired=True):
    """the four outputs as lists of records: paired.1, paired.2, unpaired.1, unpaired.2"""
    paired1, paired2, mate, pos1, pos2, P = py_pair([R.subject(r, {}) for r in recs1], [R.subject(r, {}) for r in recs2])
    by_pos = sorted((p, j) for j, p in enumerate(pos2) if p is not None)
    out = ([r for r, f in zip(recs1, paired1) if f], [recs2[j] for _, j in by_pos])
    if not save_unpaired:
        return out + ([], [])
    return out + ([r for r, f in zip(recs1, paired1) if not f], [r for r, f in zip(recs2, paired2) if not f])


def order_shift(P):
    """the least shift s with (P - 1) >> s < 4096 (P >= 1)"""
    s = 0
    while (P - 1) >> s >= ORDER_BINS:
        s += 1
    return s


def text_cost(rec, fastq, width=0):
    """the bytes a record adds to an order bin: its text + newline (FASTQ: the 4-line text)"""
    head, seq = rec
    if fastq:
        return len(head) + 2 * len(seq) + 6
    return len(R.fasta_text([rec], width))


def order_hist(pos2, costs, P):
    hb, hr = [0] * ORDER_BINS, [0] * ORDER_BINS
    if P:
        s = order_shift(P)
        for p, c in zip(pos2, costs):
            if p is not None:
                hb[p >> s] += c
                hr[p >> s] += 1
    return hb, hr


def pairs_by_intervals(subs1, subs2, bounds):
    """the match phase composed: the pairs decided inside every interval of fine bins on its own -- the records of the interval
    in input order, file 1 first --, put back by global index: (paired1, paired2, mate)"""
    n1 = len(subs1)
    subs = list(subs1) + list(subs2)
    bins = [R.bin_of(s) for s in subs]
    paired, mate = [None] * len(subs), [None] * len(subs2)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        idx = [g for g, b in enumerate(bins) if lo <= b < hi]
        a = [g for g in idx if g < n1]
        b = [g - n1 for g in idx if g >= n1]
        p1, p2, m, _, _, _ = py_pair([subs1[g] for g in a], [subs2[j] for j in b])
        for g, f in zip(a, p1):
            assert paired[g] is None                                                 # a global index belongs to one bucket only
            paired[g] = f
        for j, f, i in zip(b, p2, m):
            assert paired[n1 + j] is None
            paired[n1 + j] = f
            mate[j] = None if i is None else a[i]
    return paired[:n1], paired[n1:], mate


def order_by_intervals(pos2, P, bounds):
    """the order phase composed: the records of file 2 (indices) of every interval of order bins in ascending pos, joined"""
    out = []
    s = order_shift(P) if P else 0
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        out += [j for _, j in sorted((p, j) for j, p in enumerate(pos2) if p is not None and lo <= p >> s < hi)]
    return out


# ------------------------------------------------------------------ the inputs
VARIANTS = ("ordered", "shuffled")


@functools.lru_cache(maxsize=None)
def files_records(name, variant):
    """two lists of N_PER_FILE (header, sequence) for the shape `name`.  File 1 holds about 400 IDs, some of them twice; file 2
    keeps the first occurrences of most of them in the order of file 1, with records of its own in between -- so it is in mate
    order -- and in the "shuffled" variant the same records in another order.  r7 comes twice in file 1 and once in file 2,
    r11 twice in both, r13 once in file 1 and twice in file 2"""
    rng = random.Random(90 + len(name))
    fastq = name.startswith("fastq")

    def seq():
        L = rng.randint(1, 120) if fastq else rng.randint(0, 200)
        return bytes(rng.choice(b"ACGTNacgt") for _ in range(L))

    def head(i):
        return b"r%d" % i + (b" desc %d" % rng.randrange(100) if rng.random() < 0.5 else b"")

    ids = list(range(400))
    for dup in (7, 11) + tuple(rng.sample(range(20, 400), 30)):
        ids.insert(rng.randrange(len(ids) + 1), dup)
    quota = {i: (ids.count(i) if rng.random() < 0.8 else rng.randrange(ids.count(i))) for i in set(ids)}
    quota.update({7: 1, 11: 2, 13: 1})
    one, two, own1, own2 = [], [], 0, 0
    for i in ids:
        one.append((head(i), seq()))
        if quota[i] > 0:
            quota[i] -= 1
            two.append((head(i), seq()))
            if i == 13:
                two.append((head(13), seq()))
        if rng.random() < 0.1:
            two.append((b"only2.%d x" % own2, seq()))
            own2 += 1
    for f, n, tag in ((one, len(one), b"only1.%d"), (two, len(two), b"extra2.%d")):
        assert n <= N_PER_FILE, n
        for k in range(N_PER_FILE - n):
            f.insert(rng.randrange(len(f) + 1), (tag % k, seq()))
    if variant == "shuffled":
        random.Random(3).shuffle(two)
    return one, two


@functools.lru_cache(maxsize=None)
def files_text(name, variant):
    """((text of file 1, text of file 2), fastq) in the layout of the shape"""
    rng = random.Random(7)
    recs = files_records(name, variant)
    if name.startswith("fastq"):
        return tuple(R.fastq_text(rng, r, 7 if "wrapped" in name else 0) for r in recs), True
    return tuple(R.fasta_text(r, int(name.split()[1])) for r in recs), False


@functools.lru_cache(maxsize=None)
def restated(name, variant):
    """dict: recs (per file), subs (per file), hist = (bytes, records) per fine bin over the union, pair = py_pair(...), order_hist"""
    texts, fastq = files_text(name, variant)
    recs = [R.parse(t, fastq) for t in texts]
    subs = [[R.subject(r, {}) for r in rs] for rs in recs]
    pair = py_pair(*subs)
    width = 0 if fastq else int(name.split()[1])
    costs = [text_cost(r, fastq, width) for r in recs[1]]
    return {"recs": recs, "subs": subs, "hist": R.py_hist(subs[0] + subs[1]), "pair": pair, "order_hist": order_hist(pair[4], costs, pair[5])}


def pos_list(pair):
    """pos over the global index: file 1, then file 2"""
    return list(pair[3]) + list(pair[4])


@functools.lru_cache(maxsize=None)
def want_of(name, variant, oj):
    texts, fastq = files_text(name, variant)
    return oracle.pair(texts[0], texts[1], fastq, oj)


def tiny_text(recs, fastq):
    """records whose sequence fits one line, as Format prints them"""
    if fastq:
        return b"".join(b"@" + h + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for h, s in recs)
    return b"".join(b">" + h + b"\n" + s + b"\n" for h, s in recs)


# ------------------------------------------------------------------ distinct subjects under one key
@functools.lru_cache(maxsize=None)
def masked_key_files():
    """two FASTQ files of 3000 distinct IDs each, q0 .. q2999 and q1500 .. q4499, shuffled: half of each file has a mate"""
    rng = random.Random(16)
    files = []
    for lo in (0, 1500):
        recs = [(b"q%d" % i, bytes(rng.choice(b"ACGTacgt") for _ in range(rng.randint(20, 40)))) for i in range(lo, lo + 3000)]
        rng.shuffle(recs)
        files.append(recs)
    return files


def masked_groups(subs1, subs2, bits=16):
    """what the key path sees when only the low `bits` bits of XXH64 group: (flagged records, flagged records that are paired,
    flagged records of file 1 that stay unpaired).  A record is flagged when its text differs from the first text of its masked
    key over file 1 followed by file 2."""
    paired1, paired2 = py_pair(subs1, subs2)[:2]
    first_text, flagged, flagged_paired, flagged_alone1 = {}, 0, 0, 0
    for g, (s, f) in enumerate(zip(list(subs1) + list(subs2), paired1 + paired2)):
        if s != first_text.setdefault(oracle.xxh64(s) & ((1 << bits) - 1), s):
            flagged += 1
            flagged_paired += 1 if f else 0
            flagged_alone1 += 1 if not f and g < len(subs1) else 0
    return flagged, flagged_paired, flagged_alone1


# ------------------------------------------------------------------ IDs that differ in their last byte only
LANE_LENGTHS = (0, 1, 15, 16, 17, 127, 128, 129, 255, 256, 257)


def lane_id(L, k=0, last=b"A"):
    """an ID of L bytes (no blank) that depends on k, ending in `last`; L = 0: the empty ID"""
    return ((b"%d." % k + b"ACGT" * 70)[:L - 1] + last) if L else b""


@functools.lru_cache(maxsize=None)
def last_byte_collision(L, bits=16):
    """(s, t): two IDs of L bytes that differ in their last byte only and agree in the low `bits` bits of XXH64; None when L < 2"""
    if L < 2:
        return None
    letters = [bytes([c]) for c in b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"]
    for k in range(100000):
        seen = {}
        for c in letters:
            s = lane_id(L, k, c)
            t = seen.setdefault(oracle.xxh64(s) & ((1 << bits) - 1), s)
            if t != s:
                return t, s
    raise AssertionError("no collision found")
