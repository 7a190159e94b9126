"""`concat` in buckets of the key (PARITY.md CONB) restated in plain Python.  Records, subjects, fine bins, the histogram, the
cuts and the budgets are those of rmdup_buckets_ref.py -- the subject of `concat` is the ID, rmdup's under its default options --,
the shapes, the files and the text cost those of pair_buckets_ref.py.  What is `concat`'s own: the head of a record, the weights
C and W of a head, the shift and the cost of the window bins, the collection rule of a window and the composition of both phases
by intervals."""
import functools
import json

import oracle
import pair_buckets_ref as P
import rmdup_buckets_ref as R

WINDOW_BINS = R.BINS


# ------------------------------------------------------------------ the definition
def py_head(subs1, subs2):
    """head over the global index (file 1, then file 2): the lowest record of file 1 with the same subject bytes, None when
    file 1 has none"""
    first = {}
    for i, s in enumerate(subs1):
        first.setdefault(s, i)
    return [first.get(s) for s in list(subs1) + list(subs2)]


def py_weights(head, n1, costs2):
    """(C, W) over the index inside file 1: the number and the text costs of the records of file 2 whose head it is"""
    C, W = [0] * n1, [0] * n1
    for h, t in zip(head[n1:], costs2):
        if h is not None:
            C[h] += 1
            W[h] += t
    return C, W


def window_shift(n1):
    """the least shift s with (n1 - 1) >> s < 4096 (n1 >= 1; 0 for an empty file 1)"""
    s = 0
    while n1 and (n1 - 1) >> s >= WINDOW_BINS:
        s += 1
    return s


def py_costs(head, C, W, costs1):
    """cost(a) = t(a) * (1 + C[h]) + 2 * W[h], h = head(a)"""
    return [t * (1 + C[h]) + 2 * W[h] for t, h in zip(costs1, head)]


def window_hist(costs):
    hb, hr = [0] * WINDOW_BINS, [0] * WINDOW_BINS
    s = window_shift(len(costs))
    for a, c in enumerate(costs):
        hb[a >> s] += c
        hr[a >> s] += 1
    return hb, hr


def window_members(head, n1, lo_bin, hi_bin):
    """the collection rule: (records of file 1 of the bins [lo_bin, hi_bin), records of file 2 (indices inside the file) whose
    head is the head of one of them), both in file order"""
    s = window_shift(n1)
    a = [i for i in range(n1) if lo_bin <= i >> s < hi_bin]
    marked = {head[i] for i in a}
    b = [j for j, h in enumerate(head[n1:]) if h is not None and h in marked]
    return a, b


def tail_members(head, n1):
    """the records of file 2 (indices inside the file) without a head"""
    return [j for j, h in enumerate(head[n1:]) if h is None]


def heads_by_intervals(subs1, subs2, bounds):
    """the match phase composed: the heads decided inside every interval of fine bins on its own -- the records of the interval
    in input order, file 1 first, the first record of a subject names its group --, put back by global index"""
    n1 = len(subs1)
    subs = list(subs1) + list(subs2)
    bins = [R.bin_of(s) for s in subs]
    head = ["undecided"] * len(subs)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        first = {}
        for g in (g for g, b in enumerate(bins) if lo <= b < hi):
            f = first.setdefault(subs[g], g)
            assert head[g] == "undecided"                                            # a global index belongs to one bucket only
            head[g] = f if f < n1 else None
    return head


def record_texts(text, fastq):
    """the text of every record of a file, as it stands"""
    starts = [s for s, _ in oracle.record_spans(text, fastq)] + [len(text)]
    return [text[a:b] for a, b in zip(starts[:-1], starts[1:])]


def concat_by_windows(texts, fastq, head, wbounds, oj):
    """the join phase composed with the oracle: oracle.concat on the accumulation of every window, joined, and with Full the
    tail -- the records of file 2 without a head, which the oracle prints as records of one file only.  Also checks that a
    collected record of file 2 has a mate inside its window.  -> (bytes, [(records of file 1, of file 2) per window])"""
    one, two = (record_texts(t, fastq) for t in texts)
    n1 = len(one)
    out, sizes = [], []
    for lo, hi in zip(wbounds[:-1], wbounds[1:]):
        a, b = window_members(head, n1, lo, hi)
        heads_a = {head[i] for i in a}
        assert all(head[n1 + j] in heads_a for j in b)
        sizes.append((len(a), len(b)))
        if a:
            out.append(oracle.concat(b"".join(one[i] for i in a), b"".join(two[j] for j in b), fastq, oj))
    if json.loads(oj).get("Full"):
        out.append(oracle.concat(b"", b"".join(two[j] for j in tail_members(head, n1)), fastq, oj))
    return b"".join(out), sizes


# ------------------------------------------------------------------ the inputs
@functools.lru_cache(maxsize=None)
def restated(name, variant):
    """dict: recs, subs (per file), hist = (bytes, records) per fine bin over the union, head, C, W, costs (t per file), cost
    (per record of file 1), whist = the window histogram"""
    texts, fastq = P.files_text(name, variant)
    recs = [R.parse(t, fastq) for t in texts]
    subs = [[R.subject(r, {}) for r in rs] for rs in recs]
    width = 0 if fastq else int(name.split()[1])
    costs = [[P.text_cost(r, fastq, width) for r in rs] for rs in recs]
    head = py_head(*subs)
    C, W = py_weights(head, len(subs[0]), costs[1])
    cost = py_costs(head, C, W, costs[0])
    return {"recs": recs, "subs": subs, "hist": R.py_hist(subs[0] + subs[1]), "head": head, "C": C, "W": W, "costs": costs, "cost": cost,
            "whist": window_hist(cost)}


@functools.lru_cache(maxsize=None)
def want_of(name, variant, oj):
    texts, fastq = P.files_text(name, variant)
    return oracle.concat(texts[0], texts[1], fastq, oj)


def budget_of(hb, fraction):
    """the budget that cuts a histogram into about 1 / fraction parts: the fullest bin at least"""
    return max(max(hb), int(sum(hb) * fraction) + 1)
