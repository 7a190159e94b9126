"""`rename` in buckets of the key (PARITY.md RENB) restated in plain Python: the ordinal of a record inside its group of equal
subjects, and `rename` of parsed records.  Records, subjects, fine bins, the histogram and the shapes are those of
rmdup_buckets_ref.py -- the subject of `rename` is rmdup's without BySeq and IgnoreCase."""
import functools
import json

import oracle
import rmdup_buckets_ref as R

OPTION_SETS = ({}, {"ByName": True})


def py_ordinals(subjects):
    """ord[g] = the number of g' < g with the same subject bytes"""
    seen, out = {}, []
    for s in subjects:
        out.append(seen.get(s, 0))
        seen[s] = out[-1] + 1
    return out


def id_desc(head):
    """ID and description of a header under the default ID rule, as the reference's parseHeadIDAndDesc cuts them: the ID ends at
    the first space (none: the first tab); the description begins behind the blanks that follow, which are skipped in twos"""
    for sep in (b" ", b"\t"):
        i = head.find(sep)
        if i > 0:
            j = i + 1
            while j < len(head) and head[j] in b" \t":
                j += 2
            return head[:i], head[j:]
    return head, b""


def py_rename(recs, o):
    """[(header, sequence)]: the header of a record with ordinal k > 0 is ID + "_k " + Desc, the others are the input's"""
    out = []
    for (head, seq), k in zip(recs, py_ordinals([R.subject(r, o) for r in recs])):
        if k:
            rid, desc = id_desc(head)
            head = rid + b"_%d " % k + desc
        out.append((head, seq))
    return out


def tiny_text(recs, fastq):
    """records whose sequence fits one line, as Format prints them"""
    if fastq:
        return b"".join(b"@" + h + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for h, s in recs)
    return b"".join(b">" + h + b"\n" + s + b"\n" for h, s in recs)


@functools.lru_cache(maxsize=None)
def restated(name, oj):
    """(records, subjects, bytes per bin, records per bin, ordinals) of the shape R.shape(name) under the options `oj` (JSON;
    LineWidth is not the subject's business)"""
    o = {k: v for k, v in json.loads(oj).items() if k != "LineWidth"}
    recs, subs, hb, hr = R.restated(name, json.dumps(o))
    return recs, subs, hb, hr, py_ordinals(subs)


@functools.lru_cache(maxsize=None)
def want_of(name, oj):
    data, fastq = R.shape(name)
    return oracle.rename(data, fastq, oj)


def masked_key_input():
    """the FASTQ text of test_distinct_subjects_under_one_key_are_kept_apart (tests/test_rmdup_buckets_gpu.py): 3000 IDs and 600
    repeats of them, shuffled"""
    import random
    rng = random.Random(16)
    recs = []
    for i in range(3000):
        seq = "".join(rng.choice("ACGTacgt") for _ in range(rng.randint(20, 40)))
        recs.append(("q%d" % i, seq))
    recs += [rng.choice(recs[:3000]) for _ in range(600)]
    rng.shuffle(recs)
    return "".join("@%s\n%s\n+\n%s\n" % (h, s, "I" * len(s)) for h, s in recs).encode()


def masked_groups(subs, bits=16):
    """what the key path sees when only the low `bits` bits of XXH64 group: (flagged records, flagged texts with two or more
    records, flagged texts with three or more, key groups whose first text AND an intruding text are repeated).  A record is
    flagged when its text differs from the first text of its masked key."""
    first_text, flagged, per_text, first_count = {}, 0, {}, {}
    for s in subs:
        k = oracle.xxh64(s) & ((1 << bits) - 1)
        t0 = first_text.setdefault(k, s)
        if s != t0:
            flagged += 1
            per_text[(k, s)] = per_text.get((k, s), 0) + 1
        else:
            first_count[k] = first_count.get(k, 0) + 1
    both = {k for (k, s), n in per_text.items() if n >= 2 and first_count[k] >= 2}
    return flagged, sum(1 for n in per_text.values() if n >= 2), sum(1 for n in per_text.values() if n >= 3), len(both)
