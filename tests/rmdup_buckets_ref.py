"""`rmdup` in buckets of the key (PARITY.md RMDUPB) restated in plain Python, and the inputs of its tests: records, subjects,
fine bins (oracle.xxh64 -- the reference's own function), the histogram, the verdict."""
import functools
import json
import random

import oracle
import seqgen

BINS = 4096
RECORD_BYTES = 32   # BSK_RMDUP_BUCKET_RECORD_BYTES (include/bsk.h): k1, global index, offset, length per accumulated record

OPTION_SETS = ({}, {"ByName": True}, {"BySeq": True}, {"BySeq": True, "IgnoreCase": True})


def wrap(t, w):
    return b"\n".join(t[i:i + w] for i in range(0, len(t), w)) if w > 0 else t


def parse(data, fastq):
    """[(header without its marker, sequence)] of FASTA / FASTQ text, wrapped or not (a quality line ends the record when it
    has brought the length of the sequence)"""
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    recs, k = [], 0
    if fastq:
        while k < len(lines):
            head, seq, k = lines[k][1:], b"", k + 1
            while not lines[k].startswith(b"+"):
                seq, k = seq + lines[k], k + 1
            k, q = k + 1, 0
            if not seq:
                k += 1                                    # (the empty quality line)
            while q < len(seq):
                q, k = q + len(lines[k]), k + 1
            recs.append((head, seq))
        return recs
    for ln in lines:
        if ln.startswith(b">"):
            recs.append([ln[1:], b""])
        else:
            recs[-1][1] += ln
    return [tuple(r) for r in recs]


def subject(rec, o):
    """PARITY RMDUPB: the sequence with BySeq, the whole header with ByName, else the ID; lower-cased with IgnoreCase"""
    head, seq = rec
    if o.get("BySeq"):
        s = seq
    elif o.get("ByName"):
        s = head
    else:
        sp = head.find(b" ")
        if sp <= 0:
            sp = head.find(b"\t")
        s = head[:sp] if sp > 0 else head
    return s.lower() if o.get("IgnoreCase") else s


def bin_of(s):
    return oracle.xxh64(s) >> 52


def py_hist(subjects):
    hb, hr = [0] * BINS, [0] * BINS
    for s in subjects:
        b = bin_of(s)
        hb[b] += len(s) + RECORD_BYTES
        hr[b] += 1
    return hb, hr


def py_verdict(subjects):
    """removed[g] = some g' < g has the same subject bytes"""
    seen, out = set(), []
    for s in subjects:
        out.append(1 if s in seen else 0)
        seen.add(s)
    return bytes(out)


def with_repeats(rng, recs):
    """half of the records repeat an earlier one -- the whole record (two times in five), its ID under another description, its
    sequence under another name, or its sequence in the other case -- so that under every option set between a fifth and two
    fifths of the subjects repeat; the LAST record repeats the FIRST"""
    out = []
    for i, (head, seq) in enumerate(recs):
        if i and (rng.random() < 1 / 2 or i == len(recs) - 1):
            h0, s0 = out[0] if i == len(recs) - 1 else out[rng.randrange(i)]
            v = 0 if i == len(recs) - 1 else max(0, rng.randrange(5) - 1)
            if v == 0:
                head, seq = h0, s0
            elif v == 1:
                head = h0.split(b" ")[0] + b" other %d" % i
            elif v == 2:
                seq = s0
            else:
                seq = s0.swapcase()
        out.append((head, seq))
    return out


def fastq_text(rng, recs, width=0):
    out = []
    for head, seq in recs:
        q = bytes(rng.choice(b"ABCDEFGHI") for _ in range(len(seq)))
        out.append(b"@" + head + b"\n" + wrap(seq, width) + b"\n+\n" + wrap(q, width) + b"\n")
    return b"".join(out)


def fasta_text(recs, width):
    return b"".join(b">" + head + b"\n" + (wrap(seq, width) + b"\n" if seq else b"") for head, seq in recs)


@functools.lru_cache(maxsize=None)
def shape(name, n=500):
    """(data, fastq) of the named input: "fastq" strict, "fastq wrapped" at 7, "fasta 7" / "fasta 60" wrapped at that width"""
    rng = random.Random(20 + len(name))
    if name.startswith("fastq"):
        recs = with_repeats(rng, parse(seqgen.random_fastq(rng, n, 1, 120, alphabet="ACGTNacgt"), True))
        return fastq_text(rng, recs, 7 if "wrapped" in name else 0), True
    recs = with_repeats(rng, parse(seqgen.random_fasta(rng, n, 0, 200, alphabet="ACGTNacgt"), False))
    return fasta_text(recs, int(name.split()[1])), False


SHAPES = ("fastq", "fastq wrapped", "fasta 7", "fasta 60")


@functools.lru_cache(maxsize=None)
def restated(name, oj):
    """(records, subjects, bytes per bin, records per bin) of the named shape under the options `oj` (JSON)"""
    data, fastq = shape(name)
    o = json.loads(oj)
    recs = parse(data, fastq)
    subs = [subject(r, o) for r in recs]
    return (recs, subs) + py_hist(subs)


@functools.lru_cache(maxsize=None)
def want_of(name, oj):
    data, fastq = shape(name)
    return oracle.rmdup(data, fastq, oj)


def cuts_of(data, fastq, parts):
    """byte cuts of `data` into 1, 3 or 7 shards on record starts (the oracle's); 7: the first shard holds one record and the
    fourth is empty"""
    starts = [s for s, _ in oracle.record_spans(data, fastq)]
    n = len(starts)
    if parts == 1 or n < 8:
        return [0, len(data)]
    if parts == 3:
        return [0, starts[n // 3], starts[2 * n // 3], len(data)]
    mid = starts[n // 2]
    return [0, starts[1], starts[n // 5], mid, mid, starts[2 * n // 3], starts[n - 3], len(data)]


def budgets_of(hb):
    """the three budgets of the tests: one bucket; at least 8 buckets; the fullest bin"""
    return sum(hb), max(max(hb), sum(hb) // 12), max(hb)
