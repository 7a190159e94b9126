"""`common` in buckets of the key (PARITY.md COMB) restated in plain Python, and the inputs of its tests.  Records, subjects, fine
bins, the histogram and the shapes are those of rmdup_buckets_ref.py -- the subject of `common` is rmdup's, under the same three
options; what differs is the verdict: one KEEP bit per record of the FIRST file, set for the first occurrence of a subject that
every file holds."""
import functools
import json
import random

import oracle
import rmdup_buckets_ref as R

OPTION_SETS = ({}, {"ByName": True}, {"BySeq": True}, {"IgnoreCase": True}, {"BySeq": True, "IgnoreCase": True},
               {"ByName": True, "IgnoreCase": True, "Config": {"LineWidth": 20}})
N_PER_FILE = 500


def subject_opts(o):
    """the line width (Config) is not the subject's business"""
    return {k: v for k, v in o.items() if k != "Config"}


def file_of(file_records, g):
    """the file of global index g: the number of running sums of file_records that are <= g"""
    f, s = 0, 0
    for k in file_records:
        s += k
        f += 1 if s <= g else 0
    return f


def py_bits(subjects, file_records):
    """subjects: those of the union, in global order.  bits[g] for g < file_records[0]: 1 iff no g' < g has the same subject
    bytes and every file holds a record with those bytes"""
    mask, first = {}, {}
    for g, s in enumerate(subjects):
        mask[s] = mask.get(s, 0) | 1 << file_of(file_records, g)
        first.setdefault(s, g)
    full = (1 << len(file_records)) - 1
    return bytes(1 if mask[s] == full and first[s] == g else 0 for g, s in enumerate(subjects[:file_records[0]]))


def py_common(files_recs, o):
    """[(header, sequence)] of the first file: the records that `common` prints, in order"""
    so = subject_opts(o)
    subs = [R.subject(r, so) for recs in files_recs for r in recs]
    bits = py_bits(subs, [len(recs) for recs in files_recs])
    return [r for r, b in zip(files_recs[0], bits) if b]


# ------------------------------------------------------------------ the inputs
@functools.lru_cache(maxsize=None)
def files_records(name, nfiles):
    """`nfiles` lists of N_PER_FILE (header, sequence) for the shape `name`, built file by file from shared pools of IDs and
    sequences: a record is a pool record as it stands (one in three), a pool ID under another description, a pool name in the
    other case, a pool sequence under a name of its own, or that sequence in the other case; so under every option set some
    subjects lie in every file, some in some files, and some come twice in a file"""
    rng = random.Random(70 + len(name) + nfiles)
    fastq = name.startswith("fastq")
    pool = []
    for j in range(400):
        L = rng.randint(1, 120) if fastq else rng.randint(0, 200)
        head = b"r%d" % j + (b" desc %d" % rng.randrange(100) if rng.random() < 0.5 else b"")
        pool.append((head, bytes(rng.choice(b"ACGTNacgt") for _ in range(L))))
    files = []
    for f in range(nfiles):
        recs = []
        for i in range(N_PER_FILE):
            head, seq = pool[rng.randrange(len(pool))]
            v = rng.randrange(6)
            if v == 2:
                head, seq = head.split(b" ")[0] + b" other %d.%d" % (f, i), pool[rng.randrange(len(pool))][1]
            elif v == 3:
                head, seq = head.swapcase(), pool[rng.randrange(len(pool))][1]
            elif v >= 4:
                head, seq = b"f%d.%d own" % (f, i), seq if v == 4 else seq.swapcase()
            recs.append((head, seq))
        files.append(recs)
    return files


@functools.lru_cache(maxsize=None)
def files_text(name, nfiles):
    """([text of every file], fastq) of files_records in the layout of the shape"""
    rng = random.Random(7)
    recs = files_records(name, nfiles)
    if name.startswith("fastq"):
        return [R.fastq_text(rng, r, 7 if "wrapped" in name else 0) for r in recs], True
    return [R.fasta_text(r, int(name.split()[1])) for r in recs], False


@functools.lru_cache(maxsize=None)
def restated(name, nfiles, oj):
    """(records per file, subjects of the union, bytes per bin, records per bin, keep bits of file 1, file_records)"""
    o = subject_opts(json.loads(oj))
    texts, fastq = files_text(name, nfiles)
    recs = [R.parse(t, fastq) for t in texts]
    subs = [R.subject(r, o) for rs in recs for r in rs]
    file_records = [len(rs) for rs in recs]
    return (recs, subs) + R.py_hist(subs) + (py_bits(subs, file_records), file_records)


@functools.lru_cache(maxsize=None)
def want_of(name, nfiles, oj):
    texts, fastq = files_text(name, nfiles)
    return oracle.common(list(texts), fastq, oj)


def tiny_text(recs, fastq):
    """records whose sequence fits one line, as Format prints them"""
    if fastq:
        return b"".join(b"@" + h + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for h, s in recs)
    return b"".join(b">" + h + b"\n" + s + b"\n" for h, s in recs)


# ------------------------------------------------------------------ distinct subjects under one key
@functools.lru_cache(maxsize=None)
def masked_key_files():
    """two FASTQ files of 3000 distinct IDs each, q0 .. q2999 and q1500 .. q4499, shuffled: half of each file is shared"""
    rng = random.Random(16)
    files = []
    for lo in (0, 1500):
        recs = [(b"q%d" % i, bytes(rng.choice(b"ACGTacgt") for _ in range(rng.randint(20, 40)))) for i in range(lo, lo + 3000)]
        rng.shuffle(recs)
        files.append(recs)
    return files


def masked_groups(subs, file_records, bits=16):
    """what the key path sees when only the low `bits` bits of XXH64 group: (flagged records, kept texts that share their key
    group with another text, texts of file 1 that are not kept and share their key group with another text).  A record is
    flagged when its text differs from the first text of its masked key."""
    keep = py_bits(subs, file_records)
    first_text, texts, flagged = {}, {}, 0
    for s in subs:
        k = oracle.xxh64(s) & ((1 << bits) - 1)
        flagged += 1 if s != first_text.setdefault(k, s) else 0
        texts.setdefault(k, set()).add(s)
    kept_shared = sum(1 for s, b in zip(subs, keep) if b and len(texts[oracle.xxh64(s) & ((1 << bits) - 1)]) > 1)
    dropped = {s for s, b in zip(subs[:file_records[0]], keep) if not b}
    dropped_shared = sum(1 for s in dropped if len(texts[oracle.xxh64(s) & ((1 << bits) - 1)]) > 1)
    return flagged, kept_shared, dropped_shared


# ------------------------------------------------------------------ sequences that differ in their last byte only
LANE_LENGTHS = (0, 1, 15, 16, 17, 127, 128, 129, 255, 256, 257)


def lane_sequence(L, k=0, last=b"A"):
    """a sequence of L bytes that depends on k, ending in `last`"""
    return ((b"%d." % k + b"ACGT" * 70)[:L - 1] + last) if L else b""


@functools.lru_cache(maxsize=None)
def last_byte_collision(L, bits=16):
    """(s, t): two sequences of L bytes that differ in their last byte only and agree in the low `bits` bits of XXH64 -- the
    comparison of the key path, not the key, has to tell them apart; None when L < 2 (no prefix to vary in the search)"""
    if L < 2:
        return None
    letters = [bytes([c]) for c in b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"]
    for k in range(100000):
        seen = {}
        for c in letters:
            s = lane_sequence(L, k, c)
            t = seen.setdefault(oracle.xxh64(s) & ((1 << bits) - 1), s)
            if t != s:
                return t, s
    raise AssertionError("no collision found")
