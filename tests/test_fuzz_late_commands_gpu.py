"""Randomised cross-check of the commands that came after tests/test_fuzz_gpu.py was written -- `replace`, `fa2fq`, `sample`,
`shuffle` (one pass and in buckets of the draw) and `head-genome` -- against their plain-Python restatements (replace_ref.py,
fa2fq_ref.py, sample_ref.py, head_genome_ref.py), on the inputs of that file: empty sequences, no final newline, '>' and '@'
inside headers and quality lines, every kind of wrapping, hundreds of records of a few bytes, shards of a few dozen bytes.
Either both sides give the same bytes or both refuse (the rule of test_fuzz_gpu.one_case), and at most one case in five may end
as a refusal.  The FASTA file of a `fa2fq` case is made from the reads (test_fa2fq_gpu.fasta_entry); reads shorter than 12 bases
give many FASTA records with an EMPTY sequence, which match at position 0 and come back as empty sequence and quality lines
(PARITY FA2FQ) -- that is meant.  The seeds follow BSK_FUZZ_SEEDS (a quarter of them, at least 2), the run-time switches BSK_FUZZ_ENV."""
import os
import random

import pytest

import bigseqkit_amd as bsk
import oracle
import fa2fq_ref as F
import head_genome_ref as HG
import replace_ref
import sample_ref as R
from test_fuzz_gpu import rand_fasta, rand_fastq, rand_tiny, extra_env, dev
from test_sample_gpu import frame
from test_shuffle_buckets_gpu import BINS, py_hist
from test_replace_gpu import NAME_OPTS, SEQ_OPTS, run as replace_run, want as replace_want
from test_fa2fq_gpu import fasta_entry, run as fa2fq_run

pytestmark = pytest.mark.gpu

N_SEEDS = max(2, int(os.environ.get("BSK_FUZZ_SEEDS", "24")) // 4)
OPS = ("sample", "shuffle", "head-genome", "replace", "fa2fq")


class NoSequences(Exception):
    """PARITY FA2FQ, the `Before` errors: a FASTA file without a record is `no sequences found in fasta file: <path>`"""


REF_ERRORS = (oracle.OracleError, R.SampleError, HG.HeadGenomeError, replace_ref.ReplaceError, NoSequences)
WORDS = (b"Vibrio", b"cholerae", b"strain", b"M29", b"contig", b"x")


def seed64(rng):
    return rng.choice([11, 0, -1, (1 << 63) - 1, -(1 << 63), rng.randrange(-(1 << 63), 1 << 63)])


def described(rng, data, fastq):
    """the headers of `data` replaced by ID + description: record 0 has 1 - 5 words of WORDS; most records share exactly n1 of them
    (n1 = 0 .. 5, each as likely) and go on differently, the others have 0 - 5 random words, so every shared-prefix length occurs; about one
    record in ten has no description, in one case in five the first one"""
    lines = data.split(b"\n")
    heads = [i for i, l in enumerate(lines) if (i % 4 == 0 and l[:1] == b"@" if fastq else l[:1] == b">")]
    n1 = rng.randint(0, 5)
    desc0 = [rng.choice(WORDS) for _ in range(rng.randint(max(1, n1), 5))]
    first_bare = rng.random() < 0.2
    for k, i in enumerate(heads):
        if k == 0:
            ws = [] if first_bare else desc0
        elif rng.random() < 0.1:
            ws = []
        elif rng.random() < 0.88:
            tail = [rng.choice(WORDS) for _ in range(rng.randint(0, 5 - n1))]
            if n1 < len(desc0) and tail and tail[0] == desc0[n1]:
                tail = []
            ws = desc0[:n1] + tail
        else:
            ws = [rng.choice(WORDS) for _ in range(rng.randint(0, 5))]
        head = b"g%d" % k
        if ws:
            # (now and then two blanks behind the ID: the skip-two rule of PARITY HEADG eats the first letter of the description)
            head += (b"  " if rng.random() < 0.03 else rng.choice([b" ", b" ", b"\t"])) + ws[0]
            head += b"".join(rng.choice([b" ", b" ", b"\t", b"  "]) + w for w in ws[1:])
        elif rng.random() < 0.3:
            head += rng.choice([b" ", b"\t", b"  "])
        lines[i] = lines[i][:1] + head
    return b"\n".join(lines)


def draw_case(rng, tiny):
    """everything random about one case (the reference and the library draw nothing)"""
    op = rng.choice(OPS)
    c = {"op": op}
    if op == "replace":
        by_seq = rng.random() < 0.4
        c["opts"] = rng.choice(SEQ_OPTS if by_seq else NAME_OPTS)
        c["vm"] = by_seq and rng.random() < 0.5
        c["width"] = rng.choice([60, 0, 1, 13])
        fastq = rng.random() < (0.1 if by_seq else 0.5)    # (`-s` on FASTQ is refused by both sides)
    else:
        fastq = op == "fa2fq" or rng.random() < 0.5
    data = rand_tiny(rng, fastq) if tiny else (rand_fastq(rng) if fastq else rand_fasta(rng))
    c["fastq"] = fastq
    if op in ("sample", "shuffle"):
        c["seed"] = seed64(rng)
        c["parts"] = rng.choice([1, 2, 3, 7])
        c["device"] = rng.random() < 0.5
    if op == "sample":
        n = len(R.records(data, fastq))
        if rng.random() < 0.5:
            c["o"] = {"proportion": rng.choice([1.0, 0.5, 0.1, 1e-9, 2.0 ** -149])}
        else:
            c["o"] = {"number": rng.choice([1, n // 3, n, 5 * n])}
    elif op == "shuffle":
        c["budget"] = rng.randrange(4)
    elif op == "head-genome":
        data = described(rng, data, fastq)
        c.update(m=rng.choice([1, 2, 3]), window=rng.choice([0, 256, 4096]), parts=rng.choice([1, 3]), device=rng.random() < 0.5,
                 width=rng.choice([60, 0, 13]))
    elif op == "fa2fq":
        fa = [fasta_entry(rng, F.record_id(head), head, seq) for head, seq, _ in F.fastq_records(data)]
        fa = [e for e in fa if e is not None]
        rng.shuffle(fa)
        c.update(fasta=b"".join(fa), o={"OnlyPositiveStrand": True} if rng.random() < 0.3 else {}, parts=rng.choice([1, 3]))
    c["data"] = data
    return c


def reference(c):
    """(the bytes the restatement gives, what the library's side needs of it) -- or one of REF_ERRORS"""
    op, data, fastq = c["op"], c["data"], c["fastq"]
    if op == "sample":
        return R.sample(data, fastq, c["seed"], c["o"].get("number", 0), c["o"].get("proportion", 0.0)), None
    if op == "shuffle":
        return R.shuffle(data, fastq, c["seed"]), py_hist(R.records(data, fastq), c["seed"])
    if op == "head-genome":
        return HG.head_genome(data, fastq, c["m"], c["width"]), None
    if op == "replace":
        return replace_want(data, fastq, c["opts"], c["width"]), None
    if not F.read_fasta_map(c["fasta"]):
        raise NoSequences("no sequences found in fasta file")
    return F.fa2fq(data, c["fasta"], c["o"]), None


def shards(c):
    f = frame(c["data"], c["fastq"], c["parts"])
    return bsk.SeqFrame(f.format, [dev(bytes(s)) for s in f.shards]) if c["device"] else f


def library(c, hist, monkeypatch, tmp_path):
    """every answer of the library to the case (all of them must be the reference's bytes)"""
    op, data, fastq = c["op"], c["data"], c["fastq"]
    if op == "sample":
        return [bsk.Sample(shards(c), bsk.SeqKitSampleOptions(seed=c["seed"], **c["o"]))]
    if op == "shuffle":
        o = bsk.SeqKitShuffleOptions(seed=c["seed"])
        got = [bsk.Shuffle(frame(data, fastq), o), bsk.Shuffle(shards(c), o)]
        T, m = (sum(hist[0]), max(hist[0])) if hist else (1 << 30, 0)
        budget = [T, T // 2 + m, T // 5 + m, m][c["budget"]]
        f = shards(c)
        with bsk.Operator("Shuffle", o.to_json(), 0) as sh:
            counts = bsk.ShuffleHistRun(sh, f)
            seen = bsk.ShuffleHistGet(sh)
            assert hist is None or seen == hist, "the histogram"
            bounds = bsk.ShufflePlan(seen[0], budget)
            got.append(b"".join(bsk.ShuffleBucket(sh, f, counts, lo, hi) for lo, hi in zip(bounds[:-1], bounds[1:])))
        assert bounds[0] == 0 and bounds[-1] == BINS
        return got
    if op == "head-genome":
        monkeypatch.setenv("BSK_HEAD_GENOME_WINDOW", str(c["window"]))
        return [bsk.HeadGenome(shards(c), bsk.SeqKitHeadGenomeOptions(mini_common_words=c["m"], line_width=c["width"]))]
    if op == "replace":
        with monkeypatch.context() as mp:   # (a BSK_REPLACE of BSK_FUZZ_ENV comes back afterwards)
            if c["vm"]:
                mp.setenv("BSK_REPLACE", "vm")
            return [replace_run(data, fastq, c["opts"], c["width"])]
    return [fa2fq_run(tmp_path, data, c["fasta"], c["o"], parts=c["parts"])]


def one_case(c, monkeypatch, tmp_path):
    """both sides on one case: the same bytes, or both refuse (the library may decline what it documents as unsupported)"""
    try:
        (want, hist), werr = reference(c), None
    except REF_ERRORS as e:
        (want, hist), werr = (None, None), str(e)
    try:
        got, gerr = library(c, hist, monkeypatch, tmp_path), None
    except bsk.BskError as e:
        got, gerr = None, str(e)
    ctx = ({k: v for k, v in c.items() if k not in ("data", "fasta")}, c["data"][:300], c.get("fasta", b"")[:200])
    if werr is not None or gerr is not None:
        assert gerr is not None, ("the restatement failed, the library answered", werr, ctx)
        if werr is None:
            assert "not supported" in gerr or "not accepted" in gerr or "libbsk" in gerr, (gerr, ctx)
        elif c["op"] in ("head-genome", "fa2fq"):
            assert werr in gerr, (werr, gerr, ctx)   # the reference's own message ("no description: <ID>" names the lowest such record)
        return False
    for k, g in enumerate(got):
        assert g == want, (k, ctx)
    return True


def switches(seed, monkeypatch):
    monkeypatch.setenv("BSK_MIN_RANGE_BYTES", "4096")
    if seed % 3 == 0:
        monkeypatch.setenv("BSK_OUT", "slices")
    segcopy = (None, "off", "force")[(seed + seed // 3) % 3]
    if segcopy:
        monkeypatch.setenv("BSK_SEGCOPY", segcopy)
    extra_env(monkeypatch)


def cases_of(seed, tiny):
    rng = random.Random((88000 if tiny else 66000) + seed)
    return [draw_case(rng, tiny) for _ in range(120 if tiny else 60)]


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_fuzz_late_commands(seed, monkeypatch, tmp_path):
    switches(seed, monkeypatch)
    cases = cases_of(seed, False)
    agree = sum(one_case(c, monkeypatch, tmp_path) for c in cases)
    assert agree >= 0.8 * len(cases), (agree, len(cases))


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_fuzz_late_commands_tiny_inputs(seed, monkeypatch, tmp_path):
    """shards of a few dozen bytes (rand_tiny): one to three short records, tables of one entry, buckets of one record"""
    switches(seed, monkeypatch)
    cases = cases_of(seed, True)
    agree = sum(one_case(c, monkeypatch, tmp_path) for c in cases)
    assert agree >= 0.8 * len(cases), (agree, len(cases))
