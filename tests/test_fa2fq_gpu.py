"""Parity of `fa2fq` (bigseqkit-lib/fa2fq.go, PARITY.md FA2FQ) on the GPU: every output byte-exact against
tests/fa2fq_ref.py and the hand-written fixtures."""
import ctypes as C
import json
import os
import random
import subprocess

import pytest

import bigseqkit_amd as bsk
from bigseqkit_amd._lib import BskError, Out, lib, check
import fa2fq_ref as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "fa2fq_fixtures.json")))
CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")
SEED, N_RANDOM = 20, 300
LANE_POS = 64  # FA2FQ_LANE_POS (ops_fa2fq.hpp): start positions up to which one lane searches a record, above a wave does

_RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def rc(s):
    return s[::-1].translate(_RC)


def dna(rng, n, letters="ACGT"):
    return "".join(rng.choices(letters, k=n)).encode()


def record(name, seq, qual=None, rng=None):
    if qual is None:
        qual = bytes(33 + (7 * i + len(seq)) % 60 for i in range(len(seq))) if rng is None else bytes(rng.choices(range(33, 100), k=len(seq)))
    return b"@" + name + b"\n" + seq + b"\n+\n" + qual + b"\n"


def opts_json(fasta_path, opts):
    cfg = {"Quiet": True, "SeqType": opts.get("SeqType", "dna")}
    if opts.get("IDRegexp"):
        cfg["IDRegexp"] = opts["IDRegexp"]
    return json.dumps({"Config": cfg, "FastaFile": str(fasta_path), "OnlyPositiveStrand": bool(opts.get("OnlyPositiveStrand", False))})


class _Opts:
    def __init__(self, js):
        self.js = js

    def to_json(self):
        return self.js


_n = [0]


def run(tmp_path, fastq, fasta, opts=None, parts=1, fasta_format=False):
    _n[0] += 1
    path = tmp_path / ("t%d.fa" % _n[0])
    path.write_bytes(fasta)
    read = bsk.ReadFASTAN if fasta_format else bsk.ReadFASTQN
    return bsk.Fa2Fq(read(fastq, parts), _Opts(opts_json(path, opts or {})))


_NEXT_BASE = {65: 67, 67: 71, 71: 84, 84: 65}


def fasta_entry(rng, name, head, seq):
    """The FASTA record made from one read (ID `name`, full header `head`), or None: the read is left out, or a random slice
    of it is kept as it is, under another name, reverse-complemented or with one base changed.  (Reads shorter than 12 bases
    give slices of any length, the empty one included.)"""
    L = len(seq)
    fate = rng.random()
    if fate < 0.12:
        return None  # not in the FASTA file
    m = rng.randint(min(12, L), L)
    a = rng.randint(0, L - m)
    s = seq[a:a + m]
    if fate < 0.24:
        name = rng.choice([name + b"x", b"R" + name[1:], head + b" d"])  # renamed: absent
    elif fate < 0.52:
        pass
    elif fate < 0.82:
        s = rc(s)
    elif m:
        k = rng.randrange(m)
        s = s[:k] + bytes([_NEXT_BASE.get(s[k], 65)]) + s[k + 1:]
        if rng.random() < 0.5:
            s = rc(s)
    w = rng.choice([0, 0, 7, 60])
    return b">" + name + b"\n" + (s if not w else b"\n".join(s[k:k + w] for k in range(0, len(s), w))) + b"\n"


def random_case(rng):
    """A FASTQ shard and a FASTA made from it: a random slice of a random subset, some reverse-complemented, some renamed,
    some with one base changed."""
    fq, fa = [], []
    for i in range(rng.randint(8, 20)):
        name = b"r%d" % i
        head = name + (b" " + dna(rng, rng.randint(1, 8), "abc =") if rng.random() < 0.4 else b"")
        L = rng.choice([rng.randint(30, 90), rng.randint(30, 90), rng.randint(90, 400)])
        seq = dna(rng, L)
        fq.append(record(head, seq, rng=rng))
        entry = fasta_entry(rng, name, head, seq)
        if entry is not None:
            fa.append(entry)
    rng.shuffle(fa)
    opts = {"OnlyPositiveStrand": True} if rng.random() < 0.15 else {}
    return b"".join(fq), b"".join(fa), opts


@pytest.mark.parametrize("case", FIX, ids=[c["name"] for c in FIX])
def test_fixtures(case, tmp_path):
    assert run(tmp_path, case["fastq"].encode(), case["fasta"].encode(), case["opts"]) == case["want"].encode()


def test_random_cases_every_branch(tmp_path):
    rng = random.Random(SEED)
    count, total = {}, 0
    for k in range(N_RANDOM):
        fq, fa, opts = random_case(rng)
        for v in F.verdicts(fq, fa, opts):
            count[v[0]] = count.get(v[0], 0) + 1
            total += 1
        assert run(tmp_path, fq, fa, opts, parts=1 + k % 3) == F.fa2fq(fq, fa, opts), k
    for kind in ("plus", "minus", "absent", "nohit"):
        assert count.get(kind, 0) * 10 >= total, (kind, count, total)


def boundary_shard(rng, lengths, positions):
    fq, fa, k = [], [], 0
    for L in lengths:
        for npos in positions:
            m = L - npos + 1
            if m < 0 or (m == 0 and npos != L + 1):
                continue
            for where in ("first", "last", "minus_first", "minus_last", "none"):
                name = b"b%d" % k
                k += 1
                seq = dna(rng, L)
                a = 0 if where in ("first", "minus_first", "none") else L - m
                s = seq[a:a + m]
                if where.startswith("minus"):
                    s = rc(s)
                if where == "none" and m:
                    s = s[:-1] + (b"N")
                fq.append(record(name, seq, rng=rng))
                fa.append(b">" + name + b"\n" + s + b"\n")
    return b"".join(fq), b"".join(fa)


def test_both_search_shapes_and_their_boundary(tmp_path):
    """read lengths 0, 1, around 64 and around the number of start positions at which the search moves from a lane to a wave"""
    rng = random.Random(3)
    lengths = [0, 1, 2, 63, 64, 65, 66, 100, 127, 128, 129, 200, 1000]
    positions = [1, 2, 3, LANE_POS - 1, LANE_POS, LANE_POS + 1, LANE_POS + 2, 101, 128, 129, 201, 990, 1001]
    fq, fa = boundary_shard(rng, lengths, positions)
    kinds = {v[0] for v in F.verdicts(fq, fa, {})}
    assert kinds == {"plus", "minus", "nohit"}
    for opts in ({}, {"OnlyPositiveStrand": True}):
        assert run(tmp_path, fq, fa, opts) == F.fa2fq(fq, fa, opts)
    assert run(tmp_path, b"", fa) == b""


def test_reads_over_a_mebibyte(tmp_path):
    """the needle at the far end of a long read on each strand, and slices long enough for the block-wise writer"""
    rng = random.Random(5)
    L = (1 << 20) + 12345
    fq, fa = [], []
    for k, (a, m, minus) in enumerate([(L - 50, 50, False), (0, 50, True), (5, L - 12, False), (3, L - 7, True), (L - 50, 50, None)]):
        seq = dna(rng, L)
        s = seq[a:a + m]
        if minus:
            s = rc(s)
        if minus is None:
            s = s[:-1] + b"N"
        fq.append(record(b"big%d" % k, seq, rng=rng))
        fa.append(b">big%d\n" % k + s + b"\n")
    fq, fa = b"".join(fq), b"".join(fa)
    v = F.verdicts(fq, fa, {})
    assert [x[0] for x in v] == ["plus", "minus", "plus", "minus", "nohit"]
    assert run(tmp_path, fq, fa) == F.fa2fq(fq, fa)


def test_low_complexity_reads(tmp_path):
    fq = record(b"a1", b"A" * 300) + record(b"a2", b"A" * 300) + record(b"a3", b"AC" * 150) + record(b"a4", b"AC" * 150) + \
        record(b"a5", b"AC" * 150) + record(b"a6", b"A" * 40) + record(b"a7", b"A" * 40) + record(b"a8", b"A" * 299 + b"C")
    fa = b">a1\n" + b"A" * 20 + b"\n>a2\n" + b"T" * 20 + b"\n>a3\nCACACA\n>a4\nGTGTGT\n>a5\nTGTGTG\n>a6\n" + b"A" * 38 + \
        b"\n>a7\n" + b"T" * 39 + b"\n>a8\n" + b"A" * 30 + b"C\n"
    want = F.fa2fq(fq, fa)
    assert [v[0] for v in F.verdicts(fq, fa, {})] == ["plus", "minus", "plus", "minus", "minus", "plus", "minus", "plus"]
    assert run(tmp_path, fq, fa) == want


def test_multiline_crlf_no_final_newline_id_regexp(tmp_path):
    rng = random.Random(9)
    # (qualities without '@' and '+': a wrapped quality line that begins with one is ambiguous to any multi-line reader)
    recs = [(b"m%d some text" % i, dna(rng, rng.randint(40, 200))) for i in range(40)]
    quals = [bytes(65 + (7 * k + i) % 26 for k in range(len(s))) for i, (h, s) in enumerate(recs)]
    fa = b"".join(b">m%d\n" % i + (s[7:31] if i % 3 else rc(s[5:29])) + b"\n" for i, (h, s) in enumerate(recs) if i % 5)
    plain = b"".join(record(h, s, q) for (h, s), q in zip(recs, quals))
    wrap = lambda t: b"\n".join(t[k:k + 23] for k in range(0, len(t), 23))
    multi = b"".join(b"@" + h + b"\n" + wrap(s) + b"\n+\n" + wrap(q) + b"\n" for (h, s), q in zip(recs, quals))
    want = F.fa2fq(plain, fa)
    assert want.count(b"\n") == 4 * 32
    assert F.fa2fq(multi, fa) == want
    assert run(tmp_path, multi, fa) == want
    assert run(tmp_path, plain[:-1], fa) == want
    crlf = plain.replace(b"\n", b"\r\n")
    want_crlf = F.fa2fq(crlf, fa.replace(b"\n", b"\r\n"))
    assert want_crlf.count(b"\n") >= 4 * 16
    assert run(tmp_path, crlf, fa.replace(b"\n", b"\r\n")) == want_crlf
    # --id-regexp: the ID is what the expression captures
    fq = b"".join(record(b"x|m%d|y" % i, s) for i, (h, s) in enumerate(recs))
    o = {"IDRegexp": "\\|([^|]+)\\|"}
    want_re = F.fa2fq(fq, fa, o)
    assert want_re.count(b"\n") == 4 * 32 and F.fa2fq(fq, fa) == b""
    assert run(tmp_path, fq, fa, o) == want_re
    assert run(tmp_path, fq, fa) == b""


def test_alphabet_of_the_partition(tmp_path):
    """the minus strand is RevCom of the partition's alphabet: guessed DNA and given RNA complement, protein only reverses"""
    fq = record(b"p1", b"AACCGGGU") + record(b"p2", b"AACCGGGT")
    fa = b">p1\nACCCGG\n>p2\nACCCGG\n"
    for st in ("dna", "rna", "protein"):
        assert run(tmp_path, fq, fa, {"SeqType": st}) == F.fa2fq(fq, fa, {"SeqType": st}), st
    assert run(tmp_path, fq, b">p1\nGGGCCA\n", {"SeqType": "protein"}) == b"@p1\nGGGCCA\n+\n" + record(b"p1", b"AACCGGGU").split(b"\n")[3][::-1][1:7] + b"\n"
    path = tmp_path / "auto.fa"
    path.write_bytes(b">p2\nACCCGG\n")
    js = json.dumps({"Config": {"Quiet": True}, "FastaFile": str(path)})
    assert bsk.Fa2Fq(bsk.ReadFASTQN(record(b"p2", b"AACCGGGT"), 1), _Opts(js)) == F.fa2fq(record(b"p2", b"AACCGGGT"), b">p2\nACCCGG\n")


def test_fasta_shard_is_refused(tmp_path):
    with pytest.raises(BskError, match="this command only works for FASTQ format"):
        run(tmp_path, b">r1\nACGT\n", b">r1\nACGT\n", fasta_format=True)


def test_table_of_many_names(tmp_path):
    """120 000 names in 262 144 slots: most probes pass occupied slots and compare the bytes"""
    rng = random.Random(13)
    reads = {}
    for i in rng.sample(range(120000), 3000):
        reads[i] = dna(rng, 80)
    fa = b"".join(b">read%d\n" % i + (reads[i][10:60] if i in reads and i % 7 else b"ACGTACGTAC") + b"\n" for i in range(120000))
    fq = b"".join(record(b"read%d" % i, s) for i, s in sorted(reads.items())) + record(b"read120000", b"ACGTACGTAC") + record(b"rea", b"ACGTACGTAC")
    want = F.fa2fq(fq, fa)
    assert 2000 < want.count(b"\n") // 4 < 3000
    assert run(tmp_path, fq, fa) == want


def _host(ctx, out):
    host = C.create_string_buffer(max(1, out.len))
    check(lib.bsk_out_to_host(ctx, C.byref(out), host, out.len), ctx)
    return host.raw[:out.len]


def _whole(ctx, text):
    buf = C.create_string_buffer(text, len(text))
    out = Out()
    check(lib.bsk_fa2fq_run(ctx, buf, len(text), 0, bsk.FORMAT_FASTQ, 0, None, C.byref(out)), ctx)
    return _host(ctx, out)


def test_store_chunks_contexts_and_alternation(tmp_path, monkeypatch):
    monkeypatch.setenv("BSK_MIN_RANGE_BYTES", "4096")
    rng = random.Random(17)
    cases = [random_case(rng) for _ in range(40)]
    data = b"".join(b"".join(l.replace(b"@r", b"@c%d_r" % k) if l.startswith(b"@r") else l for l in c[0].splitlines(True)) for k, c in enumerate(cases))
    fa = b"".join(c[1].replace(b">r", b">c%d_r" % k).replace(b">Rr", b">Rc%d_" % k) for k, c in enumerate(cases))
    small = data[:data.index(b"@c3_")]
    assert len(data) > 60000 and len(small) < 20000
    want, want_small = F.fa2fq(data, fa), F.fa2fq(small, fa)
    assert want.count(b"\n") > 400
    pa = tmp_path / "a.fa"
    pa.write_bytes(fa)
    # a second table on the same device: the same names, every sequence reverse-complemented and shortened
    fb = b"".join(b">" + n + b"\n" + rc(s)[1:] + b"\n" for n, s in F.read_fasta_map(fa).items())
    pb = tmp_path / "b.fa"
    pb.write_bytes(fb)
    want_b = F.fa2fq(data, fb)
    assert want_b != want and want_b.count(b"\n") > 400
    with bsk.Operator("Fa2Fq", opts_json(pa, {}), 0) as op, bsk.Operator("Fa2Fq", opts_json(pb, {}), 0) as op_b:
        def to_store(stage, k):
            check(lib.bsk_ctx_set(op.ctx, b"stage_bytes", stage), op.ctx)
            path = tmp_path / ("s%d.fq" % k)
            st = C.c_void_p()
            assert lib.bsk_store_open(str(path).encode(), 1, C.byref(st)) == 0
            buf = C.create_string_buffer(data, len(data))
            nb, nr = C.c_uint64(), C.c_uint64()
            rc_ = lib.bsk_run_to_store(op.ctx, buf, len(data), bsk.FORMAT_FASTQ, 0, st, 0, C.byref(nb), C.byref(nr))
            assert lib.bsk_store_close(st, None) == 0
            check(rc_, op.ctx)
            assert path.read_bytes() == want, stage
            assert nr.value == want.count(b"\n") // 4

        assert _whole(op.ctx, data) == want
        assert _whole(op_b.ctx, data) == want_b   # two contexts, two tables, one device
        to_store(b"8000", 0)                      # several chunks equal the one call
        assert _whole(op.ctx, small) == want_small
        assert _whole(op_b.ctx, small) == F.fa2fq(small, fb)
        to_store(b"4000", 1)
        assert _whole(op.ctx, data) == want
        to_store(b"20000", 2)
        assert _whole(op_b.ctx, data) == want_b
        # out = slices: still one block
        check(lib.bsk_ctx_set(op.ctx, b"out", b"slices"), op.ctx)
        assert _whole(op.ctx, data) == want


def cli(args, env_extra=None, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    p = subprocess.run([CLI] + args, capture_output=True, cwd=ROOT, env=env, timeout=timeout)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    return p.stdout


def test_cli_file_devices_and_pipe(tmp_path):
    rng = random.Random(23)
    cases = [random_case(rng) for _ in range(150)]
    data = b"".join(b"".join(l.replace(b"@r", b"@c%d_r" % k) if l.startswith(b"@r") else l for l in c[0].splitlines(True)) for k, c in enumerate(cases))
    fa = b"".join(c[1].replace(b">r", b">c%d_r" % k) for k, c in enumerate(cases))
    src, fas = str(tmp_path / "in.fq"), str(tmp_path / "t.fa")
    open(src, "wb").write(data)
    open(fas, "wb").write(fa)
    for extra, o in (([], {}), (["-P"], {"OnlyPositiveStrand": True})):
        want = F.fa2fq(data, fa, o)
        assert want.count(b"\n") > 1000
        args = ["fa2fq", "-t", "dna", "-f", fas] + extra + [src]
        out = str(tmp_path / ("one" + "".join(extra)))
        cli(args + ["-o", out, "--merge"])
        assert open(out, "rb").read() == want
        assert cli(args + ["-o", "-"]) == want
        out = str(tmp_path / ("dev" + "".join(extra)))
        cli(args + ["--devices", "0", "-o", out, "--merge"],
            {"BSK_HOST_PIPELINE_FROM": "0", "BSK_STAGE_BYTES": "4096", "BSK_STREAM_PIECE_BYTES": "30000"})
        assert open(out, "rb").read() == want
        out = str(tmp_path / ("two" + "".join(extra)))
        cli(args + ["--devices", "0,0", "-o", out, "--merge"])   # every worker loads the same table
        assert open(out, "rb").read() == want
    # inside pipe: the reads that fa2fq gives back, reversed by seq
    want = F.fa2fq(data, fa)
    job = {"pipe": [{"cmd": ["fa2fq", "-t", "dna", "-f", fas, src]}], "cmd": ["seq", "-n", "-i"]}
    jf = tmp_path / "job.json"
    jf.write_text(json.dumps(job))
    names = b"".join(l[1:] + b"\n" for l in want.split(b"\n")[0::4] if l)
    assert cli(["pipe", "--job", str(jf), "-o", "-"]) == names
