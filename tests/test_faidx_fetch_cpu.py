"""`faidx -d` without a GPU (PARITY.md FAIX): the planner against the restatement in fai_fetch_ref, offsets beyond 2^32 with
no file behind them, the 4 KiB span rule, the batch cuts, every refusal of a row by its text, the one-lane source of the
kernel (bsk_faidx_fetch_host) against oracle.faidx_query on every shape the device test runs, the two checks, the header
alone under the host's sanitizers, and what the command line refuses before a device is touched."""
import json
import os
import random
import re
import subprocess

import pytest

import fai_fetch_ref as R
import oracle
import seqgen
import bigseqkit_amd as bsk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")
NO_DEVICE = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}
FORMAT, CAPACITY, OPTS = 3, 7, 2
T = 4096


class Opts:
    def __init__(self, d):
        self.d = dict(d)

    def to_json(self):
        return json.dumps(self.d)


def put(tmp_path, name, data):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def plan_of(fai, o, size, budget=0):
    with bsk.FaidxFetchPlan(fai, Opts(o), size, device=-1, budget=budget) as p:
        return p.hits, p.batches, p.T, p.fastq


def ref_plan(fai, o, size, budget=1 << 30):
    rows, fastq = R.parse_rows(fai, size, bool(o.get("FullHead")))
    cfg = o.get("Config", {})
    hs = R.hits(rows, o["Regions"], size, bool(o.get("IgnoreCase")), bool(o.get("FullHead")), cfg.get("LineWidth", 60), bool(o.get("UseRegexp")))
    alpha = 0 if cfg.get("SeqType", "auto") != "auto" else min(size, 2 * 10000 + 65536)
    return rows, hs, R.batches(hs, size, budget, alpha), fastq


def same_hits(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w, (g, w)


def test_tile_size():
    assert plan_of(b"a\t1\t3\t1\t2\n", {"Regions": ["a"]}, 5)[2] == T


@pytest.mark.parametrize("seed", range(4))
def test_planner_is_the_restatement_on_random_indices(seed):
    rng = random.Random(seed)
    fastq = seed == 3
    data = seqgen.random_fastq(rng, 150, 0, 150) if fastq else seqgen.random_fasta(rng, 150, 0, 900, width=(60, 7, 0)[seed % 3],
                                                                                    final_newline=seed != 1)
    fai = oracle.faidx(data, fastq)
    ids = [("r%d" if fastq else "s%d") % k for k in range(150)]
    qs = []
    for _ in range(80):
        i = rng.choice(ids)
        b, e = rng.randint(-60, 400) or 1, rng.randint(-60, 400) or -1
        qs.append(rng.choice([i, "%s:%d-%d" % (i, b, e), "%s:%d" % (i, abs(b)), "%s:%d-" % (i, b), "%s:-%d" % (i, abs(e)), i.upper()]))
    for extra in ({}, {"IgnoreCase": True}, {"Config": {"LineWidth": 7, "SeqType": "dna"}}):
        o = dict({"Regions": qs}, **extra)
        for budget in (1 << 30, 40000 + 2 * 10000 + 65536):
            rows, hs, bs, fq = ref_plan(fai, o, len(data), budget)
            got_h, got_b, _, got_fq = plan_of(fai, o, len(data), budget)
            same_hits(got_h, hs)
            assert got_b == bs and got_fq == fq == fastq
            assert len(hs) > 20 and (budget == 1 << 30 or len(bs) > 1)
    o = {"Regions": ["^s1\\d$", "7$"], "UseRegexp": True}
    if not fastq:
        same_hits(plan_of(fai, o, len(data))[0], ref_plan(fai, o, len(data))[1])


def test_offsets_beyond_32_bits_without_a_file():
    """a synthetic index and file size: all the arithmetic is 64-bit"""
    offs = [(1 << 32) - 1, 1 << 32, (1 << 40) + 3]
    fai = b"".join(b"c%d\t1000\t%d\t60\t61\n" % (k, o) for k, o in enumerate(offs))
    size = (1 << 40) + 5000
    o = {"Regions": ["c0:1-130", "c1:1-60", "c2:990-1000", "c2:5-6"], "Config": {"SeqType": "dna"}}
    hs, bs, _, _ = plan_of(fai, o, size)
    rows, want, wb, _ = ref_plan(fai, o, size)
    same_hits(hs, want)
    assert bs == wb
    assert [h["lines"] for h in hs] == [(offs[0], offs[0] + 3 * 61), (offs[1], offs[1] + 61), (offs[2] + 16 * 61, offs[2] + 16 * 61 + 41)]
    assert [h["probe"] for h in hs] == [o + 16 * 61 + 40 for o in offs]
    # c0 and c1 lie one byte apart: their pages merge; c2 is far away
    assert bs[0]["spans"] == [((1 << 32) - 4096, (1 << 32) + 4096), (1 << 40, (1 << 40) + 4096)]


def test_spans_merge_at_4k_edges():
    # one row per case, lines of 63 bases + newline = 64 bytes: line k of a record at offset 0 begins at 64 k
    fai = b"a\t1000000\t0\t63\t64\n"
    size = 64 * 15874
    def spans(regions, seqtype="dna"):
        return plan_of(fai, {"Regions": regions, "Config": {"SeqType": seqtype}}, size)[1][0]["spans"]
    tail = (size // 4096 * 4096, size)  # the end probe's page
    assert spans(["a:1-63"]) == [(0, 4096), tail]                      # a span ending inside a page
    assert spans(["a:4033-4095"]) == [(4096, 8192), tail]              # line 64 = bytes [4096, 4160): begins on the edge
    assert spans(["a:3970-4032"]) == [(0, 4096), tail]                 # line 63 = bytes [4032, 4096): ends on the edge, touches nothing
    assert spans(["a:3970-4033"]) == [(0, 8192), tail]                 # one base over the edge
    two = b"a\t630\t0\t63\t64\nb\t630\t8192\t63\t64\nc\t630\t12289\t63\t64\nd\t63\t40000\t63\t64\n"
    hs, bs, _, _ = plan_of(two, {"Regions": ["a:1-1", "b:1-1", "c:1-1", "d"], "Config": {"SeqType": "dna"}}, 50000)
    # a: lines in page 0, probe in page 0; b: page 2 (touches nothing of a: page 1 is not read); c: page 3, touching b's
    assert bs[0]["spans"] == [(0, 4096), (8192, 16384), (36864, 40960)]
    assert bs[0]["spans"] == R.merge([h["lines"] for h in hs] + [R.probe_span(h, 50000) for h in hs], 50000)
    # the alphabet of a minus-strand region is guessed from the head of the file: one more span, merged like the others
    assert plan_of(two, {"Regions": ["d:5-2"]}, 50000)[1][0]["spans"] == [(0, 50000)]
    assert plan_of(two, {"Regions": ["d:2-5"]}, 50000)[1][0]["spans"] == [(36864, 40960)]


def test_batch_cuts_and_the_budget():
    fai = b"".join(b"r%d\t5000\t%d\t50\t51\n" % (k, 10 + 6000 * k) for k in range(40))
    size = 6000 * 40 + 100
    o = {"Regions": ["r%d:%d-%d" % (k, 1 + k, 3000 + k) for k in range(40)], "Config": {"SeqType": "dna", "LineWidth": 0}}
    rows, hs, wb, _ = ref_plan(fai, o, size, 30000)
    got = plan_of(fai, o, size, 30000)[1]
    assert got == wb and len(got) > 5
    assert [b["hits"][0] for b in got[1:]] == [b["hits"][1] for b in got[:-1]] and got[0]["hits"][0] == 0 and got[-1]["hits"][1] == 40
    for b in got:
        assert b["out_bytes"] == sum(h["out_len"] for h in hs[b["hits"][0]:b["hits"][1]])
        assert b["read_bytes"] + b["out_bytes"] <= 30000 or b["hits"][1] - b["hits"][0] == 1
    with pytest.raises(bsk.BskError) as e:
        plan_of(fai, o, size, 5000)
    assert e.value.code == CAPACITY and re.search(r"index row 1 \(r0\) reads and writes \d+ bytes, the budget of a batch is 5000", str(e.value))


ROW_REFUSALS = [
    (b"a\tx\t3\t4\t5\n", {}, "index row 1 (a): column length is not a number: x"),
    (b"ok\t4\t4\t4\t5\na\t4\t-3\t4\t5\n", {}, "index row 2 (a): column offset is not a number: -3"),
    (b"a\t4\t3\t4\n", {}, "index row 1: fewer than 5 tab-separated columns"),
    (b"a\t4294967296\t3\t60\t61\n", {}, "index row 1 (a): length 4294967296 is 2^32 or more"),
    (b"a\t8\t3\t4\t6\n", {}, "index row 1 (a): linewidth 6 - linebases 4 is not 1"),
    (b"a\t8\t3\t4\t4\n", {}, "index row 1 (a): linewidth 4 - linebases 4 is not 1"),
    (b"a\t8\t3\t0\t1\n", {}, "index row 1 (a): linebases 0 with length 8"),
    (b"a\t8\t300\t4\t5\n", {}, "index row 1 (a): offset 300 or the predicted end of the sequence lies beyond the file (100 bytes)"),
    (b"a\t8\t92\t4\t5\n", {}, "index row 1 (a): offset 92 or the predicted end of the sequence lies beyond the file (100 bytes)"),
    (b"a b\t8\t3\t4\t5\n", {}, "index row 1 (a b): the name holds a blank or tab"),
    (b"a\tb\t8\t3\t4\t5\n", {}, "index row 1 (a\tb): the name holds a blank or tab"),
]


@pytest.mark.parametrize("k", range(len(ROW_REFUSALS)))
def test_row_refusals(k):
    fai, extra, text = ROW_REFUSALS[k]
    with pytest.raises(bsk.BskError) as e:
        plan_of(fai, dict({"Regions": ["a"]}, **extra), 100)
    assert e.value.code == FORMAT and text in str(e.value), str(e.value)
    with pytest.raises(R.Refused):
        R.parse_rows(fai, 100)


def test_rows_that_are_accepted():
    # a -f name holds blanks and tabs (split from the right); an empty record is 0 0; the end of the file is a legal end
    hs = plan_of(b"a b\tc\t8\t3\t4\t5\nz\t0\t13\t0\t0\n", {"Regions": ["a", "z"], "FullHead": True}, 13)[0]
    assert [(h["row"], h["header"]) for h in hs] == [(0, b">a\n")]       # a zero-length row is never a hit
    assert plan_of(b"a\t8\t3\t4\t5\n", {"Regions": ["a"]}, 12)[0][0]["lines"] == (3, 12)
    with pytest.raises(bsk.BskError) as e:
        plan_of(b"a\t8\t3\t4\t5\n", {"Regions": ["a"], "Config": {"IDNCBI": True}}, 13)
    assert e.value.code == OPTS and "--id-regexp / --id-ncbi" in str(e.value)


CASES = R.cases(T)


@pytest.fixture(scope="module")
def wants():
    return [oracle.faidx_query(text, fastq, json.dumps(o)) for _, text, fastq, o in CASES]


@pytest.mark.parametrize("k", range(len(CASES)))
def test_host_lane_is_the_oracle(k, tmp_path, wants):
    name, text, fastq, o = CASES[k]
    fai = oracle.faidx(text, fastq, json.dumps({"FullHead": bool(o.get("FullHead"))}))
    path = put(tmp_path, "x.fa", text)
    assert bsk.FaidxFetch(path, fai, Opts(o), device=-1, host=True) == wants[k], name
    if k == 0:
        assert wants[k].count(b">") == 6  # (the empty record and the one without a sequence line are no hits)


def test_small_batches_give_the_same_bytes(tmp_path):
    name, text, fastq, o = CASES[1]
    fai = oracle.faidx(text, fastq)
    path = put(tmp_path, "x.fa", text)
    info = {}
    want = oracle.faidx_query(text, fastq, json.dumps(o))
    assert bsk.FaidxFetch(path, fai, Opts(o), device=-1, host=True, budget=2 * 85536 + 90000, info=info) == want
    assert info["hits"] == 6 and info["T"] == T and info["bytes_written"] == len(want)


def refused(path, fai, o, **kw):
    with pytest.raises(bsk.BskError) as e:
        bsk.FaidxFetch(path, fai, Opts(o), device=-1, host=True, **kw)
    assert e.value.code == FORMAT and R.MSG in str(e.value), str(e.value)
    return str(e.value)


def test_the_index_must_fit_the_file(tmp_path):
    # lines of two widths: the rows accept the record, arithmetic cannot address it behind its first short line
    path = put(tmp_path, "two.fa", R.TWO_WIDTHS)
    fai = oracle.faidx(R.TWO_WIDTHS, False)
    assert fai == b"a\t18\t3\t6\t7\n"
    assert "index row 1 (a), file offset 23" in refused(path, fai, {"Regions": ["a:16-18"]})   # the end probe: 'G', not '\n'
    assert "index row 1 (a)" in refused(path, fai, {"Regions": ["a:1-2"]})                       # ... which every hit of the record meets
    rows, fastq = R.parse_rows(fai, len(R.TWO_WIDTHS))
    with pytest.raises(R.Refused):
        R.fetch(R.TWO_WIDTHS, rows, R.hits(rows, ["a:16-18"], len(R.TWO_WIDTHS)))
    # an index whose offsets are shifted by one byte, and one built for another file
    rng = random.Random(5)
    text = seqgen.random_fasta(rng, 30, 50, 400, width=60)
    other = seqgen.random_fasta(rng, 30, 50, 400, width=60)
    path = put(tmp_path, "x.fa", text)
    fai = oracle.faidx(text, False)
    shifted = b"".join(b"\t".join([f[0], f[1], b"%d" % (int(f[2]) + 1)] + f[3:]) + b"\n" for f in (l.split(b"\t") for l in fai.splitlines()))
    for q in (["s3:2-9"], ["s7"], ["s20:70-61"]):
        o = {"Regions": q, "Config": {"SeqType": "dna"}}
        m = refused(path, shifted, o)
        assert "index row %d (%s), file offset" % (int(q[0].split(":")[0][1:]) + 1, q[0].split(":")[0]) in m
    wrong = oracle.faidx(other, False)
    n_ref = 0
    for k in range(30):
        o = {"Regions": ["s%d" % k], "Config": {"SeqType": "dna"}}
        try:
            got = bsk.FaidxFetch(path, wrong, Opts(o), device=-1, host=True)
        except bsk.BskError as e:
            assert R.MSG in str(e) or "beyond the file" in str(e)
            n_ref += 1
        else:  # (rows that agree by chance describe the file there: the bytes are then the oracle's)
            assert got == oracle.faidx_query(text, False, json.dumps(o))
    assert n_ref >= 25
    # a newline inside a line that the index calls bases, far from the region's own bases (check 1 judges the whole line)
    bad = bytearray(text)
    row = fai.splitlines()[4].split(b"\t")
    assert int(row[1]) > 60
    bad[int(row[2]) + 50] = 10
    path2 = put(tmp_path, "bad.fa", bytes(bad))
    assert "index row 5 (s4), file offset %d" % (int(row[2]) + 50) in refused(path2, fai, {"Regions": ["s4:2-3"]})


def test_bytes_outside_the_plan_do_not_matter(tmp_path):
    rng = random.Random(9)
    text = seqgen.random_fasta(rng, 400, 100, 3000, width=60)
    fai = oracle.faidx(text, False)
    o = {"Regions": ["s3:5-900", "s200:100-7", "s399", "s120:61-61"]}
    hs, bs, _, _ = plan_of(fai, o, len(text))
    junk = R.junk_outside(text, bs[0]["spans"])
    assert junk != text and sum(hi - lo for lo, hi in bs[0]["spans"]) < len(text) // 3
    want = oracle.faidx_query(text, False, json.dumps(o))
    for name, data in (("x.fa", text), ("junk.fa", junk)):
        assert bsk.FaidxFetch(put(tmp_path, name, data), fai, Opts(o), device=-1, host=True) == want


def test_conditions_on_an_8_mib_file():
    """five 100-base regions in different records of an 8 MiB file: bytes read <= sum(line-extended span + 2 * 4096) +
    2 * 4096 per end probe -- for the restatement and for the planner"""
    nrec, L = 64, 129024  # 64 records of 2 100 lines of 60 + a header: 8.2 MiB
    rec = 8 + L + L // 60
    fai = b"".join(b"chr%03d\t%d\t%d\t60\t61\n" % (k, L, 8 + rec * k) for k in range(nrec))
    size = rec * nrec
    assert size >= 8 << 20
    o = {"Regions": ["chr%03d:%d-%d" % (k, b, b + 99) for k, b in ((2, 1), (17, 4090), (30, 61), (45, 100000), (63, L - 99))]}
    rows, hs, bs, _ = ref_plan(fai, o, size)
    assert len(hs) == 5 and all(h["p1"] - h["p0"] == 100 for h in hs)
    assert bs[0]["read_bytes"] <= R.read_bound(hs)
    got_h, got_b, _, _ = plan_of(fai, o, size)
    assert got_b == bs and got_b[0]["read_bytes"] <= R.read_bound(hs) < size // 50


def test_source_under_sanitizers(tmp_path):
    """tests/host_c/fai_fetch_check.cpp -- fai_fetch.hpp and nothing of the library -- built with the host's address and
    undefined-behaviour sanitizers: the oracle's bytes on the shapes with a plain alphabet, whole and in small batches, from
    buffers of exactly the planned size; the refusals; and no report"""
    exe = str(tmp_path / "fai_fetch_check")
    src = os.path.join(ROOT, "tests", "host_c", "fai_fetch_check.cpp")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("the sanitizer runtime cannot be linked here")
    assert r.returncode == 0, r.stderr[-2000:]

    def run(text, fai, o, budget):
        qs, seen = [], set()
        for q in o["Regions"]:
            i, b, e = R.parse_region(q)
            if i in seen:
                continue
            seen.add(i)
            whole = (b == 1 and e == -1) or (b > 0 and e < 0)
            minus = (not whole) and b > e
            qs += [i, str(e if minus else b), str(b if minus else e), str(int(minus)), "-" if whole else ":%d-%d" % (b, e)]
        p = subprocess.run([exe, put(tmp_path, "x.fa", text), put(tmp_path, "x.fai", fai), str(o.get("Config", {}).get("LineWidth", 60)),
                            str(budget), str(tmp_path / "out")] + qs, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and not p.stderr, (p.stdout[-500:], p.stderr[-2000:])
        return p.stdout.strip().split(" ", 2), open(str(tmp_path / "out"), "rb").read()

    ran = 0
    for name, text, fastq, o in CASES:
        plain = o.get("Config", {}).get("SeqType") == "dna" or not any(R.parse_region(q)[1] > R.parse_region(q)[2] > 0 for q in o["Regions"])
        if o.get("UseRegexp") or o.get("IgnoreCase") or o.get("FullHead") or not plain or name.startswith(("minus", "QUERIES")):
            continue
        want = oracle.faidx_query(text, fastq, json.dumps(o))
        fai = oracle.faidx(text, fastq)
        for budget in (1 << 30, 200000):
            head, got = run(text, fai, o, budget)
            assert head[0] == "ok" and got == want, (name, budget, head)
        ran += 1
    assert ran >= 15
    head, _ = run(R.TWO_WIDTHS, b"a\t18\t3\t6\t7\n", {"Regions": ["a:16-18"]}, 1 << 30)
    assert head[:2] == ["refused", str(FORMAT)] and R.MSG in head[2]
    head, _ = run(b">a\nACGT\n", b"a\t4\t3\t4\t6\n", {"Regions": ["a"]}, 1 << 30)
    assert head[:2] == ["refused", str(FORMAT)] and "linewidth 6 - linebases 4 is not 1" in head[2]


def test_command_line_refusals_before_a_device(tmp_path):
    import gzip
    fa = put(tmp_path, "x.fa", b">a\nACGT\n")
    idx = put(tmp_path, "x.fai", b"a\t4\t3\t4\t5\n")
    gz = put(tmp_path, "z.fa.gz", gzip.compress(b">a\nACGT\n", mtime=0))
    job = put(tmp_path, "job.json", json.dumps({"cmd": ["faidx", "-d", idx, fa, "a:1-2"]}).encode())
    plain_job = put(tmp_path, "job2.json", json.dumps({"cmd": ["faidx", "-d", idx, fa]}).encode())

    def run(args, env=()):
        r = subprocess.run([CLI, *args], capture_output=True, timeout=120, env=dict(os.environ, **NO_DEVICE, **dict(env)))
        return r.returncode, r.stdout, r.stderr.decode()

    code, out, err = run(["faidx", fa, "a:1-2", "-d", idx, "--devices", "0,1"])
    assert (code, out) == (1, b"") and "-d (--index-file) with --devices is refused" in err
    code, out, err = run(["pipe", "--job", job, "-o", "-"])
    assert (code, out) == (1, b"") and "-d (--index-file) inside a 'pipe' job is refused" in err
    code, out, err = run(["pipe", "--job", plain_job, "-o", "-"])  # (without regions -d is without effect, in a job too)
    assert code == 1 and "is refused" not in err and "no HIP device visible" in err
    code, out, err = run(["faidx", gz, "a:1-2", "-d", idx], {"BSK_GZIP": "1"})
    assert (code, out) == (1, b"") and "gzip but not BGZF" in err and "bgzip" in err and "faidx -d" in err
    for flag in (["--id-ncbi"], ["--id-regexp", "^(\\S+)"]):
        code, out, err = run(["faidx", fa, "a:1-2", "-d", idx] + flag)
        assert (code, out) == (1, b"") and "--id-regexp / --id-ncbi is refused" in err
    # an absent index with another ID rule is today's run, which needs a device next; so is a run without regions
    code, out, err = run(["faidx", fa, "a:1-2", "-d", str(tmp_path / "absent.fai"), "--id-ncbi"])
    assert code == 1 and "no HIP device visible" in err
    code, out, err = run(["faidx", fa, "-d", idx, "--devices", "0"])
    assert "is refused" not in err


def test_records_of_two_widths_are_exact_or_refused(tmp_path):
    """the argument of PARITY FAIX over every region of every small record that the rows accept: `a` lines of W bases and
    `b` lines of w < W -- a hit through the index gives the bases of the whole-file path or is refused, never other bases"""
    served = refusals = 0
    for W, w, a, b in ((6, 5, 2, 2), (6, 3, 2, 2), (5, 2, 1, 4), (3, 1, 0, 3), (6, 5, 0, 2), (4, 2, 2, 3), (6, 5, 1, 1)):
        n = a * W + b * w
        seq = bytes(b"ACGT"[k * 7 % 4] for k in range(n))
        lines = [seq[k * W:(k + 1) * W] for k in range(a)] + [seq[a * W + k * w:a * W + (k + 1) * w] for k in range(b)]
        text = b">x\nAC\n>a\n" + b"".join(l + b"\n" for l in lines) + b">z\nGG\n"
        fai = oracle.faidx(text, False)
        lb = W if a else w  # (linebases is the first line's)
        assert fai.splitlines()[1] == b"a\t%d\t9\t%d\t%d" % (n, lb, lb + 1)
        path = put(tmp_path, "x.fa", text)
        before = refusals
        for s in range(1, n + 1):
            for e in range(s, n + 1):
                o = {"Regions": ["a:%d-%d" % (s, e)], "Config": {"LineWidth": 0}}
                try:
                    got = bsk.FaidxFetch(path, fai, Opts(o), device=-1, host=True)
                except bsk.BskError as err:
                    assert err.code == FORMAT and R.MSG in str(err)
                    refusals += 1
                else:
                    assert got == b">a:%d-%d\n" % (s, e) + seq[s - 1:e] + b"\n", (W, w, a, b, s, e)
                    served += 1
        # a record of one width (and a last line) is served everywhere; one of two widths is refused from its first short line on
        assert (refusals == before) == (a == 0 or b == 1), (W, w, a, b)
    assert served and refusals


# ---------------------------------------------------------------- BGZF: the block table and the fetch through it (host lane)
import bgzf_ref as Z  # noqa: E402


bgzf_files = R.bgzf_files


def test_gzi_build_is_the_reference_index(tmp_path):
    files, _ = bgzf_files()
    for name, (text, data) in files.items():
        image, n_text = bsk.BgzfGzi(put(tmp_path, name + ".gz", data))
        assert image == R.gzi_write(Z.index(data)) and n_text == len(text), name
        assert R.gzi_read(image)[-1][0] == Z.index(data)[-1][0]
    with pytest.raises(bsk.BskError) as e:
        bsk.BgzfGzi(put(tmp_path, "cut.gz", files["b100"][1][:-40] + b"\0" * 7))
    assert e.value.code == FORMAT and "is no whole BGZF block" in str(e.value)


BGZF_QUERIES = R.BGZF_QUERIES


@pytest.mark.parametrize("name", sorted(BGZF_QUERIES))
def test_bgzf_host_lane_is_the_oracle(name, tmp_path):
    """a region inside one block, across block edges, starting on a block's first byte; the table from us and from the Python writer"""
    files, _ = bgzf_files()
    text, data = files[name]
    path = put(tmp_path, name + ".fa.gz", data)
    fai = oracle.faidx(text, False)
    ours, theirs = bsk.BgzfGzi(path)[0], R.gzi_write(Z.index(data))
    table = R.gzi_read(theirs)
    qs = list(BGZF_QUERIES[name])
    if name == "b100":  # a region whose first line begins on the first byte of a block
        rows, _ = R.parse_rows(fai, len(text))
        k = next(k for k, r in enumerate(rows) if k not in (0, 3, 7, 20, 39) and r[1] > 0 and any(u == r[2] // 4096 * 4096 for c, u in table))
        qs.append("s%d:1-5" % k)
    o = {"Regions": qs, "Config": {"SeqType": "dna"}}
    want = oracle.faidx_query(text, False, json.dumps(o))
    assert want.count(b">") == len(qs)
    for gzi in (ours, theirs):
        info = {}
        assert bsk.FaidxFetch(path, fai, Opts(o), device=-1, host=True, gzi=gzi, info=info) == want
        hs = R.hits(R.parse_rows(fai, len(text))[0], qs, len(text))
        assert 0 < info["blocks_inflated"] <= R.blocks_bound(table, hs, len(text))


def test_bgzf_wrong_table_entries(tmp_path):
    """one wrong entry: refused on a touched block with the entry named, accepted on an untouched one"""
    import struct
    files, _ = bgzf_files()
    text, data = files["b100"]
    path = put(tmp_path, "x.fa.gz", data)
    fai = oracle.faidx(text, False)
    good = R.gzi_write(Z.index(data))
    table = R.gzi_read(good)
    o = {"Regions": ["s0:1-5"], "Config": {"SeqType": "dna"}}   # reads text [0, 4096) and the page of its probe: the first blocks
    want = oracle.faidx_query(text, False, json.dumps(o))
    far = len(table) - 3                                         # a block of the last pages: not touched
    assert table[far][1] > 3 * 4096

    def with_entry(k, c, u):
        t = list(table)
        t[k] = (c, u)
        return struct.pack("<Q", len(t) - 1) + b"".join(struct.pack("<QQ", a, b) for a, b in t[1:])

    assert bsk.FaidxFetch(path, fai, Opts(o), device=-1, host=True, gzi=with_entry(far, table[far][0] + 1, table[far][1])) == want
    # entry 3 wrong in either column: the block of entry 2 contradicts it
    for c, u in ((table[3][0] + 1, table[3][1]), (table[3][0], table[3][1] + 1)):
        with pytest.raises(bsk.BskError) as e:
            bsk.FaidxFetch(path, fai, Opts(o), device=-1, host=True, gzi=with_entry(3, c, u))
        assert e.value.code == FORMAT and "block table entry 2 (compressed offset %d, text offset %d)" % table[2] in str(e.value), str(e.value)
        assert "contradicts the next entry; build the table again" in str(e.value)
    # the first block of a span that begins further in: its entry does not land on a block header
    rows, _ = R.parse_rows(fai, len(text))
    o2 = {"Regions": ["s30:1-5"], "Config": {"SeqType": "dna"}}
    h = R.hits(rows, o2["Regions"], len(text))[0]
    first, _ = R.gzi_blocks(table, *R.round_out(h["lines"][0], h["lines"][1], len(text)))
    assert first > 3
    with pytest.raises(bsk.BskError) as e:
        bsk.FaidxFetch(path, fai, Opts(o2), device=-1, host=True, gzi=with_entry(first, table[first][0] + 1, table[first][1]))
    assert e.value.code == FORMAT and "block table entry %d (compressed offset %d" % (first, table[first][0] + 1) in str(e.value)
    assert "does not land on a block header of this file; build the table again" in str(e.value)
    with pytest.raises(bsk.BskError) as e:
        bsk.FaidxFetch(path, fai, Opts(o), device=-1, host=True, gzi=good[:-3])
    assert "is not a .gzi file" in str(e.value)
    # a damaged block that is touched is the BGZF reader's refusal (the CRC), one that is not touched is not read
    bad = bytearray(data)
    bad[table[1][0] + 20] ^= 0x55
    with pytest.raises(bsk.BskError):
        bsk.FaidxFetch(put(tmp_path, "bad.fa.gz", bytes(bad)), fai, Opts(o), device=-1, host=True, gzi=good)
    bad = bytearray(data)
    bad[table[far][0] + 20] ^= 0x55
    assert bsk.FaidxFetch(put(tmp_path, "bad2.fa.gz", bytes(bad)), fai, Opts(o), device=-1, host=True, gzi=good) == want
