"""Parity of `replace` (bigseqkit-lib/replace.go) on the GPU against tests/replace_ref.py and the fixtures."""
import json
import os
import random
import subprocess

import pytest

import bigseqkit_amd as bsk
from bigseqkit_amd._lib import BskError
import replace_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "replace_fixtures.json")))


class _Opts:
    def __init__(self, d):
        self._v = dict(d)

    def to_json(self):
        return json.dumps(self._v)


def run(data, fastq, opts, width=60, parts=1):
    d = dict(opts)
    d["Config"] = dict(d.get("Config", {}), LineWidth=width, Quiet=True)
    read = (bsk.ReadFASTQN if fastq else bsk.ReadFASTAN)
    return bsk.Replace(read(data, parts), _Opts(d))


def want(data, fastq, opts, width=60, kv=b""):
    return R.replace_records(data, fastq, opts, R.read_kvs(kv, opts.get("IgnoreCase", False)), width)


def make(rng, nrec, fastq, wrap=60, crlf=False, final_newline=True):
    out = []
    for i in range(nrec):
        name = "%s%d" % (rng.choice(["id", "ID", "seq_", "gi|"]), rng.randint(0, 30))
        if rng.random() < 0.5:
            name += " " + "".join(rng.choice("abc xy_=1") for _ in range(rng.randint(0, 14)))
        L = rng.choice([0, 1, 5, rng.randint(0, 300)])
        seq = "".join(rng.choice("ACGTNacgt-") for _ in range(L))
        if fastq:
            rec = "@%s\n%s\n+\n%s\n" % (name, seq, "I" * L)
        else:
            w = wrap if wrap else max(1, L)
            if wrap == -1:  # irregular wrapping
                lines, k = [], 0
                while k < L:
                    step = rng.randint(1, 40)
                    lines.append(seq[k:k + step])
                    k += step
            else:
                lines = [seq[k:k + w] for k in range(0, L, w)]
            rec = ">%s\n%s" % (name, "".join(x + "\n" for x in lines) if lines else "")
        out.append(rec)
    text = "".join(out)
    if crlf:
        text = text.replace("\n", "\r\n")
    if not final_newline and text.endswith("\n"):
        text = text[:-1]  # (one byte: an empty last quality line stays a line)
    return text.encode()


NAME_OPTS = [
    {"Pattern": "\\s.+"},
    {"Pattern": "^(\\S+)", "Replacement": "read_${1}_{nr}", "NrWidth": 5},
    {"Pattern": "^", "Replacement": "pre_"},
    {"Pattern": "x*", "Replacement": "-"},
    {"Pattern": "(?P<k>[a-z]+)(\\d+)", "Replacement": "$2.${k}.$$"},
    {"Pattern": "ID", "Replacement": "id", "IgnoreCase": True},
    {"Pattern": "(a)|(b)|(c)", "Replacement": "<$3$2$1>"},
    {"Pattern": "nomatch", "Replacement": "z"},
    {"Pattern": "\\b", "Replacement": "|"},
    {"Pattern": "y+?", "Replacement": "{NR}{Nr}"},
]
SEQ_OPTS = [
    {"Pattern": "N", "Replacement": "n", "BySeq": True},
    {"Pattern": "[^ACGT]", "Replacement": "", "BySeq": True},
    {"Pattern": "(.)", "Replacement": "$1 ", "BySeq": True},
    {"Pattern": "a", "Replacement": "[$0]", "BySeq": True, "IgnoreCase": True},
    {"Pattern": "-", "Replacement": "", "BySeq": True},
    {"Pattern": "AC+", "Replacement": "<$0>", "BySeq": True},
    {"Pattern": "G*", "Replacement": "_", "BySeq": True},
    {"Pattern": "^A|T$", "Replacement": "x", "BySeq": True},
]


@pytest.mark.parametrize("oi", range(len(NAME_OPTS)))
def test_names_parity(oi):
    rng = random.Random(oi)
    opts = NAME_OPTS[oi]
    for fastq in (False, True):
        for wrap, width, crlf, fin in [(60, 60, False, True), (0, 7, True, False), (-1, 0, False, True), (13, 60, False, False)]:
            data = make(rng, rng.randint(1, 300), fastq, wrap if not fastq else 0, crlf, fin)
            assert run(data, fastq, opts, width) == want(data, fastq, opts, width), (opts, fastq, wrap, width)


@pytest.mark.parametrize("oi", range(len(SEQ_OPTS)))
def test_seq_parity_both_paths(oi, monkeypatch):
    rng = random.Random(100 + oi)
    opts = SEQ_OPTS[oi]
    for wrap, width, crlf in [(60, 60, False), (0, 7, True), (-1, 0, False), (11, 60, False)]:
        data = make(rng, rng.randint(1, 200), False, wrap, crlf)
        w = want(data, False, opts, width)
        assert run(data, False, opts, width) == w, (opts, wrap, width)
        monkeypatch.setenv("BSK_REPLACE", "vm")
        assert run(data, False, opts, width) == w, (opts, wrap, width, "vm")
        monkeypatch.delenv("BSK_REPLACE")


def test_fixtures_records(tmp_path):
    for f in FIX["records"]:
        opts = dict(f["opts"])
        if opts.get("KvFile") == "@kv":
            p = tmp_path / "kv.tsv"
            p.write_bytes(f["kv"].encode())
            opts["KvFile"] = str(p)
        assert run(f["in"].encode(), False, opts) == f["want"].encode(), f


def test_fixtures_replace_all_on_device():
    # every ReplaceAll fixture as a name replacement of one record (the name is the text)
    for f in FIX["replace_all"]:
        if "\n" in f["text"] or not f["text"]:
            continue
        data = (">" + f["text"] + "\nACGT\n").encode()
        got = run(data, False, {"Pattern": f["expr"], "Replacement": f["repl"]})
        assert got == (">" + f["want"] + "\nACGT\n").encode(), f


def test_kv_options(tmp_path):
    rng = random.Random(7)
    kv = tmp_path / "kv.tsv"
    kv.write_bytes(b"id1\tONE\r\nID2\tTwo$$$$x\nid3\t$1-${1}\nshort\nid4\t\n")
    data = make(rng, 400, False)
    fq = make(rng, 300, True)
    base = {"Pattern": "^(\\w+?)(\\d+)", "KvFile": str(kv)}
    for extra in [{}, {"KeepUntouch": True}, {"KeepKey": True}, {"KeyMissRepl": "NA"}, {"IgnoreCase": True},
                  {"KeepKey": True, "KeepUntouch": True}, {"KeyCaptIdx": 2, "KeyMissRepl": "m$1"}]:
        for r in ["{kv}", "x_{kv}_{nr}", "${1}{kv}", "{KV}{kv}"]:
            opts = dict(base, Replacement=r, **extra)
            if extra.get("KeyCaptIdx") == 2:
                opts["Pattern"] = "^(\\w+?)(\\d)"
            for d, fastq in ((data, False), (fq, True)):
                assert run(d, fastq, opts) == want(d, fastq, opts, kv=kv.read_bytes()), opts


def test_errors_name_the_lowest_record(tmp_path):
    kv = tmp_path / "kv.tsv"
    kv.write_bytes(b"a\tb\n")
    names = ["r%d" % i for i in range(5000)]
    names[3100] = "r3100 aa"
    names[4200] = "r4200 aa"
    data = "".join(">%s\nAC\n" % n for n in names).encode()
    with pytest.raises(BskError) as e:
        run(data, False, {"Pattern": "(a)", "Replacement": "{kv}", "KvFile": str(kv)})
    assert 'pattern "(a)" matches multiple targets in "r3100 aa", this will cause chaos' in str(e.value)
    with pytest.raises(BskError) as e:
        run(data, False, {"Pattern": "(aa)", "Replacement": "{kv}", "KvFile": str(kv), "KeyCaptIdx": 2})
    assert "value of flag -I (--key-capt-idx) overflows" in str(e.value)
    # no record matches: no overflow error (raised only for a match)
    assert run(b">zz\nAC\n", False, {"Pattern": "(aa)", "Replacement": "{kv}", "KvFile": str(kv), "KeyCaptIdx": 2}) == b">zz\nAC\n"
    with pytest.raises(BskError) as e:
        run(b"@a\nAC\n+\nII\n", True, {"Pattern": "A", "Replacement": "x", "BySeq": True})
    assert "editing FASTQ is not supported" in str(e.value)
    assert run(b"", True, {"Pattern": "A", "Replacement": "x", "BySeq": True}) == b""
    with pytest.raises(BskError) as e:
        run(b">a\nAC\n>b\xc3\xa9\nAC\n", False, {"Pattern": "."})
    assert "0x80" in str(e.value)


def test_nr_restarts_per_partition():
    data = "".join(">s%d\nACGT\n" % i for i in range(1000)).encode()
    opts = {"Pattern": "^s(\\d+)", "Replacement": "{nr}"}
    out = run(data, False, opts, parts=2)
    nums = [int(l[1:]) for l in out.split(b"\n") if l.startswith(b">")]
    assert len(nums) == 1000 and nums[0] == 1 and nums.count(1) == 2
    k = nums.index(1, 1)
    assert nums == list(range(1, k + 1)) + list(range(1, 1000 - k + 1))


def test_long_record_both_seq_paths(monkeypatch):
    rng = random.Random(3)
    seq = "".join(rng.choice("ACGTN") for _ in range((1 << 20) + 4321))
    data = (">chr1 long\n" + "".join(seq[k:k + 70] + "\n" for k in range(0, len(seq), 70)) + ">c2\nNNA\n").encode()
    for opts in ({"Pattern": "N", "Replacement": "nn", "BySeq": True}, {"Pattern": "[GC]", "Replacement": "", "BySeq": True}):
        w = want(data, False, opts, 60)
        assert run(data, False, opts, 60) == w
        monkeypatch.setenv("BSK_REPLACE", "vm")
        assert run(data, False, opts, 60) == w
        monkeypatch.delenv("BSK_REPLACE")
    opts = {"Pattern": "long", "Replacement": "L{nr}"}
    assert run(data, False, opts, 60) == want(data, False, opts, 60)


@pytest.mark.parametrize("vm", [False, True])
def test_seq_group_beside_the_class(vm, monkeypatch):
    """An empty group next to the byte class is not the byte: `()N` with $1 gives [] (the per-byte path must not take it)."""
    if vm:
        monkeypatch.setenv("BSK_REPLACE", "vm")
    data = b">s\nANNA\n>t\nNACN\n"
    for p, r in [("()N", "[$1]"), ("N()", "[$1]"), ("(?P<g>)N", "[${g}]"), ("()(N)", "[$1$2]"), ("(N)", "[$1]"), ("N", "[$1$0]")]:
        opts = {"Pattern": p, "Replacement": r, "BySeq": True}
        assert run(data, False, opts) == want(data, False, opts), (p, r)
    assert run(b">s\nANNA\n", False, {"Pattern": "()N", "Replacement": "[$1]", "BySeq": True}) == b">s\nA[][]A\n"


def test_up_to_nine_groups():
    """Templates that reference groups 4 - 9 run the 20-slot matcher on names and sequences."""
    rng = random.Random(9)
    p = "(a)(b)?(c)(d)(e)?(f)(g)(h)?(i)"
    names = ["abcdefghi", "acdfgi", "xabcdefghiy abcd", "nomatch"]
    data = "".join(">%s\nabcdfgi%s\n" % (n, "".join(rng.choice("abcdefghi") for _ in range(40))) for n in names).encode()
    for opts in ({"Pattern": p, "Replacement": "<$9$8$7$6$5$4>"}, {"Pattern": p, "Replacement": "${7}_$1", "BySeq": True},
                 {"Pattern": "(?P<x>a)(b)(c)(?P<y>d)", "Replacement": "$4${y}${x}"}):
        assert run(data, False, opts) == want(data, False, opts), opts


CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")


def cli(args, env_extra=None, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    p = subprocess.run([CLI] + args, capture_output=True, cwd=ROOT, env=env, timeout=timeout)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    return p.stdout


def test_cli_single_streamed_and_workers(tmp_path):
    rng = random.Random(11)
    data = make(rng, 3000, False, 60)
    src = str(tmp_path / "in.fa")
    open(src, "wb").write(data)
    opts = {"Pattern": "^(\\S+)", "Replacement": "n{nr}_${1}", "NrWidth": 4}
    args = ["replace", "-p", opts["Pattern"], "-r", opts["Replacement"], "--nr-width", "4", src]
    w = want(data, False, opts)
    assert cli(args + ["-o", "-"]) == w
    # streamed in pieces and small chunks: ONE partition, {nr} goes on across them
    out = str(tmp_path / "streamed")
    cli(args + ["--devices", "0", "-o", out, "--merge"],
        {"BSK_HOST_PIPELINE_FROM": "0", "BSK_STAGE_BYTES": "4096", "BSK_STREAM_PIECE_BYTES": "30000"})
    assert open(out, "rb").read() == w
    # two workers: two partitions, each numbers from 1
    out = str(tmp_path / "workers")
    cli(args + ["--devices", "0,0", "-o", out, "--merge"])
    got = open(out, "rb").read()
    heads = [l for l in got.split(b"\n") if l.startswith(b">")]
    assert len(heads) == 3000 and sum(h.startswith(b">n0001_") for h in heads) == 2
    k = [i for i, h in enumerate(heads) if h.startswith(b">n0001_")][1]
    first, second = data.split(b"\n>")[:k], data.split(b"\n>")[k:]
    part1 = b"\n>".join(first) + b"\n"
    part2 = b">" + b"\n>".join(second)
    assert got == want(part1, False, opts) + want(part2, False, opts)
    # -s through the streamed path
    out = str(tmp_path / "seq")
    cli(["replace", "-s", "-p", "[GC]", "-r", "", "-w", "7", src, "--devices", "0", "-o", out, "--merge"],
        {"BSK_HOST_PIPELINE_FROM": "0", "BSK_STAGE_BYTES": "4096", "BSK_STREAM_PIECE_BYTES": "30000"})
    assert open(out, "rb").read() == want(data, False, {"Pattern": "[GC]", "Replacement": "", "BySeq": True}, 7)
