"""`replace` without a GPU: Before() of the reference (messages and their order, readKVs, the log lines), and the
device's ReplaceAll / Expand routines run on the host (bsk_regex_replace) against tests/replace_ref.py."""
import ctypes as C
import json
import os
import random
import re
import subprocess

import pytest

import bigseqkit_amd as bsk
from bigseqkit_amd._lib import lib
import replace_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "replace_fixtures.json")))


def create(opts):
    ctx = C.c_void_p()
    rc = lib.bsk_create(b"Replace", json.dumps(opts).encode(), -1, C.byref(ctx))
    if rc == 0:
        log = lib.bsk_log_text(ctx).decode()
        lib.bsk_destroy(ctx)
        return 0, log
    return rc, lib.bsk_global_error().decode()


def regex_replace(expr, repl, text, too_large_ok=False):
    cap = 4 * len(text) * (len(repl) + 1) + 64
    out = C.create_string_buffer(cap)
    n = C.c_size_t()
    rc = lib.bsk_regex_replace(expr.encode(), repl.encode(), text, len(text), out, cap, C.byref(n))
    if rc and too_large_ok and "too large" in lib.bsk_global_error().decode():
        return None
    assert rc == 0, lib.bsk_global_error().decode()
    return out.raw[:n.value]


def test_before_messages_in_order(tmp_path):
    kv = tmp_path / "kv.tsv"
    kv.write_bytes(b"a\tb\n")
    empty = tmp_path / "empty.tsv"
    empty.write_bytes(b"onlykey\n\n")
    cases = [
        ({"Config": {"SeqType": "xyz"}}, None),  # alphabet first
        ({}, "flags -p (--pattern) needed"),
        ({"Pattern": "a(", "Replacement": ""}, "error parsing regexp"),
        ({"Pattern": "(a)", "KvFile": str(kv)}, "flag -r (--replacement) needed when given flag -k (--kv-file)"),
        ({"Pattern": "(a)", "Replacement": "x", "KvFile": str(kv)},
         'replacement symbol "{kv}"/"{KV}" not found in value of flag -r (--replacement) when flag -k (--kv-file) given'),
        ({"Pattern": "a", "Replacement": "{kv}", "KvFile": str(kv)},
         'value of -p (--pattern) must contains "(" and ")" to capture data which is used specify the KEY'),
        ({"Pattern": "(a)", "Replacement": "{KV}", "BySeq": True, "KvFile": str(kv)},
         "replaceing with key-value pairs was not supported for sequence"),
        ({"Pattern": "(a)", "Replacement": "{kv}"},
         'since replacement symbol "{kv}"/"{KV}" found in value of flag -r (--replacement), tab-delimited key-value file '
         "should be given by flag -k (--kv-file)"),
        ({"Pattern": "(a)", "Replacement": "{kv}", "KvFile": str(tmp_path / "missing.tsv")},
         "read key-value file: open %s: no such file or directory" % (tmp_path / "missing.tsv")),
        ({"Pattern": "(a)", "Replacement": "{kv}", "KvFile": str(empty)}, "no valid data in key-value file: %s" % empty),
    ]
    for opts, msg in cases:
        rc, text = create(opts)
        assert rc == 2, (opts, rc, text)
        if msg is not None:
            assert msg in text, (opts, text)
    assert create({"Pattern": "a", "Replacement": "b"}) == (0, "")
    # an empty -p is checked before the expression is compiled; a bad -p before the -k checks
    assert create({"Pattern": "", "Replacement": "{kv}"})[1] == "flags -p (--pattern) needed"
    assert "error parsing regexp" in create({"Pattern": "(", "Replacement": "x", "KvFile": str(kv)})[1]


def test_kv_file_and_log_lines(tmp_path):
    kv = tmp_path / "kv.tsv"
    kv.write_bytes(b"A\t1\r\nshort\n\nb\t2\textra\nA\t3\nlast\tno newline")
    rc, log = create({"Pattern": "(x)", "Replacement": "{kv}", "KvFile": str(kv)})
    assert rc == 0
    assert log == "[INFO] read key-value file: %s\n[INFO] 3 pairs of key-value loaded\n" % kv
    assert R.read_kvs(kv.read_bytes(), False) == {b"A": b"3", b"b": b"2", b"last": b"no newline"}
    # -i folds the keys: A and a are one key
    kv.write_bytes(b"A\t1\na\t2\n")
    assert create({"Pattern": "(x)", "Replacement": "{kv}", "KvFile": str(kv), "IgnoreCase": True})[1].endswith(
        "[INFO] 1 pairs of key-value loaded\n")
    assert create({"Pattern": "(x)", "Replacement": "{kv}", "KvFile": str(kv)})[1].endswith("[INFO] 2 pairs of key-value loaded\n")
    assert create({"Pattern": "(x)", "Replacement": "{kv}", "KvFile": str(kv), "Config": {"Quiet": True}}) == (0, "")


def test_fixtures_replace_all():
    for f in FIX["replace_all"]:
        got = regex_replace(f["expr"], f["repl"], f["text"].encode())
        assert got == f["want"].encode(), f
        assert R.replace_all(R.compile_go(f["expr"]), f["text"].encode(), f["repl"].encode()) == got, f


def test_fixture_records_restated(tmp_path):
    for f in FIX["records"]:
        kvs = R.read_kvs(f.get("kv", "").encode(), f["opts"].get("IgnoreCase", False))
        assert R.replace_records(f["in"].encode(), False, f["opts"], kvs) == f["want"].encode(), f


def _rand_expr(rng):
    atoms = ["a", "b", "x", ".", "[ab]", "[^a]", "\\d", "[[:alpha:]]", "\\s", "_"]
    quants = ["", "", "*", "+", "?", "*?", "+?", "??", "{1,2}", "{2}"]

    def seq(depth):
        parts = []
        for _ in range(rng.randint(1, 3)):
            r = rng.random()
            if r < 0.15 and depth < 2:
                name = "(?P<g%d>" % rng.randint(0, 1) if rng.random() < 0.3 else rng.choice(["(", "(?:"])
                parts.append(name + alt(depth + 1) + ")")
            elif r < 0.22:
                parts.append(rng.choice(["^", "$", "\\b"]))
            else:
                parts.append(rng.choice(atoms) + rng.choice(quants))
        return "".join(parts)

    def alt(depth):
        return "|".join(seq(depth) for _ in range(rng.choice([1, 1, 2])))

    return alt(0)


def _rand_template(rng):
    pieces = ["-", "Z", "$0", "$1", "${1}", "$2", "$$", "${g0}", "$g1", "$1_x", "$", "${", "$01", "{", "}", " "]
    return "".join(rng.choice(pieces) for _ in range(rng.randint(0, 4)))


def test_random_against_restatement():
    rng = random.Random(20261016)
    n = 0
    while n < 3000:
        expr = _rand_expr(rng)
        if re.search(r"\(\?P<(g\d)>.*\(\?P<\1>", expr):
            continue  # a name used twice: Go rejects it
        try:
            rx = R.compile_go(expr)
        except re.error:
            continue
        tmpl = _rand_template(rng)
        text = "".join(rng.choice("abx1 _\t") for _ in range(rng.randint(0, 12))).encode()
        got = regex_replace(expr, tmpl, text, too_large_ok=True)
        if got is None:
            continue  # more than 64 instructions: refused, not answered
        assert got == R.replace_all(rx, text, tmpl.encode()), (expr, tmpl, text)
        n += 1


def test_unsupported_syntax_and_group_limit():
    assert create({"Pattern": "\\pL", "Replacement": "x"})[0] == 2
    assert "not supported" in create({"Pattern": "(?=a)", "Replacement": "x"})[1]
    groups = "".join("(%s)" % c for c in "abcdefghijk")
    assert create({"Pattern": groups, "Replacement": "$9"})[0] == 0
    rc, msg = create({"Pattern": groups, "Replacement": "$10"})
    assert rc == 2 and "more than 9 groups" in msg
    assert create({"Pattern": groups, "Replacement": "$12"})[0] == 0  # no such group: nothing to keep


def test_python_options_and_api():
    o = bsk.SeqKitReplaceOptions().Pattern("a").Replacement("b").NrWidth(3)
    assert json.loads(o.to_json())["NrWidth"] == 3
    assert callable(bsk.Replace)


@pytest.mark.parametrize("src,kernel,scratch", [("ops_idre.hip", "k_id_spans", 4112), ("ops_locate.hip", "k_locate_vmILb0", 4128),
                                                ("ops_locate.hip", "k_locate_vmILb1", 4128)])
def test_vm_scratch_unchanged(src, kernel, scratch):
    """The 4-slot instantiations of the Pike VM keep their private-memory footprint (build() needs hipcc: so does this)."""
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c",
                          "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage",
                          os.path.join(ROOT, "bigseqkit_amd", "csrc", src)], capture_output=True, text=True)
    m = re.search(kernel + r".*?ScratchSize \[bytes/lane\]: (\d+)", out.stderr, re.S)
    assert m and int(m.group(1)) == scratch, out.stderr[-2000:]


def test_cli_flag_table():
    """bigseqkit-cli/replace.go:70-83: every flag reaches its ReplaceOptions field."""
    cli = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")
    p = subprocess.run([cli, "replace", "-p", "^(\\S+)", "-r", "r{nr}", "--nr-width", "3", "-s", "-i", "-k", "kv.tsv", "-U", "-K",
                        "-I", "2", "-m", "NA", "x.fa", "--dry-run"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    op, js = p.stdout.splitlines()[:2]
    assert op == "Replace"
    o = json.loads(js)
    assert {k: o[k] for k in ("Pattern", "Replacement", "NrWidth", "BySeq", "IgnoreCase", "KvFile", "KeepUntouch", "KeepKey",
                              "KeyCaptIdx", "KeyMissRepl")} == {
        "Pattern": "^(\\S+)", "Replacement": "r{nr}", "NrWidth": 3, "BySeq": True, "IgnoreCase": True, "KvFile": "kv.tsv",
        "KeepUntouch": True, "KeepKey": True, "KeyCaptIdx": 2, "KeyMissRepl": "NA"}
    p = subprocess.run([cli, "replace", "x.fa", "--dry-run"], capture_output=True, text=True)
    o = json.loads(p.stdout.splitlines()[1])
    assert (o["NrWidth"], o["KeyCaptIdx"], o["BySeq"], o["Pattern"]) == (1, 1, False, "")
