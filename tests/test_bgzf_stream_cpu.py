"""The piece reader of a BGZF file without a GPU (PARITY.md BGZF "pieces"): the reader on the host (device = -1) against zlib
and against the rule restated in bgzf_stream_ref.model, at every chunk size; what the cases cover; the refusals with the block
counted over the whole file; the cut function of the kernel, run on the host, against bsk_find_record_start; the compiler's
report for the kernel; and the reader alone under the host's sanitizers."""
import os
import re
import subprocess

import pytest

import bgzf_ref as R
import bgzf_stream_ref as S
import bigseqkit_amd as bsk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
READER = bsk.BgzfReader   # what this file is about


@pytest.fixture(scope="module")
def cases():
    return S.cases()


def test_cases_cover_what_they_claim(cases):
    """the shapes the reader must meet are in the files: asserted here, so that the cases cannot quietly cover less"""
    carries = set()
    for name, (data, fmt, piece, look) in cases.items():
        want, text = S.model(data, fmt, piece, look)
        carries |= {w[4] for w in want[:-1]}
        if name in ("empty_file", "eof_alone", "empty_blocks_only"):
            assert text == b"" and want == [(0, 0, len(data) << 16, len(data) << 16, 0)], name
        elif name == "fq_one_piece":
            assert len(want) == 1
        else:
            assert len(want) >= 4, (name, len(want))
    # a record that straddles a piece end: carried heads of every length modulo 16, short ones among them
    assert {c % 16 for c in carries} == set(range(16)) and min(carries) > 0
    assert any(c >= 33 for c in carries) and any(c < 33 for c in carries)
    # stored, fixed and dynamic blocks; ISIZE-0 blocks; an EOF block in the middle and none at the end
    assert S.block_types(cases["fq_mixed"][0]) == {0, 1, 2}
    idx = R.index(cases["fq_cat_two_files"][0])
    assert sum(1 for _, _, isize, _ in idx if isize == 0) >= 4 and idx[-1][2] == 0
    mid = cases["fq_cat_two_files"][0].find(R.EOF_BLOCK)
    assert 0 < mid < len(cases["fq_cat_two_files"][0]) - 28
    assert not cases["fa_no_eof"][0].endswith(R.EOF_BLOCK)
    assert not S.model(*cases["fq_no_last_newline"])[1].endswith(b"\n")
    # the grow path: a record longer than piece + lookahead makes a longer piece
    data, fmt, piece, look = cases["fa_long_record"]
    assert max(w[1] - w[0] for w in S.model(data, fmt, piece, look)[0]) > 9000 > piece + look
    # '@'- and '+'-led quality lines where the cuts fall, and a wrapped file that the strict rule does not read
    data, fmt, piece, look = cases["fq_small_pieces"]
    want, text = S.model(data, fmt, piece, look)
    near = [text[max(0, w[1] - 200):w[1] + 200] for w in want[:-1]]
    assert any(b"\n+\n@" in t or b"\n@" in t.replace(b"\n@read", b"") for t in near) and any(b"\n+\n+" in t for t in near)
    # a block that straddles a chunk end: at 1000 bytes a chunk, every file of blocks of a few hundred bytes has one
    offs = [off for off, _, _, _ in idx]
    assert any(off // 1000 != (off + bsize - 1) // 1000 for off, bsize, _, _ in idx)


@pytest.mark.parametrize("name", list(S.cases()))
def test_host_reader_equals_zlib_and_the_rule(tmp_path, cases, name):
    """the pieces joined are the text, every boundary is a record start, the offsets are the model's at every chunk size, and
    piece(lo, hi) gives the bytes again"""
    S.check_case(tmp_path, name, cases[name], -1)


def test_host_reader_seek_inside_a_block(tmp_path, cases):
    data, fmt, piece, look = cases["fa_mixed"]
    want, text = S.model(data, fmt, piece, look)
    path = tmp_path / "fa.gz"
    path.write_bytes(data)
    with READER(path, fmt, device=-1, piece_text_bytes=piece, lookahead_bytes=look, comp_chunk_bytes=900) as r:
        assert any(w[2] & 0xffff for w in want[1:])
        for w in (want[3], want[1], want[2]):
            r.seek(w[2])
            b, lo, hi = next(r)
            assert (lo, hi) == (w[2], w[3]) and b == text[w[0]:w[1]]
        with pytest.raises(bsk.BskError):
            r.seek((len(data) << 16) + 1)
        r.seek(len(data) << 16)
        assert next(r) == (b"", len(data) << 16, len(data) << 16)


def test_host_reader_refuses_malformed(tmp_path):
    for name, (data, chunk, code, block, off, word) in S.malformed_in_second_chunk().items():
        path = tmp_path / (name + ".gz")
        path.write_bytes(data)
        with pytest.raises(bsk.BskError) as e:
            with READER(path, S.FQ, device=-1, piece_text_bytes=1500, lookahead_bytes=600, comp_chunk_bytes=chunk) as r:
                list(r)
        assert e.value.code == code and word in str(e.value), (name, str(e.value))
        if block is not None:
            assert ("block %d at offset %d:" % (block, off)) in str(e.value), (name, str(e.value))
    # every refusal of the whole-file path, with the same block and the same word
    M, good, text = R.malformed()
    for name, (data, code, block, word) in M.items():
        path = tmp_path / (name + ".gz")
        path.write_bytes(data)
        with pytest.raises(bsk.BskError) as e:
            with READER(path, S.FQ, device=-1, piece_text_bytes=1500, lookahead_bytes=600, comp_chunk_bytes=3000) as r:
                list(r)
        assert e.value.code == code and word in str(e.value), (name, str(e.value))
        if block is not None:
            assert ("block %d at offset" % block) in str(e.value), (name, str(e.value))


def test_cut_function_agrees_or_declines():
    """stream_cut, the function k_bgzf_stream_cut runs, on the host: bsk_find_record_start's answer or "declined", never another
    offset -- and on plain four-line text it does answer"""
    answered = {S.FA: 0, S.FQ: 0}
    for window, frm, fmt in S.fuzz_windows(5, 1500):
        got = S.stream_cut(window, frm, fmt, -1)
        if got != S.DECLINED:
            assert got == S.find_record_start(window, frm, fmt), (window, frm, fmt, got)
            answered[fmt] += 1
    assert answered[S.FA] >= 250 and answered[S.FQ] >= 300, answered


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernel_uses_no_scratch(tmp_path):
    """the compiler's resource report for gfx950: the one kernel of the file uses no scratch, spills nothing and holds no LDS"""
    src = os.path.join(ROOT, "bigseqkit_amd", "csrc", "ops_bgzf_stream.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", str(tmp_path / "o.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want = {"k_bgzf_stream_cut": 0}
    assert sorted(re.findall(r"void (k_\w+)\(", open(src).read())) == sorted(want)          # every kernel of the file
    seen = {}
    for b in r.stderr.split("Function Name: ")[1:]:
        sym = b.split(" ", 1)[0]
        for k in want:
            if re.search(r"\d" + k + "E", sym):
                seen[k] = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
                assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, sym
                assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0 and int(re.search(r"SGPRs Spill: (\d+)", b).group(1)) == 0, sym
    assert seen == want, seen


def test_reader_under_sanitizers(tmp_path, cases):
    """tests/host_c/bgzf_stream_check.cpp -- the reader's header with its host backend and nothing of the library -- built with
    the host's address and undefined-behaviour sanitizers: the text on every case at two chunk sizes, the pieces of the model,
    a refusal on the malformed files, and no report"""
    exe = str(tmp_path / "bgzf_stream_check")
    src = os.path.join(ROOT, "tests", "host_c", "bgzf_stream_check.cpp")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("the sanitizer runtime cannot be linked here")
    assert r.returncode == 0, r.stderr[-2000:]
    out = str(tmp_path / "text")
    for name, (data, fmt, piece, look) in cases.items():
        want, text = S.model(data, fmt, piece, look)
        (tmp_path / "in").write_bytes(data)
        for chunk in (300, len(data) + 1):
            p = subprocess.run([exe, str(tmp_path / "in"), str(fmt), str(piece), str(look), str(chunk), out], capture_output=True, text=True, timeout=120)
            lines = p.stdout.splitlines()
            assert p.returncode == 0 and not p.stderr and lines[-1] == "ok %d %d" % (len(want), len(text)), (name, lines[-3:], p.stderr[-2000:])
            assert lines[:-1] == ["piece %d %d %d" % (w[2], w[3], w[1] - w[0]) for w in want], name
            assert open(out, "rb").read() == text, name
    for name, (data, chunk, code, block, off, word) in S.malformed_in_second_chunk().items():
        (tmp_path / "in").write_bytes(data)
        p = subprocess.run([exe, str(tmp_path / "in"), "1", "1500", "600", str(chunk), out], capture_output=True, text=True, timeout=120)
        last = p.stdout.splitlines()[-1]
        assert p.returncode == 0 and not p.stderr and last.startswith("refused %d " % code) and word in last, (name, last, p.stderr[-2000:])
