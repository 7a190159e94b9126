"""The gzip segment reader without a GPU (PARITY.md GZIP "segments"): the reader with its host backend against zlib and the piece
rule restated in gzip_stream_ref -- on the corpus of gzip_ref at three segment sizes, on small shapes that aim at the resume
points, on every malformed file, on streams without a block start to resume at --, its memory, the compiler's report for the new
kernels, the header alone under the host's sanitizers, and what the command line says before a device is touched."""
import os
import re
import subprocess

import pytest

import gzip_ref as G
import gzip_stream_ref as S
import bigseqkit_amd as bsk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
READER = bsk.GzipReader   # what this file is about
HOST = -1


def put(tmp_path, name, data):
    p = str(tmp_path / (name + ".gz"))
    open(p, "wb").write(data)
    return p


def check_file(tmp_path, name, data, fmt, piece, look, settings, device=HOST):
    """the reader on one file at every (segment, chunk): the text is zlib's, the pieces are the model's -- so they are the same
    at every setting --, and .piece() gives the same bytes again (read_all); returns the infos"""
    want = S.expected(data)
    model = S.model(want, fmt, piece, look)
    path, infos = put(tmp_path, name, data), []
    for segment, chunk in settings:
        got, info = S.read_all(path, fmt, device, piece, look, segment, chunk)
        assert b"".join(b for b, _, _ in got) == want, (name, segment, chunk)
        assert [(lo, hi) for _, lo, hi in got] == model, (name, segment, chunk)
        assert info["text_bytes"] == len(want), (name, segment, chunk, info)
        infos.append(info)
    return infos


def test_corpus_text_and_pieces_at_three_segment_sizes(tmp_path):
    for name, (data, chunk) in G.corpus().items():
        want = S.expected(data)
        piece, look = S.sizes_of(want)
        infos = check_file(tmp_path, name, data, S.fmt_of(name), piece, look, S.settings(data, chunk))
        assert infos[2]["segments"] == 1 and infos[2]["doublings"] == 0, (name, infos[2])
        if name in G.LEVELS or name in G.MEMLEVELS:     # files of dynamic blocks: many segments, none of them grown
            assert infos[0]["segments"] >= 4 and infos[0]["access_points"] == infos[0]["segments"] and infos[0]["doublings"] == 0, (name, infos[0])


def test_match_reaches_32768_back_across_segment_ends(tmp_path):
    """far_32768 at a segment of two 1 KiB chunks: it holds a stored and a fixed block, so the segment grows to the file and the
    text is exact; far_across_segments has the same match behind dynamic blocks: the match is resolved through a window that a
    dozen segments have carried on, each of which brought less than 32 KiB of text"""
    data, _ = G.corpus()["far_32768"]
    info, = check_file(tmp_path, "far_32768", data, S.FQ, 1000, 500, [S.SMALL])
    assert info["segments"] == 1 and info["doublings"] >= 4, info
    data, text = S.far_across_segments()
    infos = check_file(tmp_path, "far_across", data, S.FQ, 5000, 500, [S.SMALL, (4096, 1024), (1 << 20, 1024)])
    assert infos[0]["segments"] >= 10 and infos[0]["doublings"] == 0, infos[0]
    assert len(text) / infos[0]["segments"] < 32768


def test_window_mixes_carried_window_and_symbols(tmp_path):
    """segments of two chunks on files of dynamic blocks: every segment brings less than 32 KiB of text, so the window of its
    second chain chunk, and the window it leaves behind, hold bytes of the carried window and bytes of its own"""
    for name in ("ml1_l6", "ml1_l9", "sync_flush"):
        data, _ = G.corpus()[name]
        want = S.expected(data)
        info, = check_file(tmp_path, name, data, S.FQ, len(want) // 3, 1000, [S.SMALL])
        assert info["segments"] >= 10 and len(want) / info["segments"] < 32768, (name, info)


def test_member_ends_inside_chunk_0_and_at_a_segments_last_byte(tmp_path):
    for name in ("three_members", "empty_between", "header_fields"):
        data, _ = G.corpus()[name]
        want = S.expected(data)
        ends = S.member_ends(data)
        assert len(ends) >= 2
        settings = S.member_end_settings(ends)
        infos = check_file(tmp_path, name, data, S.FQ, len(want) // 4, 1500, settings)
        assert all(i["members"] == len(ends) for i in infos), (name, infos)


def test_reach_in_front_of_the_member_across_a_segment_end(tmp_path):
    for name, (data, chunk) in G.reach_before_member().items():
        first = G.gz(G.fastq(100_000, 31), 6)
        assert data.startswith(first)
        path = put(tmp_path, name, data)
        for segment in (len(first), len(first) - 700, 2048, 16384):     # a segment end on, in front of and far from the members' border
            code, msg = S.refusal(path, S.FQ, HOST, 20000, 1000, segment, chunk)
            assert code == 3 and "member 1 at offset" in msg and "distance too far back" in msg, (name, segment, msg)


def _where(msg):
    m = re.search(r"member (\d+) at offset (\d+)", msg)
    return m.groups() if m else None


def test_malformed_are_refused_as_by_the_whole_file_call(tmp_path):
    for name, (data, chunk, code, words) in G.malformed().items():
        with pytest.raises(bsk.BskError) as whole:
            bsk.GzipInflate(data, device=-1, chunk_bytes=chunk)
        path = put(tmp_path, name, data)
        for segment in (4 * chunk, 16 * chunk):
            got, msg = S.refusal(path, S.FQ, HOST, 100_000, 2000, segment, chunk)
            assert got == code == whole.value.code and words in msg, (name, segment, msg)
            assert _where(msg) == _where(str(whole.value)), (name, segment, msg, str(whole.value))   # members and offsets of the whole file


def test_wrong_crc_in_a_member_of_many_segments(tmp_path):
    good, bad, trailer = S.long_member()
    info, = check_file(tmp_path, "long_good", good, S.FQ, 100_000, 2000, [(8192, 1024)])
    assert info["segments"] >= 6 and info["members"] == 2
    path = put(tmp_path, "long_bad", bad)
    code, msg = S.refusal(path, S.FQ, HOST, 100_000, 2000, 8192, 1024)
    assert code == 3 and "member 0 at offset %d: CRC mismatch" % trailer in msg, msg
    # .piece() checks the DEFLATE stream only: the bytes of the bad member are handed out
    with READER(path, S.FQ, device=HOST, piece_text_bytes=100_000, lookahead_bytes=2000, segment_bytes=8192, chunk_bytes=1024) as r:
        assert r.piece(1000, 3000) == S.expected(good)[1000:3000]


def test_streams_without_a_block_start_grow_the_segment(tmp_path):
    for name in ("fixed_only", "level0", "stored_false"):
        data, chunk = G.corpus()[name]
        want = S.expected(data)
        piece, look = S.sizes_of(want)
        info, = check_file(tmp_path, name, data, S.fmt_of(name), piece, look, [(len(data) // 5, 2048)])
        assert info["doublings"] >= 2 and info["segments"] == 1, (name, info)
        # the cap (32 times the segment) under the file size: BSK_ERR_CAPACITY, which names the sizes
        segment = 2048
        assert 32 * segment < len(data)
        code, msg = S.refusal(put(tmp_path, name, data), S.fmt_of(name), HOST, piece, look, segment, 1024)
        assert code == 7 and "no non-final dynamic block" in msg and "segment of %d bytes" % segment in msg and "limit of %d bytes" % (32 * segment) in msg, (name, msg)


def test_memory_does_not_follow_the_file(tmp_path):
    data, chunk = G.corpus()["ml2_l1"]
    want = S.expected(data)
    peaks = []
    for name, d, w in (("once", data, want), ("four_times", data * 4, want * 4)):
        got, info = S.read_all(put(tmp_path, name, d), S.FQ, HOST, 40_000, 2000, 16384, chunk, again=False)
        assert b"".join(b for b, _, _ in got) == w and info["doublings"] == 0
        peaks.append(info["peak_bytes"])
    assert peaks[0] == peaks[1] and peaks[1] < 4 * len(want), peaks     # (the second text would not fit into what the reader held)


LDS = {"k_gzs_size": 3672, "k_gzs_decode": 69216}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_use_no_scratch(tmp_path):
    """the compiler's resource report for gfx950: no scratch and no spilled register in the kernels of the new file, and the LDS
    of the walks they repeat (tests/test_gzip_cpu.py): still two decode waves per CU"""
    src = os.path.join(ROOT, "bigseqkit_amd", "csrc", "ops_gzip_stream.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", str(tmp_path / "o.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(re.findall(r"void (k_\w+)\(", open(src).read())) == sorted(LDS)          # every kernel of the file
    seen = {}
    for b in r.stderr.split("Function Name: ")[1:]:
        sym = b.split(" ", 1)[0]
        for k in LDS:
            if re.search(r"\d" + k + "E", sym):
                seen[k] = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
                assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, sym
                assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0 and int(re.search(r"SGPRs Spill: (\d+)", b).group(1)) == 0, sym
    assert seen == LDS, seen
    assert 2 * LDS["k_gzs_decode"] <= 160 * 1024


def test_reader_under_sanitizers(tmp_path):
    """tests/host_c/gzip_stream_check.cpp -- the reader's header with its host backend and nothing of the library -- built with
    the host's address and undefined-behaviour sanitizers: the text and the model's pieces on the corpus at four chunks a segment
    and on the small shapes, a refusal on the malformed files, and no report"""
    exe = str(tmp_path / "gzip_stream_check")
    src = os.path.join(ROOT, "tests", "host_c", "gzip_stream_check.cpp")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("the sanitizer runtime cannot be linked here")
    assert r.returncode == 0, r.stderr[-2000:]

    def run(path, fmt, piece, look, segment, chunk):
        p = subprocess.run([exe, path, str(fmt), str(piece), str(look), str(segment), str(chunk), str(tmp_path / "text")], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and not p.stderr, (path, segment, p.stdout[-500:], p.stderr[-2000:])
        return p.stdout.splitlines()

    cases = {name: (data, chunk, S.fmt_of(name)) for name, (data, chunk) in G.corpus().items()}
    cases["far_across"] = (S.far_across_segments()[0], 1024, S.FQ)
    cases["long_member"] = (S.long_member()[0], 1024, S.FQ)
    for name, (data, chunk, fmt) in cases.items():
        want = S.expected(data)
        piece, look = S.sizes_of(want)
        model = S.model(want, fmt, piece, look)
        path = put(tmp_path, name, data)
        for segment in (4 * chunk,):
            out = run(path, fmt, piece, look, segment, chunk)
            assert out[-1].startswith("ok %d %d " % (len(model), len(want))), (name, segment, out[-1])
            assert [tuple(int(x) for x in l.split()[1:3]) for l in out[:-1]] == model, (name, segment)
            assert (tmp_path / "text").read_bytes() == want, (name, segment)
    bad = {k: (d, c) for k, (d, c, _, _) in G.malformed().items() if k != "too_many_members"}
    bad.update(G.reach_before_member())
    bad["long_bad"] = (S.long_member()[1], 1024)
    for name, (data, chunk) in bad.items():
        out = run(put(tmp_path, name, data), S.FQ, 100_000, 2000, 4 * chunk, chunk)
        assert out[-1].startswith("refused 3 "), (name, out[-1])


CLI = os.path.join(ROOT, "bigseqkit_amd", "bin", "bigseqkit")
NO_DEVICE = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}
NO_SWITCH = (" is gzip but not BGZF: one gzip stream cannot be cut into independent blocks, so it is not read; recompress it with bgzip "
             "(gzip -dc FILE | bgzip > FILE.gz) or decompress it first, or set BSK_GZIP=1 to have it inflated whole, in speculative chunks, "
             "where the file and its text fit one GPU")
DEVICES = (" is gzip but not BGZF, and --devices cuts a file by its bytes: where a worker starts in a gzip stream is known only after a pass "
           "over the stream in front of it, so BSK_GZIP_STREAM=1 reads it in pieces on one device only; run it on one device (--device N), or "
           "decompress it first (gzip -d)")


def test_command_line_refusals_without_a_device(tmp_path):
    import gzip
    z = put(tmp_path, "one.fq", gzip.compress(b"@r0 d=0\nACGTACGTAC\n+\nIIIIIIIIII\n", mtime=0))

    def refused(args, env, want):
        e = {k: v for k, v in os.environ.items() if not k.startswith(("BSK_GZIP", "BSK_BGZF_STREAM"))}
        r = subprocess.run([CLI, *args], capture_output=True, timeout=120, env=dict(e, **NO_DEVICE, **env))
        assert r.returncode == 1 and r.stderr.decode() == "Error: " + want + "\n", (args, env, r.stderr)

    both = {"BSK_GZIP": "1", "BSK_GZIP_STREAM": "1"}
    refused(["stats", "--devices", "0", z], both, z + DEVICES)
    refused(["stats", "--devices", "0", z], dict(both, BSK_BGZF_STREAM="1"), z + DEVICES)
    # the new switch alone means nothing: the text of a run without any switch
    for args in (["stats", z], ["stats", "--devices", "0", z], ["common", z, z], ["pair", "-O", str(tmp_path / "o"), z, z]):
        for env in ({"BSK_GZIP_STREAM": "1"}, {"BSK_GZIP_STREAM": "1", "BSK_GZIP": "0"}, {"BSK_GZIP_STREAM": "1", "BSK_COMMON_BUDGET_BYTES": "1", "BSK_PAIR_BUDGET_BYTES": "1"}):
            refused(args, env, z + NO_SWITCH)
