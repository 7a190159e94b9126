"""`faidx -d` restated in Python (PARITY.md FAIX): rows of an index -> hits -> bytes by arithmetic on the original text, the
two checks, the 4 KiB span rule and the batch cuts.  The tests hold the planner (bsk_faidx_fetch_plan) and the fetch against
this; `oracle.faidx_query` on the whole text stays the oracle of the bytes.  Plus strand, and the minus strand of plain
ACGTN text (the complement table of other alphabets is the oracle's business)."""
import re

PAGE = 4096
MSG = "the index does not describe this file, or the record has lines of two widths; re-index / reformat with seq"
_COMP = bytes.maketrans(b"ACGTNacgtn", b"TGCANtgcan")


class Refused(Exception):
    pass


def parse_rows(fai, file_size, full_head=False, fastq=None):
    """-> (rows [(name, length, offset, linebases, linewidth)], fastq)"""
    lines = [l for l in fai.split(b"\n") if l]
    rows = []
    for k, line in enumerate(lines):
        if k == 0 and fastq is None:
            f = line.rsplit(b"\t", 5)
            fastq = (len(f) == 6 and all(x.isdigit() for x in f[1:]) and int(f[4]) - int(f[3]) == 1 and int(f[5]) > int(f[2]))
        ncol = 6 if fastq else 5
        f = line.rsplit(b"\t", ncol - 1)
        where = "faidx -d: index row %d" % (k + 1)
        if len(f) < ncol:
            raise Refused(where + ": fewer than %d tab-separated columns" % ncol)
        named = where + " (" + f[0].decode() + ")"
        for name, x in zip(("length", "offset", "linebases", "linewidth", "qualoffset"), f[1:]):
            if not (x.isdigit() and len(x) <= 19 and x.isascii()):
                raise Refused(named + ": column %s is not a number: %s" % (name, x.decode()))
        length, offset, lb, lw = [int(x) for x in f[1:5]]
        if length >= 1 << 32:
            raise Refused(named + ": length %d is 2^32 or more" % length)
        if not (lb == 0 and lw == 0) and lw - lb != 1:
            raise Refused(named + ": linewidth %d - linebases %d is not 1" % (lw, lb))
        if length > 0 and lb == 0:
            raise Refused(named + ": linebases 0 with length %d" % length)
        if offset > file_size or (length > 0 and (lb >= 1 << 32 or predicted_end(length, offset, lb, lw) > file_size)):
            raise Refused(named + ": offset %d or the predicted end of the sequence lies beyond the file (%d bytes)" % (offset, file_size))
        if not full_head and (b" " in f[0] or b"\t" in f[0]):
            raise Refused(named + ": the name holds a blank or tab")
        rows.append((f[0], length, offset, lb, lw))
    return rows, bool(fastq)


def predicted_end(length, offset, lb, lw):
    return offset + (length - 1) // lb * lw + (length - 1) % lb + 1


def parse_region(q):
    """parseRegion (bigseqkit-lib/faidx.go:536-567) -> (id, begin, end)"""
    for rx, f in ((r"^(.+?):(-?\d+)-(-?\d+)$", lambda m: (int(m[2]), int(m[3]))), (r"^(.+?):(\d+)$", lambda m: (int(m[2]), int(m[2]))),
                  (r"^(.+?):(-?\d+)-$", lambda m: (int(m[2]), -1)), (r"^(.+?):-(-?\d+)$", lambda m: (1, int(m[2])))):
        m = re.match(rx, q, re.S)
        if m:
            return (m[1],) + f(m)
    return q, 1, -1


def sub_location(length, start, end):
    if length == 0:
        return 0, 0
    s, t = start, end
    if s < 0:
        s = max(1, length + s + 1)
    if s == 0:
        s = 1
    if t < 0:
        t = length + t + 1
    t = min(t, length)
    if s > length or t < 1 or s > t:
        return 0, 0
    return s - 1, t


def head_id(name):
    for sep in (b" ", b"\t"):
        k = name.find(sep)
        if k > 0:
            return name[:k]
    return name


def wrapped_len(n, w):
    return n if (w < 1 or n == 0) else n + (n - 1) // w


def hits(rows, queries, file_size, ignore_case=False, full_head=False, line_width=60, use_regexp=False):
    """-> [dict(row, p0, p1, minus, header, lines=(lo, hi), probe, out_len)] in row order"""
    qs = {}
    if not use_regexp:
        for q in queries:
            i, b, e = parse_region(q)
            if ignore_case:
                i = i.lower()
            qs.setdefault(i.encode(), (b, e))
    out = []
    for k, (name, length, offset, lb, lw) in enumerate(rows):
        if length == 0:
            continue
        i = head_id(name) if full_head else name
        if use_regexp:
            if not any(re.search(q.encode(), i) for q in queries):
                continue
            p0, p1, minus, suffix = 0, length, False, b""
        else:
            key = i.lower() if ignore_case else i
            if key not in qs:
                continue
            b, e = qs[key]
            whole = (b == 1 and e == -1) or (b > 0 and e < 0)
            minus = (not whole) and b > e
            p0, p1 = sub_location(length, e if minus else b, b if minus else e)
            if p0 == p1:
                continue
            suffix = b"" if whole else b":%d-%d" % (b, e)
        header = b">" + i + suffix + b"\n"
        l0, l1 = p0 // lb, (p1 - 1) // lb
        lines = (offset + l0 * lw, min(file_size, offset + l1 * lw + min(lb, length - l1 * lb) + 1))
        out.append(dict(row=k, p0=p0, p1=p1, minus=minus, header=header, lines=lines, probe=predicted_end(length, offset, lb, lw),
                        out_len=len(header) + wrapped_len(p1 - p0, line_width) + 1))
    return out


def round_out(lo, hi, file_size):
    return lo // PAGE * PAGE, min(file_size, -(-hi // PAGE) * PAGE)


def merge(spans, file_size):
    v = sorted(s for s in (round_out(lo, hi, file_size) for lo, hi in spans) if s[1] > s[0])
    out = []
    for lo, hi in v:
        if out and lo <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


def probe_span(h, file_size):
    return min(h["probe"], file_size), min(h["probe"] + 2, file_size)


def batches(hs, file_size, budget, alphabet_bytes=0):
    """whole hits, in order, while what they read (lines and probe, each rounded out) and write stays within the budget"""
    def cost(h):
        c = 0
        for lo, hi in (h["lines"], probe_span(h, file_size)):
            lo, hi = round_out(lo, hi, file_size)
            c += max(0, hi - lo)
        return c + h["out_len"] + (alphabet_bytes if h["minus"] else 0)
    out, first, used = [], 0, 0
    for k, h in enumerate(hs):
        c = cost(h)
        if c > budget:
            raise Refused("above the budget")
        if k > first and used + c > budget:
            out.append((first, k))
            first, used = k, 0
        used += c
    if first < len(hs):
        out.append((first, len(hs)))
    res = []
    for a, b in out:
        want = []
        for h in hs[a:b]:
            want += [h["lines"], probe_span(h, file_size)]
        if alphabet_bytes and any(h["minus"] for h in hs[a:b]):
            want.append((0, min(alphabet_bytes, file_size)))
        sp = merge(want, file_size)
        res.append(dict(hits=(a, b), spans=sp, read_bytes=sum(hi - lo for lo, hi in sp), out_bytes=sum(h["out_len"] for h in hs[a:b])))
    return res


def read_bound(hs):
    """the condition of the issue: bytes read <= sum(line-extended span + 2 * 4096) + 2 * 4096 per end probe"""
    return sum(h["lines"][1] - h["lines"][0] + 2 * PAGE + 2 * PAGE for h in hs)


def fetch(text, rows, hs, line_width=60, fastq=False):
    """the bytes, by arithmetic on `text`; Refused(row, offset) where a check fails"""
    out = []
    n = len(text)
    for h in hs:
        name, length, offset, lb, lw = rows[h["row"]]

        def refuse(at):
            raise Refused("faidx -d: index row %d (%s), file offset %d: %s" % (h["row"] + 1, name.decode(), at, MSG))
        # check 2: the two bytes behind the predicted last base
        p = h["probe"]
        if p < n:
            if text[p] != 10 or (p + 1 < n and text[p + 1] not in (10, ord("+" if fastq else ">"))):
                refuse(p)
        # check 1: every byte of every line read
        last_line = (length - 1) // lb
        for line in range(h["p0"] // lb, (h["p1"] - 1) // lb + 1):
            nb = min(lb, length - line * lb)
            at = offset + line * lw
            for col in range(nb):
                if text[at + col] == 10:
                    refuse(at + col)
            if at + nb < n:
                if text[at + nb] != 10:
                    refuse(at + nb)
            elif line != last_line:
                refuse(at + nb)
        seq = bytes(text[offset + p // lb * lw + p % lb] for p in range(h["p0"], h["p1"]))
        if h["minus"]:
            seq = seq.translate(_COMP)[::-1]
        w = line_width
        body = seq if w < 1 else b"\n".join(seq[k:k + w] for k in range(0, len(seq), w))
        out.append(h["header"] + body + b"\n")
    return b"".join(out)


# ---------------------------------------------------------------- the shapes both test files run (host lane and device)
def _wrap(seq, w):
    return "".join(seq[k:k + w] + "\n" for k in range(0, len(seq), w))


def cases(T):
    """-> [(name, text, fastq, options)]: every one is held against oracle.faidx_query on the whole text"""
    import random
    rng = random.Random(21)
    dna = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    out = []
    # line shapes: linebases 1, 7, 60, one line longer than a tile; an empty record, one without a sequence line; no final newline
    big = dna(2 * T + 700)
    one = dna(70001)
    shapes = (">w1 d\n" + _wrap(dna(23), 1) + ">w7\n" + _wrap(dna(50), 7) + ">empty\n\n>none\n>w60 x y\n" + _wrap(big, 60) +
              ">line\n" + one + "\n>w7\n" + _wrap(dna(15), 7) + ">last\n" + _wrap(dna(33), 7)).rstrip("\n").encode()
    edge = ["w7:1-7", "w1:1-1", "w60:60-61", "line:70001-70001", "last:29-33", "empty", "none"]
    out.append(("line shapes, regions at column 0 and linebases - 1", shapes, False, {"Regions": edge}))
    out.append(("whole records, a name in two rows", shapes, False, {"Regions": ["w7", "line", "w1", "last", "w60"]}))
    n60 = len(big)
    for L in (T - 1, T, T + 1, 2 * T + 1):
        for b in (1, 37, 60):
            e = b + L - 1
            assert e <= n60
            out.append(("length %d from %d, both strands" % (L, b), shapes, False,
                        {"Regions": ["w60:%d-%d" % (b, e), "line:%d-%d" % (e, b)], "Config": {"SeqType": "dna"}}))
            out.append(("length %d from %d, minus strand of the wrapped record" % (L, b), shapes, False,
                        {"Regions": ["w60:%d-%d" % (e, b), "line:%d-%d" % (b, e)], "Config": {"SeqType": "dna"}}))
    for w in (0, 1, 3, 60, 100000):
        out.append(("LineWidth %d" % w, shapes, False, {"Regions": ["w60:7-%d" % (T + 500), "w7:50-2", "line:3-"], "Config": {"LineWidth": w}}))
    # the minus strand: lower case, IUPAC, U -- the alphabet guessed from the first record, and given
    iu = (">r1\n" + _wrap("ACGUacguNnRYSWKMBDHVryswkmbdhv" * 9, 11) + ">r2\n" + _wrap("acgtnACGTN-." * 30, 60)).encode()
    for t in ({}, {"SeqType": "rna"}, {"SeqType": "dna"}, {"SeqType": "protein"}):
        out.append(("minus strand %r" % (t,), iu, False, {"Regions": ["r1:200-3", "r2:-2--300", "r1:-1--1"], "Config": dict(t)}))
    dn = (">d\n" + _wrap("ACGTNacgtn" * 40, 60)).encode()
    out.append(("minus strand, DNA guessed", dn, False, {"Regions": ["d:390-5"]}))
    # more hits than one block's share of the tile table: 3 000 one-base hits
    many = "".join(">m%d\n%s\n" % (k, dna(1 + k % 5)) for k in range(3000)).encode()
    out.append(("3000 one-base hits", many, False, {"Regions": ["m%d:1-1" % k for k in range(3000)]}))
    # the order of the queries, -i, -r, FASTQ rows, -f
    names = (">chr1 x\nACGTACGTAC\nGGGGGTTTTT\n>chr2\nAAAACCCC\n>Chr3\nTTTT\n>x:y d\nACGTT\n").encode()
    out.append(("queries in reverse file order", names, False, {"Regions": ["x:y", "Chr3", "chr2:2-3", "chr1:4-12"]}))
    out.append(("-i", names, False, {"Regions": ["CHR3:2-", "chr3", "CHR1"], "IgnoreCase": True}))
    out.append(("-r", names, False, {"Regions": ["^chr\\d$", "y$"], "UseRegexp": True, "Config": {"LineWidth": 4}}))
    out.append(("-f", names, False, {"Regions": ["chr1:2-11", "x:y"], "FullHead": True}))
    fq = (b"@r1 d\nACGTACGTAA\n+\nIIIIIIIIII\n@r2\nGG\n+r2\n##\n@r3\nACGTN\n+\n>>>>>")
    out.append(("FASTQ rows", fq, True, {"Regions": ["r3", "r1:2-9", "r2:2-1"], "Config": {"SeqType": "dna"}}))
    queries = [["chr1"], ["chr1:2-5", "chr2:-3", "chr2:1-2"], ["chr1:5-2"], ["chr1:-5--1"], ["chr1:3"], ["chr1:15-"], ["chr3"], ["chr9"],
               ["chr2:100-200"], ["Chr3:2-", "chr1:-4", "x:y:1-2"]]  # (tests/test_faidx_gpu.py QUERIES)
    for qs in queries:
        for extra in ({}, {"IgnoreCase": True}, {"Config": {"LineWidth": 3}}):
            out.append(("QUERIES %r %r" % (qs, extra), names, False, dict({"Regions": qs}, **extra)))
    return out


TWO_WIDTHS = b">a\nACGTAC\nACGTAC\nACG\nACG\n"  # tests/test_faidx_gpu.py:51: the rows accept it, arithmetic cannot address it


def junk_outside(text, spans):
    """every byte outside the spans overwritten with '>'-and-newline junk"""
    junk = bytearray((b">junk\n>" * (len(text) // 7 + 1))[:len(text)])
    for lo, hi in spans:
        junk[lo:hi] = text[lo:hi]
    return bytes(junk)


# ---------------------------------------------------------------- BGZF: the block table (htslib's .gzi) with struct
def gzi_write(blocks):
    """blocks: (compressed offset, size, ISIZE, ...) of every block (bgzf_ref.index) -> the image of FILE.gzi"""
    import struct
    pairs, text = [], 0
    for k, b in enumerate(blocks):
        if k:
            pairs.append((b[0], text))
        text += b[2]
    return struct.pack("<Q", len(pairs)) + b"".join(struct.pack("<QQ", c, u) for c, u in pairs)


def gzi_read(image):
    """-> [(compressed offset, text offset)] of every block, the first one (0, 0) included"""
    import struct
    n = struct.unpack_from("<Q", image, 0)[0]
    assert len(image) == 8 + 16 * n
    return [(0, 0)] + [struct.unpack_from("<QQ", image, 8 + 16 * k) for k in range(n)]


def gzi_blocks(table, lo, hi):
    """the blocks [first, last] that hold text [lo, hi): the last block that begins at or before lo .. the block of byte hi - 1"""
    first = max(k for k, (c, u) in enumerate(table) if u <= lo)
    last = max(k for k, (c, u) in enumerate(table) if u <= hi - 1)
    return first, last


def blocks_bound(table, hs, file_size, probe_blocks=None):
    """blocks inflated <= sum over the hits of the blocks that its (4 KiB-rounded) line span overlaps, plus those of its end
    probe: every span is served by whole blocks, a merged span by no more than its parts.  probe_blocks=1 is the condition as
    the issue states it for blocks of 65 280 bytes ("+ 1 per probe"); None counts the blocks under the probe's page, which
    are many where blocks are smaller than a page"""
    n = 0
    for h in hs:
        lo, hi = round_out(h["lines"][0], h["lines"][1], file_size)
        first, last = gzi_blocks(table, lo, hi)
        n += last - first + 1
        if probe_blocks is None:
            lo, hi = round_out(*probe_span(h, file_size), file_size)
            if hi > lo:
                first, last = gzi_blocks(table, lo, hi)
                n += last - first + 1
        else:
            n += probe_blocks
    return n


def _Z():
    import bgzf_ref
    return bgzf_ref


def _seqgen():
    import seqgen
    return seqgen


def bgzf_files():
    """name -> (text, BGZF file): blocks of 100 and of 65 280 bytes, empty blocks in the middle, no EOF block"""
    import random
    rng = random.Random(12)
    text = _seqgen().random_fasta(rng, 40, 0, 900, width=60)
    big = ("".join(">big%d\n" % k + "".join("ACGTTGCAAC" * 6 + "\n" for _ in range(3000)) for k in range(4)) + ">tail\nACGT\n").encode()
    empty = _Z().write(b"", eof=False)
    holes = _Z().write(text[:1000], block=100, eof=False) + _Z().EOF_BLOCK + _Z().EOF_BLOCK + _Z().write(text[1000:], block=100, eof=False)
    return {"b100": (text, _Z().write(text, block=100)), "b65280": (big, _Z().write(big, block=65280)), "holes_no_eof": (text, holes),
            "b100_no_eof": (text, _Z().write(text, block=100, eof=False))}, empty


BGZF_QUERIES = {"b100": ["s3:5-40", "s7", "s20:200-61", "s0:1-1", "s39"], "holes_no_eof": ["s1", "s2:3-70", "s30", "s39:-5--1"],
                "b100_no_eof": ["s39", "s5:10-2"], "b65280": ["big0:1000-1100", "big1:65000-1000", "big2:179990-", "tail", "big3"]}


