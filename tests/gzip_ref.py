"""Plain gzip (PARITY.md GZIP): the corpus of the gzip tests, each file with the chunk size it is run at, the malformed files,
and a restatement of what the library's finder and walk must give -- the finder's predicate (can a non-final dynamic block
start at this bit?), the lowest hit per chunk, and the walk over every member and block of a file with the bit position of
every block start.  The expected TEXT is never taken from here: it is zlib's."""
import functools
import gzip
import random
import struct
import zlib

import numpy as np

import bgzf_ref as B

NONE = (1 << 64) - 1
_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


# ---- the finder ------------------------------------------------------------------------------------------------------------
def _bits(data, pos, n):
    """n <= 57 bits from bit position pos, bits past the end read as 0"""
    b = pos >> 3
    return (int.from_bytes(data[b:b + 9], "little") >> (pos & 7)) & ((1 << n) - 1)


def header_ok(data, pos):
    """BFINAL = 0, BTYPE = 2, and a dynamic header that zlib's inflate takes: HLIT <= 286, HDIST <= 30, a complete code-length
    code, a run-length stream that neither starts with a repeat nor overruns, a code for 256, neither set over-subscribed, and
    an incomplete set only as a single code of length 1 (or no distance code at all).  Every bit must lie in the buffer"""
    total = 8 * len(data)
    if pos + 17 > total:
        return False
    v = _bits(data, pos, 17)
    if v & 7 != 4:
        return False
    hlit, hdist, hclen = ((v >> 3) & 31) + 257, ((v >> 8) & 31) + 1, ((v >> 13) & 15) + 4
    if hlit > 286 or hdist > 30:
        return False
    q = pos + 17
    if q + 3 * hclen > total:
        return False
    v = _bits(data, q, 57)
    cl = [0] * 19
    for i in range(hclen):
        cl[_ORDER[i]] = (v >> (3 * i)) & 7
    if sum(128 >> l for l in cl if l) != 128:
        return False
    q += 3 * hclen
    codes = {(c, l): s for s, (c, l) in B.canonical(cl).items()}
    lens = []
    while len(lens) < hlit + hdist:
        v = _bits(data, q, 16)
        c = 0
        for l in range(1, 8):
            c = c << 1 | (v & 1)
            v >>= 1
            if (c, l) in codes:
                break
        else:
            return False
        s = codes[(c, l)]
        q += l
        if q > total:
            return False
        if s < 16:
            lens.append(s)
            continue
        if s == 16 and not lens:
            return False
        eb = {16: 2, 17: 3, 18: 7}[s]
        rep = (11 if s == 18 else 3) + (v & ((1 << eb) - 1))
        q += eb
        if q > total:
            return False
        lens += [lens[-1] if s == 16 else 0] * rep
    if len(lens) > hlit + hdist or lens[256] == 0:
        return False
    for part in (lens[:hlit], lens[hlit:]):
        kraft, used = sum(32768 >> l for l in part if l), [l for l in part if l]
        if kraft > 32768 or (kraft < 32768 and used and max(used) > 1):
            return False
    return True


def find(data, chunk_bytes):
    """S_k per chunk: the lowest bit position inside chunk k >= 1 at which header_ok holds, or NONE; [0] is NONE"""
    n = len(data)
    nchunks = (n + chunk_bytes - 1) // chunk_bytes
    d = np.frombuffer(data + b"\0\0\0\0", dtype=np.uint8).astype(np.uint32)
    words = d[:n] | d[1:n + 1] << 8 | d[2:n + 2] << 16 | d[3:n + 3] << 24
    out = [NONE]
    for k in range(1, nchunks):
        lo, hi = k * chunk_bytes, min(n, (k + 1) * chunk_bytes)
        w, hits = words[lo:hi], []
        for s in range(8):       # the cheap part for every bit of the chunk at once: the three bits and the two ranges
            x = w >> s
            ok = ((x & 7) == 4) & (((x >> 3) & 31) <= 29) & (((x >> 8) & 31) <= 29)
            hits.append((np.nonzero(ok)[0] + lo) * 8 + s)
        found = NONE
        for pos in np.sort(np.concatenate(hits)):
            if header_ok(data, int(pos)):
                found = int(pos)
                break
        out.append(found)
    return out


# ---- the walk ----------------------------------------------------------------------------------------------------------------
def member_header(data, at):
    """the offset of the deflate data of the member whose header begins at `at`"""
    if data[at:at + 3] != b"\x1f\x8b\x08":
        raise ValueError("header")
    flg = data[at + 3]
    at += 10
    if flg & 4:
        at += 2 + struct.unpack_from("<H", data, at)[0]
    for bit in (8, 16):
        if flg & bit:
            at = data.index(b"\0", at) + 1
    if flg & 2:
        at += 2
    return at


def _table(lens):
    """(table, bits): table[the next `bits` bits] = symbol << 4 | length"""
    codes = B.canonical(lens)
    if not codes:
        return [], 0
    top = max(l for _, l in codes.values())
    table = [0] * (1 << top)
    for s, (c, l) in codes.items():
        r = int(format(c, "0%db" % l)[::-1], 2)
        table[r::1 << l] = [s << 4 | l] * (1 << (top - l))
    return table, top


_FIXED = None


def walk(data):
    """every member and block of a gzip file: (starts, members, text bytes); starts = [(bit position, BFINAL, BTYPE)].  Nothing
    is produced; the stream is taken as good (zlib has read it)"""
    global _FIXED
    if _FIXED is None:
        _FIXED = (_table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _table([5] * 32))
    starts, members, text, at, n = [], 0, 0, 0, len(data)
    get = lambda pos, k: (int.from_bytes(data[pos >> 3:(pos >> 3) + 8], "little") >> (pos & 7)) & ((1 << k) - 1)
    while at < n:
        pos = 8 * member_header(data, at)
        while True:
            hdr = get(pos, 3)
            starts.append((pos, hdr & 1, hdr >> 1))
            pos += 3
            if hdr >> 1 == 0:
                pos = (pos + 7) & ~7
                ln = get(pos, 16)
                pos += 32 + 8 * ln
                text += ln
            else:
                if hdr >> 1 == 1:
                    (lt, lb), (dt, db) = _FIXED
                else:
                    hlit, hdist, hclen = get(pos, 5) + 257, get(pos + 5, 5) + 1, get(pos + 10, 4) + 4
                    pos += 14
                    cl = [0] * 19
                    for i in range(hclen):
                        cl[_ORDER[i]] = get(pos, 3)
                        pos += 3
                    ct, cb = _table(cl)
                    lens = []
                    while len(lens) < hlit + hdist:
                        e = ct[get(pos, cb)]
                        pos += e & 15
                        s = e >> 4
                        if s < 16: lens.append(s)
                        elif s == 16: lens += [lens[-1]] * (3 + get(pos, 2)); pos += 2
                        elif s == 17: lens += [0] * (3 + get(pos, 3)); pos += 3
                        else: lens += [0] * (11 + get(pos, 7)); pos += 7
                    (lt, lb), (dt, db) = _table(lens[:hlit]), _table(lens[hlit:hlit + hdist])
                lmask, dmask = (1 << lb) - 1, (1 << db) - 1
                while True:   # (48 bits at a time: a length with its extra bits, a distance with its own)
                    v = int.from_bytes(data[pos >> 3:(pos >> 3) + 8], "little") >> (pos & 7)
                    e = lt[v & lmask]
                    s, l = e >> 4, e & 15
                    if s < 256:
                        pos += l
                        text += 1
                        continue
                    if s == 256:
                        pos += l
                        break
                    x = B._LEXT[s - 257]
                    text += B._LBASE[s - 257] + ((v >> l) & ((1 << x) - 1))
                    l += x
                    e = dt[(v >> l) & dmask]
                    pos += l + (e & 15) + B._DEXT[e >> 4]
            if hdr & 1:
                break
        at = ((pos + 7) >> 3) + 8
        members += 1
    return starts, members, text


# ---- the corpus ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fastq(n, seed):
    return B.fastq_text(n, seed)


def gz(text, level=6, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=None, flush_mode=zlib.Z_SYNC_FLUSH):
    c = zlib.compressobj(level, zlib.DEFLATED, 31, mem_level, strategy)
    if flush_every is None:
        return c.compress(text) + c.flush()
    out = b""
    for i in range(0, len(text), flush_every):
        out += c.compress(text[i:i + flush_every]) + c.flush(flush_mode)
    return out + c.flush()


def member(raw, text, flg=0, extra=b"", name=b"", comment=b""):
    """a gzip member by hand around a raw DEFLATE stream; flg chooses among FHCRC 2, FEXTRA 4, FNAME 8, FCOMMENT 16"""
    head = struct.pack("<4BI2B", 0x1f, 0x8b, 8, flg, 0, 0, 0xff)
    if flg & 4: head += struct.pack("<H", len(extra)) + extra
    if flg & 8: head += name + b"\0"
    if flg & 16: head += comment + b"\0"
    if flg & 2: head += struct.pack("<H", zlib.crc32(head) & 0xffff)
    return head + raw + struct.pack("<II", zlib.crc32(text) & 0xffffffff, len(text) & 0xffffffff)


def stored_payload():
    inner = B.deflate(fastq(200_000, 3), 6)
    return b">x\n" + b"A" * 20000 + inner + b"\n>y\nACGT\n"


LEVELS = {"fq_l1": 1, "fq_l6": 6, "fq_l9": 9}
MEMLEVELS = {"ml1_l6": (120_000, 6, 1, 1024), "ml1_l9": (120_000, 9, 1, 2048), "ml2_l1": (300_000, 1, 2, 4096)}
# what a restatement of the predicate gave on exactly these inputs when the row GZIP was specified: (chunks behind the first,
# chunks of them in which a true start is found); no false candidate in any
SPECIFIED = {"fq_l1": (24, 23), "fq_l6": (22, 21), "fq_l9": (22, 21), "ml1_l6": (68, 67), "ml1_l9": (33, 33), "ml2_l1": (42, 42)}


@functools.lru_cache(maxsize=None)
def corpus():
    """name -> (file, chunk size it is run at)"""
    K = 1024
    out = {}
    for name, level in LEVELS.items():
        out[name] = (gz(fastq(1_500_000, 7), level), 32 * K)
    for name, (n, level, ml, chunk) in MEMLEVELS.items():
        out[name] = (gz(fastq(n, 11), level, ml), chunk)
    out["stored_false"] = (gz(stored_payload(), 0), 16 * K)
    t = fastq(200_000, 5)
    out["fixed_only"] = (gz(t, 6, strategy=zlib.Z_FIXED), 16 * K)
    out["level0"] = (gz(fastq(300_000, 11), 0), 16 * K)
    out["huffman_only"] = (gz(t, 6, strategy=zlib.Z_HUFFMAN_ONLY), 16 * K)
    out["rle"] = (gz(t, 6, strategy=zlib.Z_RLE), 16 * K)
    out["sync_flush"] = (gz(t, 6, flush_every=10000), 4 * K)
    out["full_flush"] = (gz(t, 6, flush_every=10000, flush_mode=zlib.Z_FULL_FLUSH), 4 * K)
    fib = B.fibonacci_text()
    out["fibonacci"] = (gz(fib * 4, 9), 2 * K)
    raw, text = B.far_32768()
    out["far_32768"] = (member(raw, text), K)
    a, b, c = fastq(150_000, 21), B.fasta_text(120_000, 22), fastq(90_000, 23)
    out["three_members"] = (gz(a, 6) + gz(b, 9) + gz(c, 1), 8 * K)
    out["empty_between"] = (gz(a, 6) + gz(b"", 6) + gz(c, 6), 8 * K)
    out["header_fields"] = (member(B.deflate(a, 6), a, 2 | 4 | 8 | 16, extra=b"XY\x03\x00abc", name=b"reads.fq", comment=b"a comment") + gz(c, 6), 8 * K)
    out["bgzf_file"] = (B.write(fastq(400_000, 24)), 8 * K)
    out["empty_file"] = (gzip.compress(b""), K)
    return out


def expected(data):
    return gzip.decompress(data)


def reach_before_member():
    """two files whose SECOND member holds a match that reaches in front of its own start, where the first member's text would
    satisfy it.  `by_hand`: three literals, then length 3 at distance 4, assembled bit by bit.  `by_dictionary`: zlib wrote the
    second member's stream against a preset dictionary -- the last 32 KiB of the first member's text -- behind 16 KiB that do
    not compress, so that the far matches stand in a later block, which a later chunk decodes through markers.
    name -> (file, chunk size)"""
    first = fastq(100_000, 31)
    by_hand = gz(first, 6) + member(B.fixed_distance_too_far(), b"ACGGAC")
    r = random.Random(32)
    text = bytes(r.randrange(256) for _ in range(16384)) + first[-32768:] * 3
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, first[-32768:])
    by_dictionary = gz(first, 6) + member(c.compress(text) + c.flush(), text)
    return {"by_hand": (by_hand, 1024), "by_dictionary": (by_dictionary, 1024)}


def _flip(data, at, mask=1):
    return data[:at] + bytes([data[at] ^ mask]) + data[at + 1:]


def malformed():
    """name -> (file, chunk size, BSK_ERR_* code, words of the message)"""
    good, chunk = corpus()["fq_l6"]
    small = gz(fastq(90_000, 23), 6)
    out = {}
    out["flipped_bit"] = (_flip(good, 17 * chunk + chunk // 2), chunk, 3, "member 0 at offset")
    out["wrong_crc"] = (_flip(good, len(good) - 8), chunk, 3, "CRC mismatch")
    out["wrong_crc_first_of_two"] = (_flip(small, len(small) - 6) + small, 8192, 3, "member 0 at offset %d: CRC mismatch" % (len(small) - 8))
    out["wrong_isize"] = (_flip(good, len(good) - 4), chunk, 3, "ISIZE")
    out["truncated_in_block"] = (good[:len(good) // 2], chunk, 3, "truncated")
    out["truncated_in_trailer"] = (good[:-3], chunk, 3, "truncated")
    out["garbage_behind"] = (good + b"garbage!", chunk, 3, "not a gzip member header")
    out["zero_padding"] = (small + b"\0" * 512, 8192, 3, "member 1 at offset %d: the bytes after the last member" % len(small))
    out["too_many_members"] = (gz(b"", 6) * 65537, 64 * 1024, 4, "65537")
    return out
