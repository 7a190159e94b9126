"""BGZF restated for the tests (PARITY.md BGZF): a writer built on zlib's raw DEFLATE, a bit writer for the streams that
are assembled by hand, a small inflate that also REPORTS what a stream exercises, the corpus and the malformed inputs.
Nothing here is a test; tests/test_bgzf_cpu.py and tests/test_bgzf_gpu.py assert the reports, so that the corpus cannot
quietly cover less than it claims."""
import random
import struct
import zlib

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
MAX_BLOCK = 65280   # what bgzip puts into a block


def member(raw_deflate, text, extra_before=b"", extra_after=b""):
    """one BGZF block around a raw DEFLATE stream of `text`; extra_*: further subfields in front of / behind BC"""
    xlen = 6 + len(extra_before) + len(extra_after)
    bsize = 12 + xlen + len(raw_deflate) + 8
    assert bsize <= 65536, bsize
    head = struct.pack("<4BI2BH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, xlen)
    bc = b"BC" + struct.pack("<HH", 2, bsize - 1)
    return head + extra_before + bc + extra_after + raw_deflate + struct.pack("<II", zlib.crc32(text) & 0xffffffff, len(text))


def deflate(text, level=6, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None, flush_mode=zlib.Z_SYNC_FLUSH):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    if flush_at is None:
        return c.compress(text) + c.flush()
    return c.compress(text[:flush_at]) + c.flush(flush_mode) + c.compress(text[flush_at:]) + c.flush()


def write(text, block=MAX_BLOCK, eof=True, **kw):
    """`text` as a BGZF file: blocks of `block` text bytes"""
    out = [member(deflate(text[i:i + block], **kw), text[i:i + block]) for i in range(0, len(text), block)]
    return b"".join(out) + (EOF_BLOCK if eof else b"")


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, count):          # LSB first (header fields, extra bits)
        self.acc |= value << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, count):          # a Huffman code: MSB first
        for k in range(count - 1, -1, -1):
            self.bits((value >> k) & 1, 1)

    def fixed_lit(self, s):
        if s < 144: self.code(0x30 + s, 8)
        elif s < 256: self.code(0x190 + s - 144, 9)
        elif s < 280: self.code(s - 256, 7)
        else: self.code(0xc0 + s - 280, 8)

    def done(self):
        if self.n: self.bits(0, 8 - self.n)
        return bytes(self.out)


def canonical(lens):
    """code of every symbol with a length (RFC 1951 3.2.2)"""
    code, out = 0, {}
    for L in range(1, 16):
        for s, l in enumerate(lens):
            if l == L:
                out[s] = (code, L)
                code += 1
        code <<= 1
    return out


def dynamic_literals_one_distance(text):
    """a dynamic block of literals only whose distance code has ONE code, of length 1 (RFC 1951 3.2.7); every byte of `text`
    and the end-of-block code get 8 or 9 bits"""
    used = sorted(set(text)) + [256]
    assert 2 <= len(used) <= 256
    # a complete code: with n symbols, 2^k >= n: (2^k - n) symbols of k - 1 bits ... simpler: lengths 8 / 9 as a complete set
    n = len(used)
    k = max(1, (n - 1).bit_length())
    short = (1 << k) - n            # symbols with k - 1 bits
    lens = [0] * 257
    for i, s in enumerate(used):
        lens[s] = k - 1 if i < short else k
    if k - 1 == 0:
        lens[used[0]] = 1
    lit = canonical(lens)
    w = BitWriter()
    w.bits(1, 1); w.bits(2, 2)
    w.bits(0, 5); w.bits(0, 5); w.bits(15, 4)           # HLIT 257, HDIST 1, HCLEN 19
    # the code-length code: the lengths 0 .. 15 by 4 bits each (16 symbols of length 4 = complete), no repeat codes
    cl = [0] * 19
    for v in range(16): cl[v] = 4
    for at in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15): w.bits(cl[at], 3)
    clc = canonical(cl)
    for l in lens + [1]:                                # 257 literal/length lengths, then the one distance code: length 1
        w.code(*clc[l])
    for b in text: w.code(*lit[b])
    w.code(*lit[256])
    return w.done()


def fixed_distance_too_far():
    """a fixed-Huffman block: 3 literals, then a match of length 3 at distance 4 -- one byte before the start of the block"""
    w = BitWriter()
    w.bits(1, 1); w.bits(1, 2)
    for b in b"ACG": w.fixed_lit(b)
    w.fixed_lit(257)            # length 3
    w.code(3, 5)                # distance code 3 = distance 4
    w.fixed_lit(256)
    return w.done()


def oversubscribed_dynamic():
    """a dynamic header whose code-length code has three codes of length 1"""
    w = BitWriter()
    w.bits(1, 1); w.bits(2, 2)
    w.bits(0, 5); w.bits(0, 5); w.bits(0, 4)            # HCLEN 4: the lengths of 16, 17, 18, 0
    for v in (1, 1, 1, 0): w.bits(v, 3)
    w.bits(0, 32)
    return w.done()


# ---- inflate with a report ---------------------------------------------------------------------------------------------
class Report:
    def __init__(self):
        self.types, self.blocks_per_member = set(), []
        self.max_code_len = self.max_distance = self.max_match = 0
        self.repeat_codes = set()
        self.empty_stored = self.single_distance_code = self.stored_at_bit_offset = False


class _Bits:
    def __init__(self, data):
        self.d, self.pos = data, 0          # pos in bits

    def get(self, n):
        v = 0
        for k in range(n):
            if self.pos >> 3 >= len(self.d): raise ValueError("truncated")
            v |= ((self.d[self.pos >> 3] >> (self.pos & 7)) & 1) << k
            self.pos += 1
        return v


def _decoder(lens):
    codes = {(c, l): s for s, (c, l) in canonical(lens).items()}
    def dec(b, rep):
        c = 0
        for l in range(1, 16):
            c = c << 1 | b.get(1)
            if (c, l) in codes:
                rep.max_code_len = max(rep.max_code_len, l)
                return codes[(c, l)]
        raise ValueError("invalid code")
    return dec


_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


def inflate_raw(data, rep):
    b, out, nblocks = _Bits(data), bytearray(), 0
    while True:
        last, typ = b.get(1), b.get(2)
        nblocks += 1
        rep.types.add(typ)
        if typ == 0:
            if b.pos & 7: rep.stored_at_bit_offset = True
            b.pos = (b.pos + 7) & ~7
            ln, nl = b.get(16), b.get(16)
            if ln != (~nl & 0xffff): raise ValueError("stored")
            if ln == 0: rep.empty_stored = True
            at = b.pos >> 3
            if at + ln > len(data): raise ValueError("truncated")
            out += data[at:at + ln]
            b.pos += 8 * ln
        elif typ == 3:
            raise ValueError("block type")
        else:
            if typ == 1:
                ll, dl = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 32
            else:
                hlit, hdist, hclen = b.get(5) + 257, b.get(5) + 1, b.get(4) + 4
                cl = [0] * 19
                for at in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[:hclen]: cl[at] = b.get(3)
                cdec, scratch, lens = _decoder(cl), Report(), []
                while len(lens) < hlit + hdist:
                    s = cdec(b, scratch)
                    if s < 16: lens.append(s)
                    else:
                        rep.repeat_codes.add(s)
                        if s == 16: lens += [lens[-1]] * (3 + b.get(2))
                        elif s == 17: lens += [0] * (3 + b.get(3))
                        else: lens += [0] * (11 + b.get(7))
                ll, dl = lens[:hlit], lens[hlit:hlit + hdist]
                if sum(1 for l in dl if l) == 1: rep.single_distance_code = True
            ldec, ddec = _decoder(ll), _decoder(dl)
            while True:
                s = ldec(b, rep)
                if s < 256: out.append(s)
                elif s == 256: break
                else:
                    L = _LBASE[s - 257] + b.get(_LEXT[s - 257])
                    d = ddec(b, rep)
                    D = _DBASE[d] + b.get(_DEXT[d])
                    if D > len(out): raise ValueError("distance")
                    rep.max_distance, rep.max_match = max(rep.max_distance, D), max(rep.max_match, L)
                    for _ in range(L): out.append(out[-D])
        if last: break
    rep.blocks_per_member.append(nblocks)
    return bytes(out)


def index(data):
    """(offset, size, ISIZE) of every block, walking the chain from 0"""
    out, off = [], 0
    while off < len(data):
        xlen = struct.unpack_from("<H", data, off + 10)[0]
        at, bsize = off + 12, None
        while at < off + 12 + xlen:
            tag, slen = data[at:at + 2], struct.unpack_from("<H", data, at + 2)[0]
            if tag == b"BC" and slen == 2: bsize = struct.unpack_from("<H", data, at + 4)[0] + 1
            at += 4 + slen
        out.append((off, bsize, struct.unpack_from("<I", data, off + bsize - 4)[0], xlen))
        off += bsize
    return out


def inflate(data):
    """(text, Report) of a BGZF file"""
    rep, out = Report(), bytearray()
    for off, bsize, isize, xlen in index(data):
        # (the EOF block is a fixed block of nothing: it is decoded, but what it exercises is not the corpus member's)
        text = inflate_raw(data[off + 12 + xlen:off + bsize - 8], Report() if data[off:off + bsize] == EOF_BLOCK else rep)
        assert len(text) == isize and zlib.crc32(text) & 0xffffffff == struct.unpack_from("<I", data, off + bsize - 8)[0]
        out += text
    return bytes(out), rep


# ---- the texts -------------------------------------------------------------------------------------------------------------
def fastq_text(n_bytes, seed=1):
    r, out, i = random.Random(seed), [], 0
    while sum(map(len, out)) < n_bytes:
        seq = "".join(r.choice("ACGT") for _ in range(150))
        qual = "".join(chr(33 + min(40, max(2, int(r.gauss(32, 6))))) for _ in range(150))
        out.append("@read%d/1 lane=%d\n%s\n+\n%s\n" % (i, r.randrange(8), seq, qual))
        i += 1
    return "".join(out).encode()


def fasta_text(n_bytes, seed=2):
    r, out, i = random.Random(seed), [], 0
    while sum(map(len, out)) < n_bytes:
        seq = "".join(r.choice("ACGT") for _ in range(r.randrange(100, 2000)))
        out.append(">seq%d some description\n" % i + "".join(seq[k:k + 60] + "\n" for k in range(0, len(seq), 60)))
        i += 1
    return "".join(out).encode()


def fibonacci_text():
    """byte frequencies that follow the Fibonacci numbers over 40 symbols, shuffled: the deepest Huffman tree zlib builds"""
    fib, out = [1, 1], bytearray()
    while len(fib) < 40: fib.append(fib[-1] + fib[-2])
    scale = 60000 / sum(fib[:22])
    for s in range(22): out += bytes([48 + s]) * max(1, int(fib[s] * scale))
    for s in range(22, 40): out += bytes([48 + s])      # (the rare end of the sequence, once each)
    random.Random(3).shuffle(out)
    return bytes(out[:65000])


def far_text():
    r = random.Random(4)
    head = bytes(r.choice(b"ACGT") for _ in range(32500))   # (zlib looks back 32768 - 262 = 32506 bytes at the most)
    return head + head[:600]


def far_32768():
    """(stream, text) by hand: a stored block of 32768 bytes, then a fixed block with one match of length 258 at distance
    32768 -- the farthest and the longest the format has"""
    r = random.Random(7)
    head = bytes(r.choice(b"ACGT") for _ in range(32768))
    w = BitWriter()
    w.bits(1, 1); w.bits(1, 2)
    w.fixed_lit(285)                       # length 258
    w.code(29, 5); w.bits(8191, 13)        # distance 24577 + 8191
    w.fixed_lit(256)
    return b"\x00" + struct.pack("<HH", 32768, 32768 ^ 0xffff) + head + w.done(), head + head[:258]


HEADER_SIGNATURE = bytes.fromhex("1f8b08040000000000ff060042430200")


def corpus():
    """name -> BGZF file.  What each must exercise is asserted by the tests (EXPECT)"""
    fq, fa = fastq_text(120000), fasta_text(120000)
    C = {}
    for name, text in (("fq", fq), ("fa", fa)):
        for level in (0, 1, 6, 9): C["%s_l%d" % (name, level)] = write(text, level=level)
        C[name + "_fixed"] = write(text, strategy=zlib.Z_FIXED)
        C[name + "_huff"] = write(text, strategy=zlib.Z_HUFFMAN_ONLY)
        C[name + "_rle"] = write(text, strategy=zlib.Z_RLE)
        C[name + "_mem1"] = write(text, mem_level=1)
        C[name + "_sync"] = write(text, flush_at=20001, flush_mode=zlib.Z_SYNC_FLUSH)
        C[name + "_full"] = write(text, flush_at=20001, flush_mode=zlib.Z_FULL_FLUSH)
    C["run_A"] = write(b"A" * 60000)
    C["far"] = member(deflate(far_text(), level=9), far_text()) + EOF_BLOCK
    C["far_32768"] = member(*far_32768()) + EOF_BLOCK
    C["fibonacci"] = write(fibonacci_text(), block=65000, level=9)
    lit = bytes(random.Random(5).choice(b"ACGTN\n") for _ in range(3000))
    C["one_distance_code"] = member(dynamic_literals_one_distance(lit), lit) + EOF_BLOCK
    C["block_65536"] = write((fq * 2)[:65536], block=65536)
    C["stored_65280"] = write(random.Random(6).randbytes(65280), level=0)
    for n in (1, 2, 63, 64, 65): C["blocks_%d" % n] = write(fq[:10 * n], block=10)
    e = member(deflate(b""), b"")
    C["empty_blocks"] = e + e + member(deflate(fq[:1000]), fq[:1000]) + e + member(deflate(fq[1000:2000]), fq[1000:2000]) + e
    C["no_eof"] = write(fq[:70000], eof=False)
    C["eof_alone"] = EOF_BLOCK
    C["zero_bytes"] = b""
    t = fa[:5000]
    C["extra_subfields"] = member(deflate(t), t, extra_before=b"XY\x03\x00abc") + member(deflate(t), t, extra_after=b"ZZ\x00\x00") + EOF_BLOCK
    sig = fq[:3000] + HEADER_SIGNATURE + b"\x10\x00" + fq[3000:9000] + HEADER_SIGNATURE[:4] + fq[9000:12000]
    C["signature_in_stored"] = write(sig, level=0)
    return C


# what the corpus must exercise: name -> predicate on the Report
EXPECT = {
    "fq_l0": lambda r: r.types == {0}, "fa_l0": lambda r: r.types == {0},
    "fq_fixed": lambda r: r.types == {1}, "fa_fixed": lambda r: r.types == {1},
    "fq_l1": lambda r: 2 in r.types, "fq_l6": lambda r: 2 in r.types and bool(r.repeat_codes), "fq_l9": lambda r: 2 in r.types,
    "fa_l6": lambda r: 2 in r.types and {17, 18} <= r.repeat_codes,
    "fq_huff": lambda r: r.max_match == 0, "fq_rle": lambda r: r.max_distance == 1,
    "fq_mem1": lambda r: max(r.blocks_per_member) >= 8, "fa_mem1": lambda r: max(r.blocks_per_member) >= 8,
    "fq_sync": lambda r: r.empty_stored and r.stored_at_bit_offset, "fq_full": lambda r: r.empty_stored,
    "run_A": lambda r: r.max_distance == 1 and r.max_match == 258,
    "far": lambda r: r.max_distance >= 32000,          # zlib here: 32500, the distance of the copy
    "far_32768": lambda r: r.max_distance == 32768 and r.max_match == 258,
    "fibonacci": lambda r: r.max_code_len >= 13,       # zlib here: 14
    "one_distance_code": lambda r: r.single_distance_code and r.max_match == 0,
    "signature_in_stored": lambda r: r.types == {0},
}


def _patch(data, at, value):
    return data[:at] + value + data[at + len(value):]


def malformed():
    """name -> (file, BSK error code, block index or None, word of the reason).  Each is a good file with one thing wrong"""
    FORMAT, UNSUPPORTED = 3, 4
    fq = fastq_text(9000, seed=9)
    t0, t1 = fq[:4000], fq[4000:8000]
    b0, b1 = member(deflate(t0), t0), member(deflate(t1), t1)
    good = b0 + b1 + EOF_BLOCK
    n0, n1 = len(b0), len(b1)
    M = {}
    M["truncated_in_block"] = (good[:n0 + n1 // 2], FORMAT, 1, "truncated")
    M["bsize_past_end"] = (_patch(good, n0 + n1 + 16, struct.pack("<H", 999)), FORMAT, 2, "truncated")
    M["isize_small"] = (_patch(good, n0 + n1 - 4, struct.pack("<I", 3999)), FORMAT, 1, "overrun")
    M["isize_large"] = (_patch(good, n0 + n1 - 4, struct.pack("<I", 4001)), FORMAT, 1, "short")
    M["isize_65537"] = (_patch(good, n0 + n1 - 4, struct.pack("<I", 65537)), FORMAT, 1, "65536")
    M["crc_bit"] = (_patch(good, n0 + n1 - 8, bytes([good[n0 + n1 - 8] ^ 4])), FORMAT, 1, "CRC")
    M["data_bit"] = (_patch(good, n0 + 18 + 700, bytes([good[n0 + 18 + 700] ^ 16])), FORMAT, 1, "")
    M["btype3"] = (b0 + member(b"\x07" + bytes(8), t1) + EOF_BLOCK, FORMAT, 1, "block type")
    M["stored_nlen"] = (b0 + member(b"\x01\x04\x00\xfa\xff" + t1[:4], t1[:4]) + EOF_BLOCK, FORMAT, 1, "NLEN")
    M["oversubscribed"] = (b0 + member(oversubscribed_dynamic(), t1) + EOF_BLOCK, FORMAT, 1, "code lengths")
    M["distance_too_far"] = (b0 + member(fixed_distance_too_far(), b"ACGCGT"[:6]) + EOF_BLOCK, FORMAT, 1, "distance")
    M["garbage_after"] = (good + b"garbage after the last block", FORMAT, 3, "not a block header")
    import gzip
    M["plain_gzip"] = (gzip.compress(fq), UNSUPPORTED, None, "bgzip")
    return M, good, t0 + t1
