// One DEFLATE (RFC 1951) decoder for one BGZF block, the same source for the kernel (ops_bgzf.hip, one block per wavefront)
// and for the host (bsk_bgzf_inflate_host, tests/host_c/bgzf_host_check.cpp).  PARITY.md BGZF: zlib defines the bytes.
//
// The decoder is written for L lanes that run it in lockstep with the SAME values (the symbol decode is uniform); the lanes
// differ only where they share out work: the copies, the table fills, the CRC.  A policy P says what a lane is:
//     P::LANES            lanes that run the decoder together (64 on the device, 1 on the host)
//     P::CRC_CHUNK        bytes of a CRC chunk; LANES * CRC_CHUNK >= 65536, the largest ISIZE
//     lane()              this lane, 0 .. LANES-1
//     sync()              what one lane wrote to BgzfLds is visible to the others behind it
//     uni(v)              v, which is the same in every lane, as a value the compiler knows to be the same (scalar registers)
//     word(w)             the 32-bit little-endian word w of the compressed bytes, bytes [4w, 4w + 4); bytes past the end of the
//                         buffer read as 0.  The same w in every lane.  Positions count from a base in front of the block that
//                         the policy chooses (32 bits hold them: a block is at most 64 KiB)
//     in_byte(a)          byte a, from the same base; a differs between lanes; the decoder has bounded it
//     shfl(v, k)          lane k's v
//     store(ring, a, b)   output bytes [a, b) of this block, which lie in the ring at ring_at(a) .., go to the output
// What the decoder trusts: nothing.  Every compressed bit it consumes is counted against the block's data range (`left`), every
// output byte against ISIZE before it is written, every distance against the bytes produced so far, every code-length set is
// checked for over-subscription, an incomplete set is taken only where zlib takes it (see build()), and every pass of every
// loop consumes at least one bit or ends with an error -- it cannot spin on a bad code.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define BGZF_HD __host__ __device__ __forceinline__
#else
#define BGZF_HD inline
#endif

namespace bsk {
namespace bgzf {

enum : int {
    OK = 0,
    ERR_TRUNCATED = 1,      // the compressed data of the block ends inside a symbol
    ERR_BLOCK_TYPE = 2,     // BTYPE 3
    ERR_STORED_LEN = 3,     // a stored block whose NLEN is not ~LEN
    ERR_CODE_LENGTHS = 4,   // over-subscribed or incomplete code lengths, too many codes, a bad repeat, no end-of-block code
    ERR_INVALID_CODE = 5,   // a bit pattern that is no code of the table, or a length / distance symbol that does not exist
    ERR_DISTANCE = 6,       // a distance that reaches before the start of the block
    ERR_OVERRUN = 7,        // more output than ISIZE
    ERR_SHORT = 8,          // less output than ISIZE
    ERR_CRC = 9,            // the CRC32 of the output is not the one in the trailer
    ERR_ISIZE = 10,         // ISIZE > 65536 (checked before anything is decoded)
    ERR_COUNT = 11
};

BGZF_HD const char* error_text(int code) {
    switch (code) {
        case OK: return "ok";
        case ERR_TRUNCATED: return "truncated: the compressed data ends inside the block";
        case ERR_BLOCK_TYPE: return "bad block type (BTYPE 3)";
        case ERR_STORED_LEN: return "stored block: LEN and NLEN do not match";
        case ERR_CODE_LENGTHS: return "bad code lengths";
        case ERR_INVALID_CODE: return "invalid code";
        case ERR_DISTANCE: return "distance too far back";
        case ERR_OVERRUN: return "output overrun: more bytes than ISIZE";
        case ERR_SHORT: return "output short: fewer bytes than ISIZE";
        case ERR_CRC: return "CRC mismatch";
        case ERR_ISIZE: return "ISIZE above 65536";
    }
    return "unknown error";
}

constexpr uint32_t RING = 32768, RING_MASK = RING - 1;
constexpr uint32_t LIT_ROOT = 10, DIST_ROOT = 8;
constexpr uint32_t MAX_ISIZE = 65536;
constexpr uint32_t DRAIN_AT = 16384;   // bytes that wait in the ring before they are stored (and their CRC taken)

// What a block's lanes share: on the device this is the wave's LDS (37 504 bytes: four waves per CU)
struct BgzfLds {
    alignas(16) uint8_t ring[RING];       // the window; output byte q of the block lies at ring_at(q)
    uint16_t lit_fast[1u << LIT_ROOT];    // first level: (symbol << 4) | length for codes of <= LIT_ROOT bits, else 0
    uint16_t dist_fast[1u << DIST_ROOT];
    uint16_t lit_count[16], lit_sym[288]; // second level: the canonical code, codes per length and symbols in code order
    uint16_t dist_count[16], dist_sym[32];  // (also the code-length code while a dynamic header is read)
    uint8_t lens[320];
    uint32_t crc_tab[256];
    uint32_t crc_mat[32];                 // CRC32 advanced by CRC_CHUNK zero bytes
};

// ---- CRC32 (the gzip polynomial, reflected)
BGZF_HD uint32_t crc_table_entry(uint32_t i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    return c;
}
BGZF_HD uint32_t crc_mat_times(const uint32_t* mat, uint32_t v) {
    uint32_t s = 0;
    for (int i = 0; i < 32; ++i) s ^= ((v >> i) & 1u) ? mat[i] : 0u;
    return s;
}
// the operator "append `bytes` zero bytes" (bytes a power of two), as zlib's crc32_combine builds it: the operator of one zero bit,
// squared until it spans the length
inline void crc_advance_matrix(uint32_t mat[32], uint32_t bytes) {
    uint32_t a[32], b[32];
    a[0] = 0xEDB88320u;
    for (int n = 1; n < 32; ++n) a[n] = 1u << (n - 1);
    for (uint64_t bits = 1; bits < 8ull * bytes; bits <<= 1) {
        for (int n = 0; n < 32; ++n) b[n] = crc_mat_times(a, a[n]);
        for (int n = 0; n < 32; ++n) a[n] = b[n];
    }
    for (int n = 0; n < 32; ++n) mat[n] = a[n];
}
// the CRC of a text from the CRCs of its chunks, chunk 0 being the LAST one: every chunk but the first of the text (the highest
// index, which may be short) is `CRC_CHUNK` bytes long, so one operator serves every step and the first chunk needs none
template <class Get>
BGZF_HD uint32_t crc_fold(const uint32_t* mat, uint32_t nchunks, Get chunk_crc) {
    if (nchunks == 0) return 0;
    uint32_t acc = chunk_crc(nchunks - 1);
    for (uint32_t k = nchunks - 1; k-- > 0;) acc = crc_mat_times(mat, acc) ^ chunk_crc(k);
    return acc;
}

// ---- canonical Huffman code, a bit at a time: `bits` holds the code from bit 0 on.  (symbol | length << 16), or -1 when no code
// of <= maxlen bits matches
BGZF_HD int huff_walk(const uint16_t* count, const uint16_t* symtab, uint32_t bits, int maxlen) {
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= maxlen; ++len) {
        code |= (int)(bits & 1u);
        bits >>= 1;
        const int cnt = count[len];
        if (code - cnt < first) return (int)symtab[index + (code - first)] | (len << 16);
        index += cnt;
        first += cnt;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

// What every decoder of this family shares: the bit reader, the tables of a block and the decode of one symbol.  L is what the
// lanes share (BgzfLds, or another struct with the same table members), Pos the type that counts compressed words and bits: 32
// bits for a BGZF block, 64 for a gzip stream of any length (gzip_spec_dev.hpp).
template <class P, class L, class Pos>
struct HuffCore {
    P& io;
    L& S;
    // the bit reader: `buf` holds `cnt` bits, `wnext` is the next word of the compressed buffer, `left` the bits of the
    // data that are not consumed yet (those in `buf` included; what `buf` holds beyond them is never consumed)
    uint64_t buf = 0;
    Pos wnext = 0, left = 0;
    uint32_t cnt = 0;
    Pos in_end = 0;
    bool fixed_ready = false;

    BGZF_HD HuffCore(P& io_, L& S_) : io(io_), S(S_) {}

    BGZF_HD void seek(Pos byte) {
        wnext = byte >> 2;
        const uint32_t skip = (uint32_t)(byte & 3u) * 8u;
        buf = (uint64_t)(io.word(wnext++) >> skip);
        cnt = 32u - skip;
        left = (in_end - byte) * 8u;
    }
    BGZF_HD void need32() {  // at least 32 bits in buf
        if (cnt < 32u) {
            buf |= (uint64_t)io.word(wnext++) << cnt;
            cnt += 32u;
        }
    }
    BGZF_HD bool drop(uint32_t n) {  // n <= cnt
        if (n > left) return false;
        buf >>= n;
        cnt -= n;
        left -= n;
        return true;
    }
    BGZF_HD uint32_t peek(uint32_t n) const { return (uint32_t)buf & ((1u << n) - 1u); }

    // The tables of one code from lens[0, n).  kind 0: the code-length code, 1: literal/length, 2: distance.  What zlib's
    // inflate_table takes and refuses: an over-subscribed set is refused; an incomplete one is refused for the code-length code
    // and for any code with a length above 1, so the ONE incomplete set that passes is a single code of length 1 (RFC 1951
    // 3.2.7: "one distance code"), and a set with no code at all passes too (a block of literals only): using a code that does
    // not exist is then ERR_INVALID_CODE.
    BGZF_HD int build(const uint8_t* lens, uint32_t n, uint16_t* count, uint16_t* symtab, uint16_t* fast, uint32_t root, int kind) {
        const uint32_t l = io.lane();
        // lane L < 16 counts the codes of length L ...
        for (uint32_t len = l; len < 16u; len += P::LANES) {
            uint32_t c = 0;
            for (uint32_t s = 0; s < n; ++s) c += lens[s] == len ? 1u : 0u;
            count[len] = (uint16_t)c;
        }
        io.sync();
        int room = 1;
        uint32_t maxlen = 0;
        for (uint32_t len = 1; len < 16u; ++len) {
            const uint32_t c = io.uni(count[len]);
            room = 2 * room - (int)c;
            if (room < 0) return ERR_CODE_LENGTHS;
            if (c) maxlen = len;
        }
        if (room > 0 && maxlen != 0 && (kind == 0 || maxlen > 1)) return ERR_CODE_LENGTHS;
        if (maxlen == 0 && kind == 0) return ERR_CODE_LENGTHS;
        // ... and puts their symbols, in symbol order, behind those of the shorter codes (length 0 is no code: nothing to put)
        for (uint32_t len = l; len < 16u; len += P::LANES) {
            uint32_t at = 0;
            for (uint32_t k = 1; k < len; ++k) at += count[k];
            const uint32_t ns = len ? n : 0u;
            for (uint32_t s = 0; s < ns; ++s)
                if (lens[s] == len) symtab[at++] = (uint16_t)s;
        }
        io.sync();
        if (root) {
            for (uint32_t i = l; i < (1u << root); i += P::LANES) {
                const int r = huff_walk(count, symtab, i, (int)root);
                fast[i] = r < 0 ? (uint16_t)0 : (uint16_t)(((r & 0xFFFF) << 4) | (r >> 16));
            }
            io.sync();
        }
        return OK;
    }

    // a symbol of the code (fast, count, symtab): its value, or -ERR_*
    BGZF_HD int symbol(const uint16_t* fast, uint32_t root, const uint16_t* count, const uint16_t* symtab) {
        need32();
        const uint32_t e = io.uni(fast[peek(root)]);
        uint32_t sym, len;
        if (e & 15u) {
            sym = e >> 4;
            len = e & 15u;
        } else {
            const int r = (int)io.uni((uint32_t)huff_walk(count, symtab, (uint32_t)buf, 15));
            if (r < 0) return left < 15u ? -ERR_TRUNCATED : -ERR_INVALID_CODE;
            sym = (uint32_t)r & 0xFFFFu;
            len = (uint32_t)r >> 16;
        }
        if (!drop(len)) return -ERR_TRUNCATED;
        return (int)sym;
    }

    // the code lengths of a dynamic block through the code-length code (in dist_count / dist_sym) into lens[0, total)
    BGZF_HD int read_lengths(uint32_t total) {
        const uint32_t l = io.lane();
        uint32_t i = 0, prev = 0, have256 = 0;
        while (i < total) {
            need32();
            const int r = (int)io.uni((uint32_t)huff_walk(S.dist_count, S.dist_sym, (uint32_t)buf, 7));
            if (r < 0) return left < 7u ? ERR_TRUNCATED : ERR_CODE_LENGTHS;
            if (!drop((uint32_t)r >> 16)) return ERR_TRUNCATED;
            const uint32_t sym = (uint32_t)r & 0xFFFFu;
            uint32_t rep = 1, val = sym;
            if (sym >= 16u) {
                if (sym == 16u && i == 0) return ERR_CODE_LENGTHS;
                const uint32_t eb = sym == 16u ? 2u : sym == 17u ? 3u : 7u;
                val = sym == 16u ? prev : 0u;
                rep = (sym == 18u ? 11u : 3u) + peek(eb);
                if (!drop(eb)) return ERR_TRUNCATED;
            }
            if (i + rep > total) return ERR_CODE_LENGTHS;
            if (val && i <= 256u && 256u < i + rep) have256 = 1;
            for (uint32_t k = l; k < rep; k += P::LANES) S.lens[i + k] = (uint8_t)val;
            i += rep;
            prev = val;
        }
        io.sync();
        return have256 ? OK : ERR_CODE_LENGTHS;  // (no end-of-block code)
    }

    // the tables of a block of type 1 (fixed) or 2 (dynamic).  One loop builds every code -- stage 0: the code-length code of a
    // dynamic block, 1: literal/length, 2: distance -- so that build() stands in the kernel once
    BGZF_HD int tables(uint32_t type) {
        const uint32_t l = io.lane();
        uint32_t hlit = 288u, hdist = 32u, stage = 1;
        if (type == 1u) {
            if (fixed_ready) return OK;
            for (uint32_t s = l; s < 320u; s += P::LANES) S.lens[s] = (uint8_t)(s < 144u ? 8 : s < 256u ? 9 : s < 280u ? 7 : s < 288u ? 8 : 5);
        } else {
            fixed_ready = false;
            need32();
            hlit = peek(5) + 257u;
            hdist = ((uint32_t)(buf >> 5) & 31u) + 1u;
            const uint32_t hclen = ((uint32_t)(buf >> 10) & 15u) + 4u;
            if (!drop(14)) return ERR_TRUNCATED;
            if (hlit > 286u || hdist > 30u) return ERR_CODE_LENGTHS;
            for (uint32_t i = l; i < 64u; i += P::LANES) S.lens[i] = 0;  // (the 19 of the code-length code, and what every lane can reach)
            io.sync();
            // (the order of the code-length code's lengths, RFC 1951 3.2.7, five bits each)
            const uint64_t order_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
            const uint64_t order_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
            for (uint32_t i = 0; i < hclen; ++i) {
                need32();
                const uint32_t v = peek(3);
                if (!drop(3)) return ERR_TRUNCATED;
                const uint32_t at = (uint32_t)((i < 12u ? order_lo >> (5u * i) : order_hi >> (5u * (i - 12u))) & 31u);
                if (l == 0) S.lens[at] = (uint8_t)v;
            }
            stage = 0;
        }
        io.sync();
        for (; stage < 3u; ++stage) {
            const bool lit = stage == 1u;
            const int rc = build(stage == 2u ? S.lens + hlit : S.lens, stage == 0u ? 19u : lit ? hlit : hdist, lit ? S.lit_count : S.dist_count,
                                 lit ? S.lit_sym : S.dist_sym, lit ? S.lit_fast : S.dist_fast, stage == 0u ? 0u : lit ? LIT_ROOT : DIST_ROOT, (int)stage);
            if (rc) return rc;
            if (stage == 0u) {
                const int e = read_lengths(hlit + hdist);
                if (e) return e;
            }
        }
        fixed_ready = type == 1u;
        return OK;
    }
};

template <class P>
struct Inflater : HuffCore<P, BgzfLds, uint32_t> {
    using Core = HuffCore<P, BgzfLds, uint32_t>;
    using Core::io; using Core::S; using Core::buf; using Core::wnext; using Core::left; using Core::cnt; using Core::in_end;
    using Core::seek; using Core::need32; using Core::drop; using Core::peek; using Core::symbol; using Core::tables;
    // the output: p bytes produced, f of them stored; ring_at(q) = (shift + q) & RING_MASK
    uint32_t p = 0, f = 0, isize = 0, shift = 0;
    uint32_t nlit = 0, mylit = 0;   // literals that wait in the lanes' registers, lane k holds literal k
    uint32_t crc = 0xFFFFFFFFu;     // of this lane's chunk

    BGZF_HD Inflater(P& io_, BgzfLds& S_) : Core(io_, S_) {}

    BGZF_HD uint32_t ring_at(uint32_t q) const { return (shift + q) & RING_MASK; }

    // bytes [a, b) leave the ring: every lane takes the CRC of what is its chunk's, then they are stored
    BGZF_HD void drain(uint32_t a, uint32_t b) {
        const uint32_t l = io.lane();
        const uint64_t back = (uint64_t)l * P::CRC_CHUNK;
        if (back < isize) {
            const uint32_t ce = isize - (uint32_t)back, cs = ce > P::CRC_CHUNK ? ce - P::CRC_CHUNK : 0u;
            const uint32_t q0 = a > cs ? a : cs, q1 = b < ce ? b : ce;
            uint32_t c = crc;
            for (uint32_t q = q0; q < q1; ++q) c = S.crc_tab[(c ^ S.ring[ring_at(q)]) & 255u] ^ (c >> 8);
            crc = c;
        }
        io.store(S.ring, shift, a, b);
        f = b;
    }
    // after every step that produced bytes: at most DRAIN_AT + 4096 + 15 < RING bytes ever wait
    BGZF_HD void maybe_drain() {
        if (p - f >= DRAIN_AT) drain(f, p - ((shift + p) & 15u));  // (up to a 16-byte boundary of the output)
    }
    BGZF_HD void flush_lits() {
        if (nlit) {
            if (io.lane() < nlit) S.ring[ring_at(p + io.lane())] = (uint8_t)mylit;
            p += nlit;
            nlit = 0;
            io.sync();
            maybe_drain();
        }
    }

    BGZF_HD int read_stored() {
        if (!drop(cnt & 7u)) return ERR_TRUNCATED;
        need32();
        const uint32_t len = peek(16), nlen = (uint32_t)(buf >> 16) & 0xFFFFu;
        if (!drop(32)) return ERR_TRUNCATED;
        if (len != (~nlen & 0xFFFFu)) return ERR_STORED_LEN;
        if (len * 8u > left) return ERR_TRUNCATED;
        if (len > isize - p) return ERR_OVERRUN;
        const uint32_t src = in_end - left / 8u;
        for (uint32_t done = 0; done < len;) {
            const uint32_t m = len - done < 4096u ? len - done : 4096u;
            for (uint32_t i = io.lane(); i < m; i += P::LANES) S.ring[ring_at(p + i)] = io.in_byte(src + done + i);
            p += m;
            done += m;
            io.sync();
            maybe_drain();
        }
        seek(src + len);
        return OK;
    }

    BGZF_HD int read_codes() {
        const uint32_t l = io.lane();
        for (;;) {
            int r = symbol(S.lit_fast, LIT_ROOT, S.lit_count, S.lit_sym);
            if (r < 0) return -r;
            uint32_t sym = (uint32_t)r;
            if (sym < 256u) {
                if (p + nlit >= isize) return ERR_OVERRUN;
                if (l == nlit) mylit = sym;
                if (++nlit == P::LANES) flush_lits();
                continue;
            }
            if (sym == 256u) return OK;
            if (sym > 285u) return ERR_INVALID_CODE;
            flush_lits();
            uint32_t L, eb;
            if (sym < 265u) { L = sym - 254u; eb = 0; }
            else if (sym == 285u) { L = 258u; eb = 0; }
            else { const uint32_t s = sym - 261u; eb = s >> 2; L = ((4u + (s & 3u)) << eb) + 3u; }
            L += peek(eb);
            if (!drop(eb)) return ERR_TRUNCATED;
            r = symbol(S.dist_fast, DIST_ROOT, S.dist_count, S.dist_sym);
            if (r < 0) return -r;
            sym = (uint32_t)r;
            if (sym > 29u) return ERR_INVALID_CODE;
            uint32_t D;
            if (sym < 4u) { D = sym + 1u; eb = 0; }
            else { eb = (sym >> 1) - 1u; D = ((2u + (sym & 1u)) << eb) + 1u; }
            D += peek(eb);
            if (!drop(eb)) return ERR_TRUNCATED;
            if (D > p) return ERR_DISTANCE;
            if (L > isize - p) return ERR_OVERRUN;
            // lane i writes byte p + i from p - D + (i mod D): every source byte lies in front of p
            for (uint32_t i = l; i < L; i += P::LANES) S.ring[ring_at(p + i)] = S.ring[ring_at(p - D + (i < D ? i : i % D))];
            p += L;
            io.sync();
            maybe_drain();
        }
    }

    // data = bytes [in_begin, in_end_) from the policy's base (the block without its header and its 8-byte trailer); the
    // output is `isize_` bytes at out_shift modulo 16 (the ring is laid out so that 16-byte pieces of it are 16-byte pieces of
    // the output)
    BGZF_HD int run(uint32_t in_begin, uint32_t in_end_, uint32_t isize_, uint32_t want_crc, uint32_t out_shift) {
        if (isize_ > MAX_ISIZE) return ERR_ISIZE;
        in_end = in_end_;
        isize = isize_;
        shift = out_shift & 15u;
        for (uint32_t i = io.lane(); i < 256u; i += P::LANES) S.crc_tab[i] = crc_table_entry(i);
        io.sync();
        seek(in_begin);
        for (;;) {
            need32();
            const uint32_t last = peek(1), type = (uint32_t)(buf >> 1) & 3u;
            if (!drop(3)) return ERR_TRUNCATED;
            int rc;
            if (type == 0u) rc = read_stored();
            else if (type == 3u) rc = ERR_BLOCK_TYPE;
            else {
                rc = tables(type);
                if (rc == OK) rc = read_codes();
                if (rc == OK) flush_lits();
            }
            if (rc) return rc;
            if (last) break;
        }
        if (p != isize) return ERR_SHORT;
        drain(f, p);
        const uint32_t mine = ~crc;
        const uint32_t nchunks = (isize + P::CRC_CHUNK - 1u) / P::CRC_CHUNK;
        const uint32_t got = crc_fold(S.crc_mat, nchunks, [&](uint32_t k) { return io.uni(io.shfl(mine, k)); });
        return got == want_crc ? OK : ERR_CRC;
    }
};

// ---- the host's lane: one lane, one chunk
struct HostLane {
    static constexpr uint32_t LANES = 1, CRC_CHUNK = 65536;
    const uint8_t* comp;  // the block
    uint64_t n;           // from the block to the end of the buffer
    uint8_t* out;         // this block's output
    uint32_t lane() const { return 0; }
    void sync() const {}
    uint32_t uni(uint32_t v) const { return v; }
    uint32_t word(uint32_t w) const {
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; ++k)
            if (4ull * w + k < n) v |= (uint32_t)comp[4ull * w + k] << (8 * k);
        return v;
    }
    uint8_t in_byte(uint32_t a) const { return comp[a]; }
    uint32_t shfl(uint32_t v, uint32_t) const { return v; }
    void store(const uint8_t* ring, uint32_t shift, uint32_t a, uint32_t b) const {
        for (uint32_t q = a; q < b; ++q) out[q] = ring[(shift + q) & RING_MASK];
    }
};

// ---- the frame of a block (RFC 1952 + the BGZF subfield)
struct BlockHeader {
    uint32_t bsize;   // the whole block, header and trailer included
    uint32_t xlen;
};
// 0: not gzip; 1: a BGZF header (h.bsize, h.xlen set); 2: gzip that is not BGZF; -1: the bytes end inside the header (n < 12 + XLEN)
inline int parse_header(const uint8_t* b, uint64_t n, BlockHeader* h) {
    if (n < 2 || b[0] != 0x1f || b[1] != 0x8b) return 0;
    if (n < 4) return 2;
    if (b[2] != 8 || !(b[3] & 4)) return 2;
    if (n < 12) return -1;
    const uint32_t xlen = b[10] | (uint32_t)b[11] << 8;
    if (n < 12ull + xlen) return -1;
    for (uint32_t at = 0; at + 4 <= xlen;) {
        const uint8_t* s = b + 12 + at;
        const uint32_t slen = s[2] | (uint32_t)s[3] << 8;
        if (at + 4 + slen > xlen) break;
        if (s[0] == 'B' && s[1] == 'C' && slen == 2) {
            h->bsize = (s[4] | (uint32_t)s[5] << 8) + 1u;
            h->xlen = xlen;
            return 1;
        }
        at += 4 + slen;
    }
    return 2;
}

}  // namespace bgzf
}  // namespace bsk
