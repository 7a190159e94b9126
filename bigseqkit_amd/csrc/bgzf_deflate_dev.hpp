// One DEFLATE (RFC 1951) encoder for one BGZF block, the same source for the kernel (ops_bgzf_write.hip, one block per
// wavefront) and for the host (bsk_bgzf_deflate_host, tests/host_c/bgzf_deflate_check.cpp).  PARITY.md BGZFW: zlib judges
// the bytes, and the bytes do not depend on the number of lanes -- every step below is defined over POSITIONS of the block.
//
// The block (n <= 65 280 bytes of text) becomes one gzip member: the 18-byte BGZF header, a raw DEFLATE stream of ONE
// block, CRC32 and ISIZE.
//   tokens    positions are taken in groups of 64.  Every position q of a group with four bytes in front of it hashes them
//             and looks at two candidates: the position the hash table held for that hash BEFORE the group (the highest
//             earlier position of that hash, at most 32 768 back) and q - 1 (a run).  The longer match wins, q - 1 on a tie;
//             fewer than MIN_MATCH bytes is no match.  Then all 64 positions enter the table (the highest position of a hash
//             stays).  A greedy pass from the first position no earlier match covers takes match or literal, left to right.
//   codes     the histogram of the tokens -> Huffman lengths (Moffat-Katajainen in place over the sorted counts, then the
//             lengths above the limit are folded back until the Kraft sum is 1), 15 bits for literal/length and distance, 7
//             for the code-length code over the run-length symbols 16-18
//   form      the bit cost of dynamic, fixed and stored is counted exactly; the cheapest in BYTES is written, stored before
//             fixed before dynamic on a tie.  So a member is never longer than its text + 31 bytes
// A policy P says what a lane is (LANES = 64 on the device, 1 on the host):
//     lane() sync() uni(v) shfl(v, k)   as in bgzf_inflate_dev.hpp;  CRC_CHUNK as there
//     for64(f)          f(k) for every k in 0..63: lane k on the device, a loop on the host
//     ballot64(f)       bit k = f(k)
//     scan64(a)         a[0..64) becomes its exclusive prefix sum; returns the total
//     reduce_add(v)     the sum of v over the lanes, the same in every lane
//     add(p, v) or32(p, v) max32(p, v)   *p += v, |= v, = max(*p, v) on a word the lanes share
//     text8(q) text32(q)   byte q / the little-endian word at byte q (any alignment) of the block's text; the encoder has
//                          bounded q (q + 4 <= n for text32)
//     tok(i, t) tok_at(i)   write / read token i of the block (room for n + 1)
//     out8(a, v) out32(w, v)   byte a / the aligned word w of the member's slot (room for n + 31 bytes rounded up to a word)
// In the stretches that cannot be shared out (the tree, the run-length pass) every lane computes the same values and writes
// the same words: no lane ever reads what another lane has not written identically.
// Every loop is bounded by the block: by n, by the 64 positions of a group, by the number of symbols or by the Kraft sum.
#pragma once
#include <cstdint>

#include "bgzf_inflate_dev.hpp"

#if defined(__clang__)
#define BGZF_NO_UNROLL _Pragma("clang loop unroll(disable)")
#else
#define BGZF_NO_UNROLL
#endif

namespace bsk {
namespace bgzf {

constexpr uint32_t BLOCK_TEXT = 0xff00;    // bgzip's choice: a stored block of it fits 65 536
constexpr uint32_t MEMBER_EXTRA = 31;      // header 18 + stored block 5 + trailer 8
constexpr uint32_t HASH_BITS = 13;
constexpr uint32_t MIN_MATCH = 4, MAX_MATCH = 258, MAX_DIST = 32768;
constexpr uint32_t FAR_DIST = 4096, FAR_MIN_MATCH = 6;   // a short match far back costs more bits than its literals
constexpr uint32_t OBUF_WORDS = 100;       // 31 bits that wait + 64 items of at most 48 bits, and two words of reach
constexpr uint32_t NO_HASH = 0xFFFFFFFFu;
constexpr uint32_t EOF_BYTES = 28;

BGZF_HD uint8_t eof_byte(uint32_t i) {     // the empty block bgzip ends a file with
    return i == 0 ? 0x1f : i == 1 ? 0x8b : i == 2 ? 8 : i == 3 ? 4 : i == 9 ? 0xff : i == 10 ? 6 : i == 12 ? 0x42 : i == 13 ? 0x43
         : i == 14 ? 2 : i == 16 ? 0x1b : i == 18 ? 3 : 0;
}

// What a block's lanes share: on the device this is the wave's LDS
struct DeflateLds {
    uint32_t head[1u << HASH_BITS];        // hash -> highest position with that hash + 1, 0: none
    uint32_t lit_freq[288], dist_freq[32], cl_freq[20];
    uint32_t key[288];                     // the sorted counts, then the tree, then the depths
    uint16_t sym[288];                     // ... and whose they are
    uint16_t lit_code[288], dist_code[32], cl_code[20];   // bit-reversed: ready to be written from bit 0 on
    uint8_t lit_len[288], dist_len[32], cl_len[20];
    uint16_t rle[320];                     // the code lengths in run-length symbols: symbol | extra bits << 8
    uint32_t num_codes[32], next_code[16];
    uint32_t glen[64], gdist[64];          // a group's match per position
    uint32_t gcode_lo[64], gcode_hi[64], gnb[64];   // a group's items: bits and where they go
    uint32_t obuf[OBUF_WORDS];             // the bits of a group on their way out; obuf[0] holds what waits of the last word
    uint32_t crc_tab[256];
    uint32_t crc_mat[32];                  // CRC32 advanced by CRC_CHUNK zero bytes
};

BGZF_HD uint32_t len_symbol(uint32_t L, uint32_t& eb, uint32_t& extra) {
    if (L == MAX_MATCH) { eb = 0; extra = 0; return 285u; }
    const uint32_t l = L - 3u;
    if (l < 8u) { eb = 0; extra = 0; return 257u + l; }
    eb = 29u - (uint32_t)__builtin_clz(l);   // floor(log2 l) - 2
    extra = l & ((1u << eb) - 1u);
    return 261u + 4u * eb + ((l >> eb) & 3u);
}
BGZF_HD uint32_t dist_symbol(uint32_t D, uint32_t& eb, uint32_t& extra) {
    const uint32_t d = D - 1u;
    if (d < 4u) { eb = 0; extra = 0; return d; }
    eb = 30u - (uint32_t)__builtin_clz(d);   // floor(log2 d) - 1
    extra = d & ((1u << eb) - 1u);
    return 2u * eb + 2u + ((d >> eb) & 1u);
}
BGZF_HD uint32_t len_extra_bits(uint32_t s) { return s >= 265u && s < 285u ? (s - 261u) >> 2 : 0u; }
BGZF_HD uint32_t dist_extra_bits(uint32_t s) { return s < 4u ? 0u : (s >> 1) - 1u; }
BGZF_HD uint32_t fixed_lit_len(uint32_t s) { return s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : 8u; }
BGZF_HD uint32_t bit_reverse(uint32_t v, uint32_t n) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < 16u; ++i) r |= ((v >> i) & 1u) << (15u - i);
    return n ? r >> (16u - n) : 0u;
}
// the order in which a dynamic header lists the lengths of the code-length code (RFC 1951 3.2.7)
BGZF_HD uint32_t cl_order(uint32_t i) {
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((i < 12u ? lo >> (5u * i) : hi >> (5u * (i - 12u))) & 31u);
}

template <class P>
struct Deflater {
    P& io;
    DeflateLds& S;
    uint32_t n = 0, ntok = 0, bitpos = 0;

    BGZF_HD Deflater(P& io_, DeflateLds& S_) : io(io_), S(S_) {}

    // once per lane group, before the first block (crc_mat is the caller's to fill)
    BGZF_HD void init() {
        for (uint32_t i = io.lane(); i < 256u; i += P::LANES) S.crc_tab[i] = crc_table_entry(i);
        io.sync();
    }

    BGZF_HD uint32_t match_len(uint32_t q, uint32_t c, uint32_t maxl) const {
        uint32_t l = 0;
        while (l + 4u <= maxl) {
            const uint32_t x = io.text32(q + l) ^ io.text32(c + l);
            if (x) return l + ((uint32_t)__builtin_ctz(x) >> 3);
            l += 4u;
        }
        while (l < maxl && io.text8(q + l) == io.text8(c + l)) ++l;
        return l;
    }

    // ---- the tokens and their histogram
    BGZF_HD void tokens() {
        uint32_t next = 0;   // the first position no match covers yet
        for (uint32_t g0 = 0; g0 < n; g0 += 64u) {
            const uint32_t valid = n - g0 < 64u ? n - g0 : 64u;
            io.for64([&](uint32_t k) {
                const uint32_t q = g0 + k;
                uint32_t len = 0, dist = 0, h = NO_HASH;
                if (k < valid && q + 4u <= n) {
                    const uint32_t v = io.text32(q);
                    h = (v * 0x9E3779B1u) >> (32u - HASH_BITS);
                    const uint32_t maxl = n - q < MAX_MATCH ? n - q : MAX_MATCH;
                    const uint32_t c1 = S.head[h];
                    if (c1 && q - (c1 - 1u) <= MAX_DIST) {
                        len = match_len(q, c1 - 1u, maxl);
                        dist = q - (c1 - 1u);
                    }
                    if (q > 0u) {
                        const uint32_t lb = match_len(q, q - 1u, maxl);
                        if (lb >= len) { len = lb; dist = 1u; }
                    }
                    if (len < MIN_MATCH || (dist > FAR_DIST && len < FAR_MIN_MATCH)) len = 0;
                }
                S.glen[k] = len;
                S.gdist[k] = dist;
                S.gnb[k] = h;
            });
            io.sync();   // every probe of the group saw the table as it stood before the group
            io.for64([&](uint32_t k) {
                const uint32_t h = S.gnb[k];
                if (h != NO_HASH) io.max32(&S.head[h], g0 + k + 1u);
            });
            const uint64_t mm = io.ballot64([&](uint32_t k) { return S.glen[k] != 0u; });
            // the greedy pass: at most one turn per match taken, 64 at the most
            uint64_t sel = 0;
            uint32_t pos = next > g0 ? next - g0 : 0u;
            for (uint32_t turn = 0; turn < 65u && pos < valid; ++turn) {
                const uint64_t rest = mm & ~((1ull << pos) - 1ull);
                uint32_t m = rest ? (uint32_t)__builtin_ctzll(rest) : valid;
                if (m > valid) m = valid;
                // literals at [pos, m)
                const uint64_t upto_m = m >= 64u ? ~0ull : (1ull << m) - 1ull;
                sel |= upto_m & ~((1ull << pos) - 1ull);
                if (m >= valid) { pos = valid; break; }
                sel |= 1ull << m;
                pos = m + io.uni(S.glen[m]);
            }
            next = g0 + pos;
            const uint32_t base = ntok;
            io.for64([&](uint32_t k) {
                if (!((sel >> k) & 1ull)) return;
                const uint32_t idx = base + (uint32_t)__builtin_popcountll(sel & ((1ull << k) - 1ull));
                uint32_t t;
                if ((mm >> k) & 1ull) {
                    const uint32_t L = S.glen[k], D = S.gdist[k];
                    uint32_t eb, ex;
                    io.add(&S.lit_freq[len_symbol(L, eb, ex)], 1u);
                    io.add(&S.dist_freq[dist_symbol(D, eb, ex)], 1u);
                    t = 0x80000000u | (D - 1u) << 8 | (L - 3u);
                } else {
                    t = io.text8(g0 + k);
                    io.add(&S.lit_freq[t], 1u);
                }
                io.tok(idx, t);
            });
            ntok += (uint32_t)__builtin_popcountll(sel);
            io.sync();   // glen / gnb are the next group's to write
        }
    }

    // ---- Huffman lengths of freq[0, ns), at most maxbits each, into len[0, ns): always a complete code of >= 2 symbols
    BGZF_HD void build_lengths(const uint32_t* freq, uint32_t ns, uint32_t maxbits, uint8_t* len) {
        // the symbols in use, sorted by (count, symbol): every lane ranks its own
        uint32_t mine = 0;
        for (uint32_t s = io.lane(); s < ns; s += P::LANES) {
            const uint32_t f = freq[s];
            len[s] = 0;
            if (!f) continue;
            uint32_t r = 0;
            for (uint32_t t = 0; t < ns; ++t) {
                const uint32_t ft = freq[t];
                r += (ft && (ft < f || (ft == f && t < s))) ? 1u : 0u;
            }
            S.key[r] = f;
            S.sym[r] = (uint16_t)s;
            ++mine;
        }
        const uint32_t used = io.reduce_add(mine);
        io.sync();
        // (from here every lane does the same)
        if (used < 2u) {
            const uint32_t s0 = used ? io.uni(S.sym[0]) : 0u;
            len[s0] = 1;
            len[s0 == 0u ? 1u : 0u] = 1;
            io.sync();
            return;
        }
        uint32_t* A = S.key;
        const int nn = (int)used;
        A[0] += A[1];
        int root = 0, leaf = 2;
        for (int nx = 1; nx < nn - 1; ++nx) {
            if (leaf >= nn || io.uni(A[root]) < io.uni(A[leaf])) { A[nx] = A[root]; A[root++] = (uint32_t)nx; }
            else A[nx] = A[leaf++];
            if (leaf >= nn || (root < nx && io.uni(A[root]) < io.uni(A[leaf]))) { A[nx] += A[root]; A[root++] = (uint32_t)nx; }
            else A[nx] += A[leaf++];
        }
        A[nn - 2] = 0;
        for (int nx = nn - 3; nx >= 0; --nx) A[nx] = A[io.uni(A[nx])] + 1u;
        int avbl = 1, usedn = 0, dpth = 0;
        root = nn - 2;
        int nx = nn - 1;
        for (int turn = 0; turn < 64 && avbl > 0; ++turn) {   // (a tree over fewer than 2^17 counts is under 32 deep)
            while (root >= 0 && (int)io.uni(A[root]) == dpth) { ++usedn; --root; }
            while (avbl > usedn && nx >= 0) { A[nx--] = (uint32_t)dpth; --avbl; }
            avbl = 2 * usedn;
            ++dpth;
            usedn = 0;
        }
        for (uint32_t i = 0; i < 32u; ++i) S.num_codes[i] = 0;
        for (int i = 0; i < nn; ++i) {
            const uint32_t d = io.uni(A[i]);
            S.num_codes[d < 31u ? d : 31u] += 1u;
        }
        // lengths above the limit come down to it, and the code is made complete again
        for (uint32_t i = maxbits + 1u; i < 32u; ++i) S.num_codes[maxbits] += S.num_codes[i];
        uint32_t total = 0;
        for (uint32_t i = maxbits; i > 0u; --i) total += io.uni(S.num_codes[i]) << (maxbits - i);
        for (uint32_t turn = 0; turn < 65536u && total != (1u << maxbits); ++turn) {
            S.num_codes[maxbits] -= 1u;
            uint32_t i = maxbits - 1u;
            BGZF_NO_UNROLL
            while (i > 0u && io.uni(S.num_codes[i]) == 0u) --i;
            if (i) {
                S.num_codes[i] -= 1u;
                S.num_codes[i + 1u] += 2u;
            }
            --total;
        }
        int j = nn;
        for (uint32_t i = 1; i <= maxbits; ++i)
            for (uint32_t l = io.uni(S.num_codes[i]); l > 0u && j > 0; --l) len[io.uni(S.sym[--j])] = (uint8_t)i;
        io.sync();
    }

    // the canonical code of len[0, ns), bit-reversed
    BGZF_HD void assign_codes(const uint8_t* len, uint32_t ns, uint16_t* code) {
        for (uint32_t L = io.lane(); L < 16u; L += P::LANES) {
            uint32_t c = 0;
            for (uint32_t s = 0; s < ns; ++s) c += len[s] == L ? 1u : 0u;
            S.num_codes[L] = L ? c : 0u;
        }
        io.sync();
        uint32_t c = 0;
        S.next_code[0] = 0;
        for (uint32_t L = 1; L < 16u; ++L) {   // (every lane the same)
            c = (c + io.uni(S.num_codes[L - 1u])) << 1;
            S.next_code[L] = c;
        }
        io.sync();
        for (uint32_t s = io.lane(); s < ns; s += P::LANES) {
            const uint32_t L = len[s];
            uint32_t r = 0;
            for (uint32_t t = 0; t < s; ++t) r += len[t] == L ? 1u : 0u;
            code[s] = (uint16_t)(L ? bit_reverse(S.next_code[L] + r, L) : 0u);
        }
        io.sync();
    }

    // ---- the bits.  gen(i, code, nb): item i of `count` is `nb` <= 48 bits, `code` from bit 0 on
    template <class Gen>
    BGZF_HD void emit(uint32_t count, Gen gen) {
        for (uint32_t base = 0; base < count; base += 64u) {
            const uint32_t m = count - base < 64u ? count - base : 64u;
            io.for64([&](uint32_t k) {
                uint64_t c = 0;
                uint32_t nb = 0;
                if (k < m) gen(base + k, c, nb);
                S.gcode_lo[k] = (uint32_t)c;
                S.gcode_hi[k] = (uint32_t)(c >> 32);
                S.gnb[k] = nb;
            });
            io.sync();
            const uint32_t total = io.scan64(S.gnb);
            const uint32_t sh0 = bitpos & 31u;
            io.for64([&](uint32_t k) {
                const uint64_t c = (uint64_t)S.gcode_lo[k] | (uint64_t)S.gcode_hi[k] << 32;
                if (!c) return;
                const uint32_t o = sh0 + S.gnb[k], w = o >> 5, s = o & 31u;
                const uint64_t c2 = s ? c >> (32u - s) : c >> 32;
                const uint32_t v0 = (uint32_t)c << s, v1 = (uint32_t)c2, v2 = (uint32_t)(c2 >> 32);
                if (v0) io.or32(&S.obuf[w], v0);
                if (v1) io.or32(&S.obuf[w + 1u], v1);
                if (v2) io.or32(&S.obuf[w + 2u], v2);
            });
            io.sync();
            const uint32_t full = (sh0 + total) >> 5, wbase = bitpos >> 5;
            for (uint32_t i = io.lane(); i < full; i += P::LANES) io.out32(wbase + i, S.obuf[i]);
            const uint32_t carry = io.uni(S.obuf[full]);
            io.sync();
            for (uint32_t i = io.lane(); i < OBUF_WORDS; i += P::LANES) S.obuf[i] = i ? 0u : carry;
            io.sync();
            bitpos += total;
        }
    }

    BGZF_HD void put_bytes(uint32_t at, uint64_t v, uint32_t count) {   // count <= 8 bytes of v at byte `at` of the member
        for (uint32_t k = io.lane(); k < count; k += P::LANES) io.out8(at + k, (uint8_t)(v >> (8u * k)));
    }

    BGZF_HD uint32_t crc_of_text() {
        const uint32_t l = io.lane();
        const uint64_t back = (uint64_t)l * P::CRC_CHUNK;
        uint32_t c = 0xFFFFFFFFu;
        if (back < n) {
            const uint32_t ce = n - (uint32_t)back, cs = ce > P::CRC_CHUNK ? ce - P::CRC_CHUNK : 0u;
            for (uint32_t q = cs; q < ce; ++q) c = S.crc_tab[(c ^ io.text8(q)) & 255u] ^ (c >> 8);
        }
        const uint32_t mine = ~c;
        const uint32_t nchunks = (n + P::CRC_CHUNK - 1u) / P::CRC_CHUNK;
        return crc_fold(S.crc_mat, nchunks, [&](uint32_t k) { return io.uni(io.shfl(mine, k)); });
    }

    // the block's text (n_ >= 1 bytes, at most BLOCK_TEXT) -> the member; returns its size
    BGZF_HD uint32_t run(uint32_t n_) {
        const uint32_t l = io.lane();
        n = n_;
        ntok = 0;
        for (uint32_t i = l; i < (1u << HASH_BITS); i += P::LANES) S.head[i] = 0;
        for (uint32_t i = l; i < 288u; i += P::LANES) S.lit_freq[i] = 0;
        for (uint32_t i = l; i < 32u; i += P::LANES) S.dist_freq[i] = 0;
        for (uint32_t i = l; i < 20u; i += P::LANES) S.cl_freq[i] = 0;
        for (uint32_t i = l; i < OBUF_WORDS; i += P::LANES) S.obuf[i] = 0;
        io.sync();
        const uint32_t crc = crc_of_text();
        tokens();
        if (l == 0) S.lit_freq[256] = 1;   // the end-of-block code
        io.sync();
        build_lengths(S.lit_freq, 288u, 15u, S.lit_len);   // (286, 287 and the distances 30, 31 never count: length 0)
        build_lengths(S.dist_freq, 32u, 15u, S.dist_len);
        uint32_t hlit = 286u, hdist = 30u;
        while (hlit > 257u && io.uni(S.lit_len[hlit - 1u]) == 0u) --hlit;
        while (hdist > 1u && io.uni(S.dist_len[hdist - 1u]) == 0u) --hdist;
        // the lengths as run-length symbols (every lane the same)
        const uint32_t nlen = hlit + hdist;
        auto seq = [&](uint32_t i) { return (uint32_t)io.uni(i < hlit ? S.lit_len[i] : S.dist_len[i - hlit]); };
        uint32_t nr = 0;
        for (uint32_t i = 0; i < nlen;) {
            const uint32_t v = seq(i);
            uint32_t run = 1;
            while (i + run < nlen && seq(i + run) == v) ++run;
            i += run;
            if (v == 0u) {
                while (run >= 11u) {
                    const uint32_t c = run < 138u ? run : 138u;
                    S.rle[nr++] = (uint16_t)(18u | (c - 11u) << 8);
                    S.cl_freq[18] += 1u;
                    run -= c;
                }
                if (run >= 3u) {
                    S.rle[nr++] = (uint16_t)(17u | (run - 3u) << 8);
                    S.cl_freq[17] += 1u;
                    run = 0;
                }
            } else {
                S.rle[nr++] = (uint16_t)v;
                S.cl_freq[v] += 1u;
                --run;
                while (run >= 3u) {
                    const uint32_t c = run < 6u ? run : 6u;
                    S.rle[nr++] = (uint16_t)(16u | (c - 3u) << 8);
                    S.cl_freq[16] += 1u;
                    run -= c;
                }
            }
            for (; run > 0u; --run) {
                S.rle[nr++] = (uint16_t)v;
                S.cl_freq[v] += 1u;
            }
        }
        io.sync();
        build_lengths(S.cl_freq, 19u, 7u, S.cl_len);
        uint32_t hclen = 19u;
        while (hclen > 4u && io.uni(S.cl_len[cl_order(hclen - 1u)]) == 0u) --hclen;
        // ---- what each form costs, in bits
        uint32_t dyn = 0, fix = 0;
        for (uint32_t s = l; s < 286u; s += P::LANES) {
            const uint32_t f = S.lit_freq[s], e = len_extra_bits(s);
            dyn += f * (S.lit_len[s] + e);
            fix += f * (fixed_lit_len(s) + e);
        }
        for (uint32_t s = l; s < 30u; s += P::LANES) {
            const uint32_t f = S.dist_freq[s], e = dist_extra_bits(s);
            dyn += f * (S.dist_len[s] + e);
            fix += f * (5u + e);
        }
        for (uint32_t i = l; i < nr; i += P::LANES) {
            const uint32_t s = S.rle[i] & 255u;
            dyn += S.cl_len[s] + (s == 16u ? 2u : s == 17u ? 3u : s == 18u ? 7u : 0u);
        }
        dyn = io.reduce_add(dyn) + 3u + 14u + 3u * hclen;
        fix = io.reduce_add(fix) + 3u;
        const uint32_t dyn_bytes = (dyn + 7u) >> 3, fix_bytes = (fix + 7u) >> 3, stored_bytes = n + 5u;
        uint32_t end;   // the byte behind the DEFLATE stream
        put_bytes(0, 0x0000000004088b1full, 8);
        put_bytes(8, 0x000243420006ff00ull, 8);
        if (stored_bytes <= dyn_bytes && stored_bytes <= fix_bytes) {
            put_bytes(18, 1ull | (uint64_t)n << 8 | (uint64_t)(~n & 0xFFFFu) << 24, 5);
            for (uint32_t i = l; i < n; i += P::LANES) io.out8(23u + i, io.text8(i));
            end = 23u + n;
        } else {
            const bool fixed = fix_bytes <= dyn_bytes;
            if (fixed) {
                for (uint32_t s = l; s < 288u; s += P::LANES) S.lit_len[s] = (uint8_t)fixed_lit_len(s);
                for (uint32_t s = l; s < 32u; s += P::LANES) S.dist_len[s] = 5;
                io.sync();
            }
            assign_codes(S.lit_len, 288u, S.lit_code);
            assign_codes(S.dist_len, 32u, S.dist_code);
            bitpos = 18u * 8u;   // (obuf[0] is zero: the two bytes of BSIZE in front of the stream are written last)
            if (fixed) {
                emit(1u, [&](uint32_t, uint64_t& c, uint32_t& nb) { c = 3u; nb = 3u; });   // BFINAL, BTYPE 01
            } else {
                assign_codes(S.cl_len, 19u, S.cl_code);
                emit(1u + hclen, [&](uint32_t i, uint64_t& c, uint32_t& nb) {
                    if (i == 0u) { c = 5u | (uint64_t)(hlit - 257u) << 3 | (uint64_t)(hdist - 1u) << 8 | (uint64_t)(hclen - 4u) << 13; nb = 17u; }
                    else { c = S.cl_len[cl_order(i - 1u)]; nb = 3u; }
                });
                emit(nr, [&](uint32_t i, uint64_t& c, uint32_t& nb) {
                    const uint32_t r = S.rle[i], s = r & 255u, cl = S.cl_len[s];
                    c = (uint64_t)S.cl_code[s] | (uint64_t)(r >> 8) << cl;
                    nb = cl + (s == 16u ? 2u : s == 17u ? 3u : s == 18u ? 7u : 0u);
                });
            }
            emit(ntok + 1u, [&](uint32_t i, uint64_t& c, uint32_t& nb) {
                if (i == ntok) { c = S.lit_code[256]; nb = S.lit_len[256]; return; }
                const uint32_t t = io.tok_at(i);
                if (!(t & 0x80000000u)) { c = S.lit_code[t]; nb = S.lit_len[t]; return; }
                uint32_t leb, lex, deb, dex;
                const uint32_t ls = len_symbol((t & 255u) + 3u, leb, lex), ds = dist_symbol(((t >> 8) & 0x7FFFu) + 1u, deb, dex);
                c = S.lit_code[ls];
                nb = S.lit_len[ls];
                c |= (uint64_t)lex << nb;
                nb += leb;
                c |= (uint64_t)S.dist_code[ds] << nb;
                nb += S.dist_len[ds];
                c |= (uint64_t)dex << nb;
                nb += deb;
            });
            end = (bitpos + 7u) >> 3;
            const uint32_t wb = bitpos >> 5;
            put_bytes(4u * wb, S.obuf[0], end - 4u * wb);   // what waits of the last word (BSIZE, if the stream ends in its word)
            io.sync();
        }
        const uint32_t size = end + 8u;
        put_bytes(end, (uint64_t)crc | (uint64_t)n << 32, 8);
        put_bytes(16, size - 1u, 2);
        io.sync();
        return size;
    }
};

// ---- the host's lane: one lane, every step a loop
struct HostDeflateLane {
    static constexpr uint32_t LANES = 1, CRC_CHUNK = 65536;
    const uint8_t* text;
    uint32_t* toks;
    uint8_t* out;
    uint32_t lane() const { return 0; }
    void sync() const {}
    uint32_t uni(uint32_t v) const { return v; }
    uint32_t shfl(uint32_t v, uint32_t) const { return v; }
    template <class F> void for64(F f) const { for (uint32_t k = 0; k < 64u; ++k) f(k); }
    template <class F> uint64_t ballot64(F f) const {
        uint64_t m = 0;
        for (uint32_t k = 0; k < 64u; ++k) m |= (uint64_t)(f(k) ? 1u : 0u) << k;
        return m;
    }
    uint32_t scan64(uint32_t* a) const {
        uint32_t s = 0;
        for (uint32_t k = 0; k < 64u; ++k) { const uint32_t v = a[k]; a[k] = s; s += v; }
        return s;
    }
    uint32_t reduce_add(uint32_t v) const { return v; }
    void add(uint32_t* p, uint32_t v) const { *p += v; }
    void or32(uint32_t* p, uint32_t v) const { *p |= v; }
    void max32(uint32_t* p, uint32_t v) const { if (v > *p) *p = v; }
    uint8_t text8(uint32_t q) const { return text[q]; }
    uint32_t text32(uint32_t q) const { return text[q] | (uint32_t)text[q + 1] << 8 | (uint32_t)text[q + 2] << 16 | (uint32_t)text[q + 3] << 24; }
    void tok(uint32_t i, uint32_t t) const { toks[i] = t; }
    uint32_t tok_at(uint32_t i) const { return toks[i]; }
    void out8(uint32_t a, uint8_t v) const { out[a] = v; }
    void out32(uint32_t w, uint32_t v) const {
        for (uint32_t k = 0; k < 4u; ++k) out[4u * w + k] = (uint8_t)(v >> (8u * k));
    }
};

// the bytes a slot of the staging area needs for a block of `bt` bytes of text: the member, and room for word stores and loads
BGZF_HD uint32_t slot_bytes(uint32_t bt) { return ((bt + MEMBER_EXTRA + 15u) & ~15u) + 16u; }

}  // namespace bgzf
}  // namespace bsk
