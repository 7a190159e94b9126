// Plain gzip (RFC 1952, any number of members, DEFLATE blocks of every type) read in chunks that are decoded at once: the same
// source for the kernels (ops_gzip.hip, 64 lanes) and for the host (bsk_gzip_inflate_host, tests/host_c/gzip_host_check.cpp, one
// lane).  PARITY.md GZIP: zlib defines the bytes; the method below is a way to compute them, and its output does not depend on
// the chunk size or on what the finder reports.
//
//   find       for every chunk of the compressed bytes but the first, the lowest bit position S_k inside it at which a non-final
//              dynamic block can start (header_ok).  A true header is never rejected; a false one costs time, never bytes.
//   size       from S_k (chunk 0: from the first member's header) the stream is decoded without producing bytes, until a block
//              ends exactly on the S_j of a later chunk ("landed on j"), or behind the last trailer ("landed on the end"), or in
//              an error.  The result is where it landed, the text bytes, the members crossed.
//   chain      walking from chunk 0 by "landed on" gives the chunks that the true chain of blocks visits; the others are dropped.
//              A scan of their byte counts gives every chunk its text offset.
//   decode     the chain chunks again, now writing 16-bit symbols: 0..255 is a byte, 0x8000 | m is "the byte at text position
//              chunk_start - 32768 + m", which the chunk cannot know.  The window is a ring of symbols, matches copy symbols.
//   windows    for the chain chunks in order, the 32 KiB of text in front of chunk j from its predecessor's symbols and window.
//   translate  text[q] = sym < 0x8000 ? sym : W_chunk[sym & 0x7FFF], every symbol on its own.
//   crc        pieces of at most 64 KiB that never span members; the host joins a member's pieces with the advance operator of
//              their lengths and compares with the CRC32 and ISIZE of the trailer.
//
// Positions are bit positions from the start of the compressed buffer, in 64 bits.  The bit reader, the tables of a block and
// the decode of a symbol are those of the BGZF decoder (bgzf::HuffCore); what is new here is the walk over blocks and members,
// the symbol ring, and everything after it.  Hang safety as there: every pass of every loop consumes at least one bit or ends,
// every position is counted against the end of the buffer, so a decode from a false start ends in an error, on a candidate, or
// at the end of the buffer.
//
// A lane policy P: LANES, lane(), sync(), uni(v), uni64(v), word(w) (64-bit word index, zero past the end), in_byte(a) (64-bit,
// bounded by the caller), vec64(v) (v as a value that need not be the same in every lane), store(ring, out, shift, a, b) (symbols [a, b) of the chunk leave the ring for out[a, b)).
#pragma once
#include <cstdint>

#include "bgzf_inflate_dev.hpp"

#include <string>
#include <vector>

namespace bsk {
namespace gz {

using bgzf::DIST_ROOT;
using bgzf::LIT_ROOT;
using bgzf::RING;
using bgzf::RING_MASK;

enum : int {
    ERR_HEADER = 12,   // the bytes where a member must begin are no gzip member header (zero padding included)
    ERR_MARKER = 13,   // (internal) a symbol that names a byte in front of its member: reported as ERR_DISTANCE
};

BGZF_HD const char* error_text(int code) {
    if (code == ERR_HEADER) return "the bytes after the last member are not a gzip member header";
    return bgzf::error_text(code);
}

constexpr uint64_t NONE = ~0ull;          // no candidate in the chunk / the chunk was not run / no member began in the chunk
constexpr uint64_t LAND_END = ~0ull - 1;  // landed behind the last trailer, at the end of the buffer
constexpr uint32_t MAX_MEMBERS = 65536;
constexpr uint32_t WIN = 32768;           // bytes of text a match can reach back
constexpr uint32_t FIND_STEP = 8192;      // compressed bytes that the finder searches before it looks whether it has a hit
constexpr uint32_t PIECE = 65536;         // text bytes of a CRC piece
constexpr uint32_t CRC_CHUNK = 1024;      // ... of which a lane takes this many at a time
constexpr uint32_t DRAIN_AT = 16384;      // symbols that wait in the ring before they are stored

struct ChunkResult {
    uint64_t land;      // a chunk index, LAND_END, or NONE with err set
    uint64_t text;      // text bytes from the start position to where it landed
    uint64_t mstart;    // text offset inside the chunk at which the last member began that began here, or NONE
    uint64_t err_bit;   // where the error was met
    uint32_t members;   // trailers crossed
    uint32_t err;
};
struct MemberRec {
    uint64_t trailer;   // file offset of CRC32, ISIZE
    uint64_t text_end;  // text offset behind the member's last byte (as the walk leaves it: from the chunk's start)
    uint32_t crc, isize;
};

// what every walk of a call shares: the compressed bytes are cut into `nchunks` chunks of `chunk_bytes`, cand[k] is S_k.  The
// walks read it where a block ends, not before: nothing of it stays in registers while symbols are decoded
struct Geometry {
    uint64_t n, chunk_bytes, nchunks;
    const uint64_t* cand;
    uint32_t chunk_shift;  // chunk_bytes * 8 == 1 << chunk_shift, or one chunk and 63: a chunk is found by a shift
};
// chunk sizes are powers of two (a size in between is rounded down); 0 or a size that holds everything: one chunk
inline Geometry geometry(uint64_t n, uint64_t chunk_bytes, const uint64_t* cand) {
    if (chunk_bytes == 0 || chunk_bytes >= n) return Geometry{n, n, n ? 1u : 0u, cand, 63u};
    uint32_t lg = 0;
    while ((2ull << lg) <= chunk_bytes) ++lg;
    return Geometry{n, 1ull << lg, (n + (1ull << lg) - 1) >> lg, cand, lg + 3u};
}

// What a walk needs only where a block or a member ends.  It waits with the tables, not in registers: the tables of a dynamic
// block are built with every scalar register the wave has (the BGZF kernel shows it), and whatever else is live then is spilled
struct Parked {
    Geometry G;
    uint64_t k;        // the chunk
    uint64_t limit;    // EMIT: the symbols this chunk may write (what the size pass counted)
    uint64_t mstart;   // where the last member began that began in this chunk, or NONE
    MemberRec* mrec;   // EMIT: the members that end in this chunk
    uint16_t* out;     // EMIT: the chunk's symbols
    uint32_t mcap;     // EMIT: how many mrec holds
};

// the tables of a block, as bgzf::BgzfLds has them (HuffCore reaches them by name)
struct GzTables {
    uint16_t lit_fast[1u << LIT_ROOT];
    uint16_t dist_fast[1u << DIST_ROOT];
    uint16_t lit_count[16], lit_sym[288];
    uint16_t dist_count[16], dist_sym[32];
    uint8_t lens[320];
    Parked park;
};
// ... and with the window of the decode: 32 Ki symbols of 16 bits
struct GzDecodeLds {
    alignas(16) uint16_t ring[RING];
    GzTables T;
};

// a CRC piece: text [off, off + len) of member `member`
struct Piece { uint64_t off; uint32_t len; uint32_t member; };

// ---- the finder's predicate.  64 bits from bit position pos, bits past the end read as 0; word(w) as in the policy
template <class Word>
BGZF_HD uint64_t bits_at(Word word, uint64_t pos) {
    const uint64_t w = pos >> 5;
    const uint32_t sh = (uint32_t)(pos & 31u);
    const uint64_t lo = (uint64_t)word(w) | (uint64_t)word(w + 1) << 32;
    return sh ? (lo >> sh) | ((uint64_t)word(w + 2) << (64u - sh)) : lo;
}

// Can a non-final dynamic block start at bit `pos` of a buffer of `total` bits?  Exactly: BFINAL = 0, BTYPE = 2, and
// HuffCore::tables(2) would return OK there -- HLIT <= 286, HDIST <= 30, a complete code-length code, a legal run-length stream
// that does not overrun, a code for 256, and neither set over-subscribed, nor incomplete except as a single code of length 1 (or,
// for distances, no code at all).  It holds no array: tables() refuses a set by the COUNTS of its lengths alone, and those are
// what the Kraft sums below carry (over-subscribed at some length <=> the whole sum is above 1).  A TRUE HEADER IS NEVER REJECTED:
// every `return false` below stands for one `return ERR_*` of tables(), build() or read_lengths(), and nothing else is refused;
// tests/test_gzip_cpu.py and tests/host_c/gzip_host_check.cpp pin it against the decoder itself.  The cheap rejections come
// first: three bits, the two ranges, the Kraft sum of the 3-bit lengths.
template <class Word>
BGZF_HD bool header_ok(Word word, uint64_t total, uint64_t pos) {
    if (pos + 17u > total) return false;
    uint64_t v = bits_at(word, pos);
    if ((v & 7u) != 4u) return false;
    const uint32_t hlit = ((uint32_t)(v >> 3) & 31u) + 257u, hdist = ((uint32_t)(v >> 8) & 31u) + 1u, hclen = ((uint32_t)(v >> 13) & 15u) + 4u;
    if (hlit > 286u || hdist > 30u) return false;
    uint64_t q = pos + 17u;
    if (q + 3u * hclen > total) return false;
    v = bits_at(word, q);
    const uint64_t order_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t order_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    uint64_t cl = 0;     // the 19 lengths of the code-length code, three bits each, by symbol
    uint64_t cnts = 0;   // codes per length 1 .. 7, five bits each
    uint32_t kraft = 0;  // in units of 2^-7
    for (uint32_t i = 0; i < hclen; ++i) {
        const uint64_t len = (v >> (3u * i)) & 7u;
        const uint32_t at = (uint32_t)((i < 12u ? order_lo >> (5u * i) : order_hi >> (5u * (i - 12u))) & 31u);
        cl |= len << (3u * at);
        if (len) {
            kraft += 128u >> len;
            cnts += 1ull << (5u * len);
        }
    }
    if (kraft != 128u) return false;
    q += 3u * hclen;
    const uint32_t ncodes = hlit + hdist;
    uint32_t i = 0, prev = 0, have256 = 0, kl = 0, kd = 0, maxl = 0, maxd = 0;  // Kraft sums in units of 2^-15
    while (i < ncodes) {
        v = bits_at(word, q);
        uint32_t code = 0, first = 0, len = 1, rank = 0;
        for (; len <= 7u; ++len) {
            code |= (uint32_t)(v & 1u);
            v >>= 1;
            const uint32_t c = (uint32_t)(cnts >> (5u * len)) & 31u;
            if (code < first + c) { rank = code - first; break; }
            first = (first + c) << 1;
            code <<= 1;
        }
        if (len > 7u) return false;  // (cannot be: the code is complete)
        q += len;
        if (q > total) return false;
        uint32_t sym = 0;  // the rank-th symbol of this length, in symbol order
        for (uint32_t s = 0, seen = 0; s < 19u; ++s)
            if (((cl >> (3u * s)) & 7u) == len) {
                if (seen == rank) { sym = s; break; }
                ++seen;
            }
        uint32_t rep = 1, val = sym;
        if (sym >= 16u) {
            if (sym == 16u && i == 0) return false;
            const uint32_t eb = sym == 16u ? 2u : sym == 17u ? 3u : 7u;
            val = sym == 16u ? prev : 0u;
            rep = (sym == 18u ? 11u : 3u) + ((uint32_t)v & ((1u << eb) - 1u));
            q += eb;
            if (q > total) return false;
        }
        if (i + rep > ncodes) return false;
        if (val && i <= 256u && 256u < i + rep) have256 = 1;
        if (val) {
            const uint32_t nl = i >= hlit ? 0u : (hlit - i < rep ? hlit - i : rep), nd = rep - nl;
            kl += nl * (32768u >> val);
            kd += nd * (32768u >> val);
            if (nl && val > maxl) maxl = val;
            if (nd && val > maxd) maxd = val;
            if (kl > 32768u || kd > 32768u) return false;
        }
        i += rep;
        prev = val;
    }
    if (!have256) return false;
    if (kl < 32768u && maxl > 1u) return false;
    if (kd < 32768u && maxd > 1u) return false;
    return true;
}

// ---- the walk over blocks and members from one start.  EMIT false: sizes only (no ring); true: symbols.  RESUME: the buffer is
// a segment of a file that is re-entered (gzip_stream.hpp): chunk 0 starts at the bit cand[0] like every later chunk, inside a
// member whose start it does not know
template <class P, bool EMIT, bool RESUME = false>
struct Walker : bgzf::HuffCore<P, GzTables, uint64_t> {
    using Core = bgzf::HuffCore<P, GzTables, uint64_t>;
    using Core::io; using Core::S; using Core::buf; using Core::left; using Core::cnt; using Core::in_end;
    using Core::seek; using Core::need32; using Core::drop; using Core::peek; using Core::symbol; using Core::tables;
    uint16_t* ring;
    uint64_t p = 0;               // symbols produced
    uint32_t wait = 0;            // ... of which the last `wait` are not stored yet
    uint64_t room = 0;            // EMIT: the symbols this chunk may still write (the size pass counted them)
    uint32_t since = ~0u;         // symbols since the member began, if it began in this chunk: counted up to 65536; else ~0
    uint32_t shift = 0, nlit = 0, mylit = 0;

    BGZF_HD Walker(P& io_, GzTables& T_, uint16_t* ring_) : Core(io_, T_), ring(ring_) {}
    BGZF_HD uint32_t ring_at(uint64_t q) const { return (shift + (uint32_t)q) & RING_MASK; }
    BGZF_HD uint64_t bit_pos() const { return in_end * 8u - left; }

    BGZF_HD void grew(uint32_t by) {  // by <= 65535
        if (since < 65536u) since += by;
    }
    BGZF_HD void drain(uint32_t keep) {  // all but the last `keep` symbols leave the ring
        io.store(ring, S.park.out, shift, p - wait, p - keep);
        wait = keep;
    }
    BGZF_HD void maybe_drain() {
        if (wait >= DRAIN_AT) drain((shift + (uint32_t)p) & 7u);  // (up to a 16-byte boundary of the symbol buffer)
    }
    BGZF_HD void flush_lits() {
        if (EMIT && nlit) {
            if (io.lane() < nlit) ring[ring_at(p + io.lane())] = (uint16_t)mylit;
            p += nlit;
            wait += nlit;
            room -= nlit;
            grew(nlit);
            nlit = 0;
            io.sync();
            maybe_drain();
        }
    }

    // a bounded, byte-counting read of a member header at `byte`; behind it, `byte` is the first byte of the deflate data
    BGZF_HD int member_header(uint64_t& byte) {
        const uint64_t n = in_end;
        auto at = [&](uint64_t a) { return io.uni((uint32_t)io.in_byte(a)); };
        if (byte < n && at(byte) != 0x1fu) return ERR_HEADER;
        if (byte + 1u < n && at(byte + 1u) != 0x8bu) return ERR_HEADER;
        if (n - byte < 10u) return bgzf::ERR_TRUNCATED;
        const uint32_t flg = at(byte + 3u);
        if (at(byte + 2u) != 8u || (flg & 0xE0u)) return ERR_HEADER;
        byte += 10u;
        if (flg & 4u) {  // FEXTRA
            if (n - byte < 2u) return bgzf::ERR_TRUNCATED;
            const uint32_t xlen = at(byte) | at(byte + 1u) << 8;
            byte += 2u;
            if (n - byte < xlen) return bgzf::ERR_TRUNCATED;
            byte += xlen;
        }
        for (uint32_t bit = 8u; bit <= 16u; bit <<= 1) {  // FNAME, FCOMMENT: zero-terminated
            if (!(flg & bit)) continue;
            for (;;) {
                if (byte >= n) return bgzf::ERR_TRUNCATED;
                if (at(byte++) == 0u) break;
            }
        }
        if (flg & 2u) {  // FHCRC
            if (n - byte < 2u) return bgzf::ERR_TRUNCATED;
            byte += 2u;
        }
        return bgzf::OK;
    }

    BGZF_HD int read_stored() {
        if (!drop((uint32_t)(left & 7u))) return bgzf::ERR_TRUNCATED;
        need32();
        const uint32_t len = peek(16), nlen = (uint32_t)(buf >> 16) & 0xFFFFu;
        if (!drop(32)) return bgzf::ERR_TRUNCATED;
        if (len != (~nlen & 0xFFFFu)) return bgzf::ERR_STORED_LEN;
        if ((uint64_t)len * 8u > left) return bgzf::ERR_TRUNCATED;
        const uint64_t src = in_end - left / 8u;
        grew(len);
        if (EMIT) {
            if (len > room) return bgzf::ERR_OVERRUN;
            room -= len;
            for (uint32_t done = 0; done < len;) {
                const uint32_t m = len - done < 4096u ? len - done : 4096u;
                for (uint32_t i = io.lane(); i < m; i += P::LANES) ring[ring_at(p + i)] = (uint16_t)io.in_byte(src + done + i);
                p += m;
                wait += m;
                done += m;
                io.sync();
                maybe_drain();
            }
        } else {
            p += len;
        }
        seek(src + len);
        return bgzf::OK;
    }

    BGZF_HD int read_codes() {
        const uint32_t l = io.lane();
        for (;;) {
            int r = symbol(S.lit_fast, LIT_ROOT, S.lit_count, S.lit_sym);
            if (r < 0) return -r;
            uint32_t sym = (uint32_t)r;
            if (sym < 256u) {
                if (EMIT) {
                    if (nlit >= room) return bgzf::ERR_OVERRUN;
                    if (l == nlit) mylit = sym;
                    if (++nlit == P::LANES) flush_lits();
                } else {
                    ++p;
                    grew(1);
                }
                continue;
            }
            if (sym == 256u) return bgzf::OK;
            if (sym > 285u) return bgzf::ERR_INVALID_CODE;
            flush_lits();
            uint32_t L, eb;
            if (sym < 265u) { L = sym - 254u; eb = 0; }
            else if (sym == 285u) { L = 258u; eb = 0; }
            else { const uint32_t s = sym - 261u; eb = s >> 2; L = ((4u + (s & 3u)) << eb) + 3u; }
            L += peek(eb);
            if (!drop(eb)) return bgzf::ERR_TRUNCATED;
            r = symbol(S.dist_fast, DIST_ROOT, S.dist_count, S.dist_sym);
            if (r < 0) return -r;
            sym = (uint32_t)r;
            if (sym > 29u) return bgzf::ERR_INVALID_CODE;
            uint32_t D;
            if (sym < 4u) { D = sym + 1u; eb = 0; }
            else { eb = (sym >> 1) - 1u; D = ((2u + (sym & 1u)) << eb) + 1u; }
            D += peek(eb);
            if (!drop(eb)) return bgzf::ERR_TRUNCATED;
            // a member that began in this chunk knows its start: nothing in front of it can be meant.  Otherwise the ring
            // holds markers in front of the chunk (D <= 32768 by the format), and the windows pass checks what they name
            if (D > since) return bgzf::ERR_DISTANCE;
            grew(L);
            if (EMIT) {
                if (L > room) return bgzf::ERR_OVERRUN;
                room -= L;
                // lane i writes symbol p + i from p - D + (i mod D): every source lies in front of p
                for (uint32_t i = l; i < L; i += P::LANES) ring[ring_at(p + i)] = ring[ring_at(p - D + (i < D ? i : i % D))];
                p += L;
                wait += L;
                io.sync();
                maybe_drain();
            } else {
                p += L;
            }
        }
    }

    // The chunk of S.park (the caller has filled it and synchronised).  EMIT: the symbols go out through the policy, laid out for
    // a text offset that is `shift_` modulo 8; the members that end here go to park.mrec[0 ..) with text_end counted from the
    // chunk's start (the caller has sized it by the size pass)
    BGZF_HD ChunkResult run(uint32_t shift_) {
        ChunkResult R{NONE, 0, NONE, 0, 0, 0};
        // (counters that steer nothing live in vector registers on the device: the scalar ones are what the tables are built with)
        p = io.vec64(0);
        R.members = (uint32_t)io.vec64(0);
        in_end = io.n;
        room = io.uni64(S.park.limit);
        shift = shift_ & 7u;
        int rc = bgzf::OK;
        if (!RESUME && io.uni64(S.park.k) == 0) {
            uint64_t byte = 0;
            rc = member_header(byte);
            if (rc) {
                R.err = rc == ERR_HEADER ? (uint32_t)-1 : (uint32_t)rc;  // (the first bytes: not gzip at all)
                return R;
            }
            seek(byte);
            since = 0;
        } else {
            const uint64_t s = io.uni64(S.park.G.cand[io.uni64(S.park.k)]);
            seek(s >> 3);
            (void)drop((uint32_t)(s & 7u));
            if (EMIT) {  // in front of the chunk: markers.  Text position -32768 + m lies at ring_at(m)
                for (uint32_t m = io.lane(); m < WIN; m += P::LANES) ring[ring_at(m)] = (uint16_t)(0x8000u | m);
                io.sync();
            }
        }
        for (;;) {
            need32();
            const uint32_t last = peek(1), type = (uint32_t)(buf >> 1) & 3u;
            if (!drop(3)) rc = bgzf::ERR_TRUNCATED;
            else if (type == 0u) rc = read_stored();
            else if (type == 3u) rc = bgzf::ERR_BLOCK_TYPE;
            else {
                rc = tables(type);
                if (rc == bgzf::OK) rc = read_codes();
                if (rc == bgzf::OK) flush_lits();
            }
            if (rc) break;
            if (!last) {
                const uint64_t e = bit_pos(), j = e >> io.uni(S.park.G.chunk_shift);
                if (j > io.uni64(S.park.k) && j < io.uni64(S.park.G.nchunks) && io.uni64(S.park.G.cand[j]) == e) { R.land = j; break; }
                continue;
            }
            (void)drop((uint32_t)(left & 7u));
            uint64_t byte = in_end - left / 8u;
            if (in_end - byte < 8u) { rc = bgzf::ERR_TRUNCATED; break; }
            if (EMIT) {
                auto at = [&](uint64_t a) { return io.uni((uint32_t)io.in_byte(a)); };
                const uint32_t c = at(byte) | at(byte + 1) << 8 | at(byte + 2) << 16 | at(byte + 3) << 24;
                const uint32_t z = at(byte + 4) | at(byte + 5) << 8 | at(byte + 6) << 16 | at(byte + 7) << 24;
                if (io.lane() == 0 && R.members < S.park.mcap) S.park.mrec[R.members] = MemberRec{byte, p, c, z};
            }
            ++R.members;
            byte += 8u;
            seek(byte);  // (an error of the header is reported where the header begins)
            if (byte == in_end) { R.land = LAND_END; break; }
            rc = member_header(byte);
            if (rc) break;
            seek(byte);
            since = 0;
            if (io.lane() == 0) S.park.mstart = p;
        }
        if (rc) {
            R.err = (uint32_t)rc;
            R.err_bit = bit_pos();
        }
        if (EMIT) drain(0);
        io.sync();
        R.mstart = io.uni64(S.park.mstart);
        R.text = p;
        return R;
    }
};

// ================= the host's side of the method: shared by the device path (ops_gzip.hip) and the host path below

// the advance operator of any length: "append 2^k zero bytes" by squaring, a length by its binary digits
struct CrcAdvance {
    uint32_t pow[48][32];
    CrcAdvance() {
        bgzf::crc_advance_matrix(pow[0], 1);
        for (int k = 1; k < 48; ++k)
            for (int i = 0; i < 32; ++i) pow[k][i] = bgzf::crc_mat_times(pow[k - 1], pow[k - 1][i]);
    }
    uint32_t advance(uint32_t crc, uint64_t bytes) const {
        for (int k = 0; bytes && k < 48; ++k, bytes >>= 1)
            if (bytes & 1u) crc = bgzf::crc_mat_times(pow[k], crc);
        return crc;
    }
};

enum : int { FAIL_NONE = 0, FAIL_FORMAT = 1, FAIL_UNSUPPORTED = 2, FAIL_NOT_GZIP = 3 };

inline std::string where(uint64_t member, uint64_t off) { return "libbsk: gzip: member " + std::to_string(member) + " at offset " + std::to_string(off) + ": "; }

struct ChainChunk {
    uint64_t k;          // the chunk
    uint64_t text_off;   // where its text begins
    uint64_t text;       // bytes
    uint64_t member0;    // members in front of it
    uint32_t members;
    uint32_t marker_lo;  // markers below this name a byte in front of the member that is open at the chunk's start
};

struct Plan {
    uint64_t chunks = 0, with_candidate = 0, on_chain = 0, off_chain = 0, members = 0, text = 0, dropped_text = 0, chunk_bytes = 0;
    void to(uint64_t out[8]) const {
        out[0] = chunks; out[1] = with_candidate; out[2] = on_chain; out[3] = off_chain;
        out[4] = members; out[5] = text; out[6] = dropped_text; out[7] = chunk_bytes;
    }
};

inline int chunk_failure(const ChunkResult& r, uint64_t member0, std::string& err, uint64_t file_off = 0) {
    if (r.err == (uint32_t)-1) { err = "libbsk: gzip: the input is not gzip"; return FAIL_NOT_GZIP; }
    const int code = r.err == (uint32_t)ERR_MARKER ? (int)bgzf::ERR_DISTANCE : (int)r.err;
    err = where(member0 + r.members, file_off + r.err_bit / 8u) + error_text(code);
    return FAIL_FORMAT;
}

// A buffer that is a segment of a file (gzip_stream.hpp): what the chain is told of the file in front of the buffer, how the
// segment may end, and how it did end
struct SegmentEnds {
    int64_t open_at = 0;        // the text offset at which the open member began, from the segment's first text byte (<= 0)
    uint64_t members = 0;       // the members in front
    uint64_t file_off = 0;      // the file offset of the buffer: messages name offsets of the whole file
    bool more = false;          // the file goes on behind the buffer: a chain chunk that runs into the buffer's end ends the segment
    uint64_t text_cap = ~0ull;  // the chain is cut in front of the chunk that would bring the segment's text above this (not chunk 0)
    // out
    uint64_t next = NONE;       // the chunk whose start is the next resume point; NONE: the segment ends the file
    bool grow = false;          // chunk 0 itself did not land inside the buffer: nothing was decoded
};

// the chain from chunk 0 by "landed on"; res[k].land == NONE and no error: the chunk had no candidate and was not run
inline int walk_chain(const std::vector<uint64_t>& cand, const std::vector<ChunkResult>& res, uint64_t chunk_bytes, std::vector<ChainChunk>& chain,
                      Plan& plan, std::string& err, SegmentEnds* seg = nullptr) {
    plan = Plan();
    plan.chunks = res.size();
    plan.chunk_bytes = chunk_bytes;
    uint64_t all_text = 0;
    for (size_t k = 1; k < cand.size(); ++k)
        if (cand[k] != NONE) {
            ++plan.with_candidate;
            all_text += res[k].text;
        }
    uint64_t text = 0, members = seg ? seg->members : 0;
    int64_t open_at = seg ? seg->open_at : 0;  // text offset at which the member began that is open now
    for (uint64_t c = 0;;) {
        const ChunkResult& r = res[c];
        // a segment of a file ends in front of the chunk that meets the end of the buffer -- inside a block (truncated) or behind a
        // trailer, where the next member cannot be resumed at -- and in front of the one that brings too much text
        if (seg && ((seg->more && (r.err == (uint32_t)bgzf::ERR_TRUNCATED || (!r.err && r.land == LAND_END))) || (c != 0 && !r.err && text + r.text > seg->text_cap))) {
            if (c == 0) { seg->grow = true; return FAIL_NONE; }
            seg->next = c;
            break;
        }
        int64_t lo = open_at - ((int64_t)text - (int64_t)WIN);
        lo = lo < 0 ? 0 : lo > (int64_t)WIN ? (int64_t)WIN : lo;
        chain.push_back(ChainChunk{c, text, r.text, members, r.members, (uint32_t)lo});
        if (r.err) return chunk_failure(r, members, err, seg ? seg->file_off : 0);
        if (r.mstart != NONE) open_at = (int64_t)(text + r.mstart);
        text += r.text;
        members += r.members;
        if (members > MAX_MEMBERS) {
            err = "libbsk: gzip: the file has more than " + std::to_string(MAX_MEMBERS) + " members (" + std::to_string(members) +
                  (r.land == LAND_END ? "" : " so far") + "); that many are not read";
            return FAIL_UNSUPPORTED;
        }
        if (r.land == LAND_END) break;
        c = r.land;  // (always a later chunk: the walk ends)
    }
    if (seg) seg->open_at = open_at;  // (as the segment leaves it: from ITS first text byte)
    plan.on_chain = chain.size();
    plan.off_chain = plan.with_candidate - (plan.on_chain - 1);
    plan.members = members;
    plan.text = text;
    uint64_t kept = 0;
    for (size_t i = 1; i < chain.size(); ++i) kept += chain[i].text;
    plan.dropped_text = all_text - kept;
    return FAIL_NONE;
}

// the CRC pieces of the members: at most PIECE bytes, never across a member's end
inline void crc_pieces(const std::vector<MemberRec>& mem, std::vector<Piece>& pieces) {
    uint64_t at = 0;
    for (size_t m = 0; m < mem.size(); ++m) {
        for (; at < mem[m].text_end; ) {
            const uint64_t len = mem[m].text_end - at < PIECE ? mem[m].text_end - at : PIECE;
            pieces.push_back(Piece{at, (uint32_t)len, (uint32_t)m});
            at += len;
        }
    }
}

// every member's CRC32 from its pieces' and its length against the trailer.  ISIZE is the length modulo 2^32
// A segment of a file (gzip_stream.hpp): what the member that is open at its start has behind it, and -- afterwards -- what the
// member that is open at its end has; mem then holds one record more than members end in the segment, whose text_end is the
// segment's and which is not compared
struct OpenMember {
    uint64_t member0 = 0, file_off = 0;  // members and bytes of the file in front of the segment
    uint32_t crc = 0;
    uint64_t len = 0;
};
inline int check_members(const std::vector<MemberRec>& mem, const std::vector<Piece>& pieces, const std::vector<uint32_t>& piece_crc, std::string& err,
                         OpenMember* open = nullptr) {
    static const CrcAdvance A;
    size_t pi = 0;
    uint64_t begin = 0;
    const uint64_t member0 = open ? open->member0 : 0, file_off = open ? open->file_off : 0;
    for (size_t m = 0; m < mem.size(); ++m) {
        uint32_t crc = open && m == 0 ? open->crc : 0;
        for (; pi < pieces.size() && pieces[pi].member == m; ++pi) crc = A.advance(crc, pieces[pi].len) ^ piece_crc[pi];
        const uint64_t len = mem[m].text_end - begin + (open && m == 0 ? open->len : 0);
        begin = mem[m].text_end;
        if (open && m + 1 == mem.size()) {
            open->crc = crc;
            open->len = len;
            break;
        }
        if ((uint32_t)len != mem[m].isize) {
            err = where(member0 + m, file_off + mem[m].trailer) + bgzf::error_text((uint32_t)len < mem[m].isize ? bgzf::ERR_SHORT : bgzf::ERR_OVERRUN) + " (the member has " +
                  std::to_string(len) + " bytes, ISIZE says " + std::to_string(mem[m].isize) + ")";
            return FAIL_FORMAT;
        }
        if (crc != mem[m].crc) {
            err = where(member0 + m, file_off + mem[m].trailer) + bgzf::error_text(bgzf::ERR_CRC);
            return FAIL_FORMAT;
        }
    }
    return FAIL_NONE;
}

// ---- the host's lane
struct HostLane {
    static constexpr uint32_t LANES = 1;
    const uint8_t* comp;
    uint64_t n;
    uint32_t lane() const { return 0; }
    void sync() const {}
    uint32_t uni(uint32_t v) const { return v; }
    uint64_t uni64(uint64_t v) const { return v; }
    uint64_t vec64(uint64_t v) const { return v; }
    uint32_t word(uint64_t w) const {
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; ++k)
            if (w < (n + 3) / 4 && 4 * w + k < n) v |= (uint32_t)comp[4 * w + k] << (8 * k);
        return v;
    }
    uint8_t in_byte(uint64_t a) const { return comp[a]; }
    void store(const uint16_t* ring, uint16_t* out, uint32_t shift, uint64_t a, uint64_t b) const {
        for (uint64_t q = a; q < b; ++q) out[q] = ring[(shift + (uint32_t)q) & RING_MASK];
    }
};

// S_k of chunk k >= 1: the lowest hit (one lane: a scan that stops at it)
inline uint64_t find_host(const uint8_t* comp, uint64_t n, uint64_t chunk_bytes, uint64_t k) {
    const HostLane io{comp, n};
    auto word = [&](uint64_t w) { return io.word(w); };
    const uint64_t lo = k * chunk_bytes * 8u, hi = (k + 1) * chunk_bytes < n ? (k + 1) * chunk_bytes * 8u : n * 8u;
    for (uint64_t pos = lo; pos < hi; ++pos)
        if (header_ok(word, n * 8u, pos)) return pos;
    return NONE;
}

// the W of the chain chunks: W[i * WIN + m] is the text byte at chain[i].text_off - WIN + m (0 in front of the text)
// (carried: the window of a segment that is re-entered, in place of the zeros in front of a file)
inline void windows_host(const std::vector<ChainChunk>& chain, const uint16_t* sym, uint8_t* W, const uint8_t* carried = nullptr) {
    for (size_t j = 0; j < chain.size(); ++j) {
        uint8_t* Wj = W + j * (size_t)WIN;
        if (j == 0) { for (uint32_t m = 0; m < WIN; ++m) Wj[m] = carried ? carried[m] : 0; continue; }
        const uint8_t* Wi = Wj - WIN;
        const int64_t start_i = (int64_t)chain[j - 1].text_off, start_j = (int64_t)chain[j].text_off;
        for (uint32_t m = 0; m < WIN; ++m) {
            const int64_t pos = start_j - (int64_t)WIN + m;
            if (pos >= start_i) {
                const uint16_t s = sym[pos];
                Wj[m] = s < 0x8000u ? (uint8_t)s : Wi[s & 0x7FFFu];
            } else {
                Wj[m] = Wi[pos - start_i + (int64_t)WIN];  // (chunk i produced less than the window; the index is >= start_j - start_i)
            }
        }
    }
}

// The whole method with one lane.  chunk_bytes 0: one piece.  text.size() is the size of the text
inline int inflate_host(const uint8_t* comp, uint64_t n, uint64_t chunk_bytes, std::vector<uint8_t>& text, Plan& plan, std::string& err) {
    text.clear();
    plan = Plan();
    if (n == 0) return FAIL_NONE;
    Geometry G = geometry(n, chunk_bytes, nullptr);
    chunk_bytes = G.chunk_bytes;
    const uint64_t nchunks = G.nchunks;
    std::vector<uint64_t> cand(nchunks, NONE);
    G.cand = cand.data();
    for (uint64_t k = 1; k < nchunks; ++k) cand[k] = find_host(comp, n, chunk_bytes, k);
    std::vector<ChunkResult> res(nchunks, ChunkResult{NONE, 0, NONE, 0, 0, 0});
    GzDecodeLds* lds = new GzDecodeLds;
    struct Free { GzDecodeLds* p; ~Free() { delete p; } } guard{lds};
    for (uint64_t k = 0; k < nchunks; ++k) {
        if (k && cand[k] == NONE) continue;
        HostLane io{comp, n};
        lds->T.park = Parked{G, k, 0, k ? NONE : 0, nullptr, nullptr, 0};
        Walker<HostLane, false> Wk(io, lds->T, nullptr);
        res[k] = Wk.run(0);
    }
    std::vector<ChainChunk> chain;
    int rc = walk_chain(cand, res, chunk_bytes, chain, plan, err);
    if (rc) return rc;
    std::vector<uint16_t> sym(plan.text + 8);
    std::vector<MemberRec> mem(plan.members);
    for (const ChainChunk& c : chain) {
        HostLane io{comp, n};
        lds->T.park = Parked{G, c.k, c.text, c.k ? NONE : 0, mem.data() + c.member0, sym.data() + c.text_off, c.members};
        Walker<HostLane, true> Wk(io, lds->T, lds->ring);
        const ChunkResult r = Wk.run((uint32_t)(c.text_off & 7u));
        if (r.err) return chunk_failure(r, c.member0, err);
        if (r.members != c.members || r.text != c.text) { err = "libbsk: gzip: the decode of chunk " + std::to_string(c.k) + " does not repeat its size pass"; return FAIL_FORMAT; }
        for (uint32_t m = 0; m < c.members; ++m) mem[c.member0 + m].text_end += c.text_off;
    }
    std::vector<uint8_t> W(chain.size() * (size_t)WIN);
    windows_host(chain, sym.data(), W.data());
    text.resize(plan.text);
    for (size_t j = 0; j < chain.size(); ++j) {
        const ChainChunk& c = chain[j];
        for (uint64_t q = c.text_off; q < c.text_off + c.text; ++q) {
            const uint16_t s = sym[q];
            if (s < 0x8000u) { text[q] = (uint8_t)s; continue; }
            if ((s & 0x7FFFu) < c.marker_lo) {
                err = where(c.member0, cand[c.k] / 8u) + error_text((int)bgzf::ERR_DISTANCE) + " (in chunk " + std::to_string(c.k) + ")";
                return FAIL_FORMAT;
            }
            text[q] = W[j * (size_t)WIN + (s & 0x7FFFu)];
        }
    }
    std::vector<Piece> pieces;
    crc_pieces(mem, pieces);
    std::vector<uint32_t> pcrc(pieces.size());
    uint32_t tab[256];
    for (uint32_t i = 0; i < 256; ++i) tab[i] = bgzf::crc_table_entry(i);
    for (size_t i = 0; i < pieces.size(); ++i) {
        uint32_t c = 0xFFFFFFFFu;
        for (uint32_t q = 0; q < pieces[i].len; ++q) c = tab[(c ^ text[pieces[i].off + q]) & 255u] ^ (c >> 8);
        pcrc[i] = ~c;
    }
    return check_members(mem, pieces, pcrc, err);
}
}  // namespace gz
}  // namespace bsk
