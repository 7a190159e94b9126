// `faidx -d`: one tile of the indexed fetch, the same source for the kernel (ops_faidx_fetch.hip, 256 lanes per tile) and
// for the host (bsk_faidx_fetch_host, tests/host_c/fai_fetch_check.cpp, 1 lane).  PARITY.md FAIX, DESIGN.md f21.
//
// A hit is the region [p0, p1) of an index row (length, offset, linebases; linewidth = linebases + 1, the planner refuses
// every other row).  Base p of the record lies at  offset + (p / linebases) * linewidth + p % linebases  of the file.  The
// file bytes that the plan read stand in one buffer; FetchHit::src is the place that the record's first base has (or would
// have: the buffer holds only the lines of the region) in it, FetchHit::eof the place of the end of the file.
//
// Work is cut by OUTPUT: a tile is FETCH_T consecutive output bases of one hit.  Its source bytes are one contiguous range
// (ascending for either strand), brought into the lanes' shared memory with aligned 16-byte loads; every lane then owns runs
// of FETCH_RUN consecutive output bases -- one division for the source column and one for the output column at the start
// of a run, then steps -- and writes them, wrapped at LineWidth, into a shared image of the tile's output, laid out so that
// image and output agree modulo 16: the image leaves with aligned 16-byte stores, byte stores only at its two edges.
//
// Check 1 of FAIX: every byte of every line that is read is judged -- columns 0 .. linebases-1 are no '\n', column
// linebases is one; behind the bases of the record's last line stands '\n' or the end of the file.  The tile's own bytes are
// judged in shared memory; the first tile of a hit also judges the part of the first line in front of the region, the tile
// that holds base p1 - 1 the rest of the last line (both straight from the buffer: they can be longer than a tile).  A
// violation leaves  tile << 32 | byte offset behind the tile's first judged byte  in the status word, the lowest one wins.
//
// A policy P says what a lane is:
//     LANES             256 on the device, 1 on the host
//     lane() sync()     this lane's number / a barrier of the tile's lanes
//     load16(i)         the aligned 16 bytes at buffer index i (a multiple of 16; the buffer is padded to one)
//     byte(i)           one byte of the buffer
//     store16(o, v) store8(o, b)   the aligned 16 bytes / one byte at output offset o
//     fail(word)        status = min(status, word)
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FAI_HD __host__ __device__ __forceinline__
#else
#define FAI_HD inline
#endif

namespace bsk {
namespace fai {

constexpr uint32_t FETCH_T = 4096;      // output bases of a tile
constexpr uint32_t FETCH_RUN = 16;      // consecutive output bases of a lane
constexpr uint32_t FETCH_IN_BYTES = 2 * FETCH_T + 32;   // linebases 1: T bases and T - 1 newlines, 15 bytes of alignment
constexpr uint32_t FETCH_OUT_BYTES = 2 * FETCH_T + 32;  // LineWidth 1: T bases and T newlines, 15 bytes of alignment
constexpr uint64_t FETCH_NO_FAULT = ~0ull;

struct Vec16 { uint32_t w[4]; };

struct FetchHit {
    uint64_t src;        // buffer index of the record's first base (modulo 2^64: lines in front of the region are not there)
    uint64_t eof;        // buffer index of the end of the file, by the same arithmetic
    uint64_t out;        // output offset of the hit's '>'
    uint64_t hdr;        // where ">name[:b-e]\n" stands among the header texts
    uint32_t hdr_len;
    uint32_t length, linebases;
    uint32_t p0, p1;     // the region, 0-based half-open; p0 < p1 <= length
    uint32_t minus;      // reverse complement
    uint32_t tile0;      // the hit's first tile
    uint32_t pad_;
};
struct FetchTile { uint32_t hit, q0; };  // output bases [q0, q0 + FETCH_T) of the hit, cut at its end

struct FetchShared {  // what the lanes of a tile share: LDS on the device
    alignas(16) uint8_t in[FETCH_IN_BYTES];
    alignas(16) uint8_t img[FETCH_OUT_BYTES];
    uint8_t comp[256];
};

FAI_HD uint64_t wrapped_len64(uint64_t L, uint32_t w) { return (w < 1 || L == 0) ? L : L + (L - 1) / w; }
// place of base p behind the record's first base
FAI_HD uint64_t base_at(const FetchHit& h, uint32_t p) { return (uint64_t)(p / h.linebases) * ((uint64_t)h.linebases + 1) + p % h.linebases; }
// bases on line `line` of the record
FAI_HD uint32_t line_bases(const FetchHit& h, uint64_t line) {
    const uint64_t left = (uint64_t)h.length - line * h.linebases;
    return left < h.linebases ? (uint32_t)left : h.linebases;
}
// output offset of base k behind the header (k == n: one past the final newline)
FAI_HD uint64_t out_pos(uint32_t k, uint32_t n, uint32_t w) {
    if (k >= n) return wrapped_len64(n, w) + 1;
    return (uint64_t)k + (w ? k / w : 0u);
}

// what a tile reads and judges, in places behind the record's first base (add FetchHit::src for buffer indices)
struct TileGeo {
    uint32_t q1, sb0, sb1;   // output bases [q0, q1) = source bases [sb0, sb1)
    uint64_t c_lo, c_hi;     // the tile's own bytes: first base through last base
    uint64_t j_lo, j_hi;     // judged: c_lo / c_hi, extended to the line start in the first tile, through the newline that ends
                             // the line of p1 - 1 in the tile that holds it, through a newline right behind c_hi otherwise
};
FAI_HD TileGeo tile_geo(const FetchHit& h, uint32_t q0) {
    TileGeo g;
    const uint32_t n = h.p1 - h.p0;
    g.q1 = n - q0 > FETCH_T ? q0 + FETCH_T : n;
    g.sb0 = h.minus ? h.p1 - g.q1 : h.p0 + q0;
    g.sb1 = h.minus ? h.p1 - q0 : h.p0 + g.q1;
    g.c_lo = base_at(h, g.sb0);
    g.c_hi = base_at(h, g.sb1 - 1) + 1;
    const uint64_t lw = (uint64_t)h.linebases + 1;
    g.j_lo = g.sb0 == h.p0 ? (g.c_lo / lw) * lw : g.c_lo;
    if (g.sb1 == h.p1) {
        const uint64_t line = (g.c_hi - 1) / lw;  // the line of base p1 - 1
        g.j_hi = line * lw + line_bases(h, line) + 1;
    } else {
        g.j_hi = base_at(h, g.sb1);  // behind a newline when base sb1 begins a line
    }
    return g;
}

// is byte b at place x (behind the record's first base) what the index predicts?
FAI_HD bool byte_ok(const FetchHit& h, uint64_t line, uint32_t col, uint8_t b, bool at_eof) {
    const uint32_t nb = line_bases(h, line);
    if (col < nb) return !at_eof && b != '\n';
    if (at_eof) return (line + 1) * h.linebases >= h.length;  // only behind the record's last line
    return b == '\n';
}

template <class P>
FAI_HD void judge_far(P& p, const FetchHit& h, uint64_t lo, uint64_t hi, uint64_t j_lo, uint32_t tile) {
    // [lo, hi) straight from the buffer: runs of 16 bytes per lane, one division per run
    const uint64_t lw = (uint64_t)h.linebases + 1;
    for (uint64_t r = lo + (uint64_t)p.lane() * 16; r < hi; r += (uint64_t)P::LANES * 16) {
        uint64_t line = r / lw;
        uint32_t col = (uint32_t)(r % lw);
        const uint64_t e = hi - r < 16 ? hi : r + 16;
        for (uint64_t x = r; x < e; ++x) {
            const bool at_eof = h.src + x >= h.eof;
            const uint8_t b = at_eof ? 0 : p.byte(h.src + x);
            if (!byte_ok(h, line, col, b, at_eof)) {
                const uint64_t off = x - j_lo;
                p.fail((uint64_t)tile << 32 | (off > 0xFFFFFFFFull ? 0xFFFFFFFFull : off));
            }
            if (++col == lw) { col = 0; ++line; }
        }
    }
}

template <class P>
FAI_HD void fetch_tile(P& p, FetchShared& S, const FetchHit& h, uint32_t tile, uint32_t q0, uint32_t line_width,
                       const uint8_t* comp, const uint8_t* headers) {
    const TileGeo g = tile_geo(h, q0);
    const uint32_t n = h.p1 - h.p0;
    const uint32_t w = line_width;
    const uint64_t lw = (uint64_t)h.linebases + 1;
    // ---- the tile's bytes into shared memory, aligned 16-byte loads (the buffer is padded: no load leaves it)
    const uint64_t b_lo = h.src + g.c_lo, b_hi = h.src + g.c_hi;
    const uint64_t a_lo = b_lo & ~15ull;
    const uint32_t nvec = (uint32_t)((b_hi - a_lo + 15) / 16);
    for (uint32_t i = p.lane(); i < nvec; i += P::LANES) *reinterpret_cast<Vec16*>(S.in + 16 * i) = p.load16(a_lo + 16ull * i);
    if (h.minus)
        for (uint32_t i = p.lane(); i < 256; i += P::LANES) S.comp[i] = comp[i];
    // the header, by the hit's first tile
    if (q0 == 0)
        for (uint32_t i = p.lane(); i < h.hdr_len; i += P::LANES) p.store8(h.out + i, headers[h.hdr + i]);
    p.sync();
    const uint32_t in0 = (uint32_t)(b_lo - a_lo);  // S.in[in0] is the byte at place c_lo
    // ---- check 1 on the bytes in shared memory: runs of consecutive bytes, one division per run
    {
        const uint32_t len = (uint32_t)(g.c_hi - g.c_lo);
        for (uint32_t r = p.lane() * FETCH_RUN; r < len; r += P::LANES * FETCH_RUN) {
            const uint64_t x0 = g.c_lo + r;
            uint64_t line = x0 / lw;
            uint32_t col = (uint32_t)(x0 % lw);
            const uint32_t e = len - r < FETCH_RUN ? len : r + FETCH_RUN;
            for (uint32_t i = r; i < e; ++i) {
                const bool at_eof = b_lo + i >= h.eof;
                if (!byte_ok(h, line, col, S.in[in0 + i], at_eof)) {
                    const uint64_t off = (g.c_lo - g.j_lo) + i;
                    p.fail((uint64_t)tile << 32 | (off > 0xFFFFFFFFull ? 0xFFFFFFFFull : off));
                }
                if (++col == lw) { col = 0; ++line; }
            }
        }
        if (g.j_lo < g.c_lo) judge_far(p, h, g.j_lo, g.c_lo, g.j_lo, tile);
        if (g.c_hi < g.j_hi) judge_far(p, h, g.c_hi, g.j_hi, g.j_lo, tile);
    }
    // ---- the output image: img[og + (o - o_lo)] is output byte o of the hit's body
    const uint64_t body = h.out + h.hdr_len;
    const uint64_t o_lo = out_pos(q0, n, w), o_hi = out_pos(g.q1, n, w);
    const uint32_t og = (uint32_t)((body + o_lo) & 15);
    for (uint32_t r = p.lane(); r * FETCH_RUN < g.q1 - q0; r += P::LANES) {
        const uint32_t k0 = q0 + r * FETCH_RUN;
        const uint32_t k1 = g.q1 - k0 < FETCH_RUN ? g.q1 : k0 + FETCH_RUN;
        const uint32_t s = h.minus ? h.p1 - 1 - k0 : h.p0 + k0;
        uint32_t col = s % h.linebases;
        uint32_t li = in0 + (uint32_t)(base_at(h, s) - g.c_lo);
        uint32_t ow = w ? k0 % w : 0;
        uint32_t oi = og + (uint32_t)(out_pos(k0, n, w) - o_lo);
        for (uint32_t k = k0; k < k1; ++k) {
            uint8_t b = S.in[li];
            if (h.minus) b = S.comp[b];
            S.img[oi++] = b;
            if (k + 1 == n) S.img[oi++] = '\n';
            else if (w && ++ow == w) { S.img[oi++] = '\n'; ow = 0; }
            if (h.minus) {
                if (col == 0) { col = h.linebases - 1; li -= 2; } else { --col; --li; }
            } else {
                if (++col == h.linebases) { col = 0; li += 2; } else ++li;
            }
        }
    }
    p.sync();
    // ---- the image leaves: bytes up to the first 16-byte boundary of the output, whole vectors, bytes behind the last one
    const uint64_t g_lo = body + o_lo, g_hi = body + o_hi;
    uint64_t v_lo = (g_lo + 15) & ~15ull, v_hi = g_hi & ~15ull;
    if (v_lo > v_hi) { v_lo = g_hi; v_hi = g_hi; }
    for (uint64_t o = g_lo + p.lane(); o < v_lo; o += P::LANES) p.store8(o, S.img[og + (uint32_t)(o - g_lo)]);
    for (uint64_t o = v_lo + 16ull * p.lane(); o < v_hi; o += 16ull * P::LANES)
        p.store16(o, *reinterpret_cast<const Vec16*>(S.img + og + (uint32_t)(o - g_lo)));
    for (uint64_t o = v_hi + p.lane(); o < g_hi; o += P::LANES) p.store8(o, S.img[og + (uint32_t)(o - g_lo)]);
    p.sync();  // (the next tile of this block writes the shared memory again)
}

}  // namespace fai
}  // namespace bsk
