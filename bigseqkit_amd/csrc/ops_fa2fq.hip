// ============================================================================
// ops_fa2fq.hip -- Fa2Fq.Call (bigseqkit-lib/fa2fq.go:59-120, as decided in PARITY.md FA2FQ) on the
// record table: join on the ID, search on both strands, sliced FASTQ record out.
//   k_fa2fq_match      : one lane per record.  FNV-1a of the ID, probe, byte verification (the membership test of a Go
//                        map), then bytes.Index of the FASTA sequence in the read, 8 bytes per compare.  The '-' strand is
//                        searched on the forward text: position p matches when complement(reverse(text[p, p + m))) is the
//                        needle, and the FIRST hit in the reversed read is the LAST such p, so p runs downwards.
//                        A read that leaves more than FA2FQ_LANE_POS start positions is listed instead.
//   k_fa2fq_match_wave : one wave per listed record: 64 start positions per step, the first lane that matches wins.
//   k_fa2fq_emit       : every output byte is a function of (record, offset): '@' ID '\n' slice '\n' '+' '\n' slice '\n',
//                        the '-' strand slices reversed (and the bases mapped through the complement in LDS).
// ============================================================================
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "ops_fa2fq.hpp"
#include "pattern_match_dev.hpp"  // fnv1a64, id_span_rec (text_dev.hpp)

namespace bsk {

namespace {

struct FqRec {
    const uint8_t* id;
    uint32_t id_len;
    const uint8_t* seq;
    const uint8_t* qual;
    uint32_t L;
};

__device__ __forceinline__ FqRec fq_rec(const uint8_t* buf, const RecordTable& t, uint64_t i, const Fa2FqParams& P) {
    FqRec r;
    const uint64_t s = t.start[i];
    const uint32_t lh = t.l_head[i];
    const uint8_t* head = buf + s + 1;
    uint32_t off;
    r.id_len = id_span_rec(t, i, head, lh > 0 ? lh - 1 : 0, P.id_mode, &off, P.buf_end);
    r.id = head + off;
    r.seq = buf + s + lh + 1;
    r.L = t.l_seq[i];
    r.qual = r.seq + r.L + 1 + t.aux[i] + 1;
    return r;
}

// entry of the FASTA table whose full name is the ID, or -1
__device__ int64_t fa_lookup(const Fa2FqParams& P, const uint8_t* id, uint32_t id_len) {
    const uint64_t key = fnv1a64(id, id_len, false);
    for (uint64_t slot = key & P.mask;; slot = (slot + 1) & P.mask) {
        const uint64_t sk = P.keys[slot];
        if (sk == 0) return -1;
        if (sk != key) continue;
        const uint32_t e = P.idx[slot];
        const uint64_t o = P.name_off[e];
        if (P.name_off[e + 1] - o != id_len) continue;
        bool ok = true;
        for (uint32_t q = 0; q < id_len; ++q)
            if (id[q] != P.names[o + q]) { ok = false; break; }
        if (ok) return (int64_t)e;
    }
}

// tx[0, m) == nd[0, m); both lie inside their blocks (the text inside the read)
__device__ __forceinline__ bool eq_plus(const uint8_t* tx, const uint8_t* nd, uint32_t m) {
    uint32_t q = 0;
    for (; q + 8u <= m; q += 8u) {
        uint64_t a, b;
        __builtin_memcpy(&a, tx + q, 8);
        __builtin_memcpy(&b, nd + q, 8);
        if (a != b) return false;
    }
    for (; q < m; ++q)
        if (tx[q] != nd[q]) return false;
    return true;
}

// complement(reverse(tx[0, m))) == nd[0, m): the needle at this place of the reverse-complemented read
__device__ __forceinline__ bool eq_minus(const uint8_t* tx, const uint8_t* nd, uint32_t m, const uint8_t* lut) {
    if (m && lut[tx[m - 1u]] != nd[0]) return false;  // (most places end here, before eight map reads)
    uint32_t q = 0;
    for (; q + 8u <= m; q += 8u) {
        uint64_t a, b;
        __builtin_memcpy(&a, tx + (m - 8u - q), 8);
        __builtin_memcpy(&b, nd + q, 8);
        a = __builtin_bswap64(a);
        uint64_t x = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) x |= (uint64_t)lut[(a >> (8 * k)) & 0xFFu] << (8 * k);
        if (x != b) return false;
    }
    for (; q < m; ++q)
        if (lut[tx[m - 1u - q]] != nd[q]) return false;
    return true;
}

__global__ __launch_bounds__(256) void k_fa2fq_match(const uint8_t* __restrict__ buf, RecordTable t, Fa2FqParams P,
                                                     uint32_t* __restrict__ ent, uint32_t* __restrict__ pos,
                                                     uint32_t* __restrict__ out_len, uint32_t* __restrict__ list) {
    __shared__ uint8_t s_lut[256];
    for (int k = threadIdx.x; k < 256; k += blockDim.x) s_lut[k] = P.comp[k];
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.n) return;
    const FqRec r = fq_rec(buf, t, i, P);
    uint32_t v_ent = FA2FQ_NONE, v_pos = 0, v_len = 0;
    const int64_t e = fa_lookup(P, r.id, r.id_len);
    if (e >= 0) {
        const uint64_t so = P.seq_off[e];
        const uint64_t m64 = P.seq_off[e + 1] - so;
        const uint64_t n64 = (uint64_t)r.id_len + 2u * m64 + 6u;  // '@' ID '\n' slice '\n' '+' '\n' slice '\n'
        if (m64 <= r.L) {
            if (n64 > FA2FQ_RECORD_MAX) {
                atomicMin(&P.ctl[1], (unsigned long long)i);
            } else {
                const uint32_t m = (uint32_t)m64;
                const uint32_t npos = r.L - m + 1u;
                const uint8_t* nd = P.seqs + so;
                if (npos > FA2FQ_LANE_POS) {  // a wave searches this one
                    list[atomicAdd(&P.ctl[0], 1ull)] = (uint32_t)i;
                    v_ent = (uint32_t)e;
                    v_len = (uint32_t)n64;
                } else {
                    bool hit = false;
                    for (uint32_t p = 0; p < npos && !hit; ++p)
                        if (eq_plus(r.seq + p, nd, m)) { hit = true; v_ent = (uint32_t)e; v_pos = p; }
                    if (!hit && !P.only_plus) {
                        for (uint32_t p = npos; p-- > 0 && !hit;)
                            if (eq_minus(r.seq + p, nd, m, s_lut)) { hit = true; v_ent = (uint32_t)e | FA2FQ_MINUS; v_pos = r.L - m - p; }
                    }
                    if (hit) v_len = (uint32_t)n64;
                }
            }
        }
    }
    ent[i] = v_ent;
    pos[i] = v_pos;
    out_len[i] = v_len;
}

__global__ __launch_bounds__(256) void k_fa2fq_match_wave(const uint8_t* __restrict__ buf, RecordTable t, Fa2FqParams P,
                                                          uint32_t* __restrict__ ent, uint32_t* __restrict__ pos,
                                                          uint32_t* __restrict__ out_len, const uint32_t* __restrict__ list) {
    __shared__ uint8_t s_lut[256];
    for (int k = threadIdx.x; k < 256; k += blockDim.x) s_lut[k] = P.comp[k];
    __syncthreads();
    const uint64_t listed = P.ctl[0];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    for (uint64_t k = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; k < listed; k += waves) {
        const uint64_t i = list[k];
        const uint32_t e = ent[i];
        const uint64_t s = t.start[i];
        const uint8_t* seq = buf + s + t.l_head[i] + 1;
        const uint32_t L = t.l_seq[i];
        const uint64_t so = P.seq_off[e];
        const uint32_t m = (uint32_t)(P.seq_off[e + 1] - so);
        const uint8_t* nd = P.seqs + so;
        const uint32_t npos = L - m + 1u;  // (listed: m <= L and npos > FA2FQ_LANE_POS)
        uint32_t v_ent = FA2FQ_NONE, v_pos = 0;
        bool hit = false;
        for (uint64_t base = 0; base < npos && !hit; base += 64u) {
            const uint64_t p = base + lane;
            const bool ok = p < npos && eq_plus(seq + p, nd, m);
            const unsigned long long b = __ballot(ok);
            if (b) { hit = true; v_ent = e; v_pos = (uint32_t)(base + (uint64_t)__ffsll(b) - 1u); }
        }
        if (!hit && !P.only_plus) {
            for (uint64_t base = 0; base < npos && !hit; base += 64u) {
                const uint64_t back = base + lane;  // places counted from the end: the first lane holds the last place
                const bool ok = back < npos && eq_minus(seq + (npos - 1u - back), nd, m, s_lut);
                const unsigned long long b = __ballot(ok);
                if (b) {
                    hit = true;
                    v_ent = e | FA2FQ_MINUS;
                    v_pos = (uint32_t)(base + (uint64_t)__ffsll(b) - 1u);  // L - m - p with p = npos - 1 - back
                }
            }
        }
        if (lane == 0) {
            ent[i] = v_ent;
            pos[i] = v_pos;
            if (!hit) out_len[i] = 0;
        }
    }
}

constexpr uint32_t FA2FQ_LONG_CH = 64u * 1024u;  // output bytes per block of a record written by whole blocks

template <bool LONG>
__global__ __launch_bounds__(256) void k_fa2fq_emit(const uint8_t* __restrict__ buf, RecordTable t, Fa2FqParams P,
                                                    const uint32_t* __restrict__ ent, const uint32_t* __restrict__ pos,
                                                    const uint32_t* __restrict__ out_len, const uint64_t* __restrict__ out_off,
                                                    uint8_t* __restrict__ out, const uint32_t* __restrict__ long_list,
                                                    uint32_t long_thresh) {
    __shared__ uint8_t s_lut[256];
    for (int k = threadIdx.x; k < 256; k += blockDim.x) s_lut[k] = P.comp[k];
    __syncthreads();
    constexpr uint32_t LANES = LONG ? 256u : 16u;
    const uint64_t g = LONG ? (uint64_t)long_list[blockIdx.y] : ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / 16u;
    const uint32_t gl = LONG ? threadIdx.x : threadIdx.x % 16u;
    if (g >= t.n) return;
    const uint32_t n = out_len[g];
    if (n == 0) return;
    if (!LONG && long_thresh && n >= long_thresh) return;  // written by the LONG launch
    const uint32_t clo = LONG ? blockIdx.x * FA2FQ_LONG_CH : 0u;  // this block's slice [clo, chi) of the record's output
    if (clo >= n) return;
    const uint32_t chi = LONG ? (n - clo < FA2FQ_LONG_CH ? n : clo + FA2FQ_LONG_CH) : n;
    auto first_step = [&](uint32_t off) -> uint32_t { return clo > off ? ((clo - off) & ~15u) : 0u; };
    auto last_byte = [&](uint32_t off, uint32_t nb) -> uint32_t { return chi < off ? 0u : (chi - off < nb ? chi - off : nb); };
    auto mine = [&](uint32_t x) -> bool { return x >= clo && x < chi; };
    uint8_t* o = out + out_off[g];
    const FqRec r = fq_rec(buf, t, g, P);
    const bool minus = (ent[g] & FA2FQ_MINUS) != 0u;
    const uint32_t m = (n - r.id_len - 6u) / 2u;
    const uint32_t at = pos[g];
    const uint32_t a = 1u + r.id_len + 1u;  // bytes of the header line
    // header: '@' ID '\n'
    for (uint32_t x = clo + gl; x < (a < chi ? a : chi); x += LANES) o[x] = x == 0 ? '@' : (x == a - 1u ? '\n' : r.id[x - 1u]);
    // a slice of m bytes at output offset `off`: src[at, at + m) of the read, or the same span of the reversed read
    auto slice = [&](uint32_t off, const uint8_t* src, bool map) {
        uint8_t* dst = o + off;
        // (reversed read: its bytes [at, at + m) are the read's [L - at - m, L - at) backwards)
        const uint8_t* from = minus ? src + (r.L - at - m) : src + at;
        const uint32_t hi = last_byte(off, m);
        for (uint32_t x0 = first_step(off) + gl * 16u; x0 < hi; x0 += LANES * 16u) {
            // the last, partial step of a slice of 16 bytes or more is taken 16 wide from the slice's end (same bytes twice)
            const uint32_t x = (!LONG && x0 + 16u > m && m >= 16u) ? m - 16u : x0;
            if (x + 16u <= m) {
                uint4 v;
                __builtin_memcpy(&v, from + (minus ? m - 16u - x : x), 16);
                uint32_t w[4] = {v.x, v.y, v.z, v.w};
                if (minus) {
                    const uint32_t r0 = __builtin_bswap32(w[3]), r1 = __builtin_bswap32(w[2]), r2 = __builtin_bswap32(w[1]),
                                   r3 = __builtin_bswap32(w[0]);
                    w[0] = r0; w[1] = r1; w[2] = r2; w[3] = r3;
                    if (map) {
#pragma unroll
                        for (int d = 0; d < 4; ++d)
                            w[d] = (uint32_t)s_lut[w[d] & 0xFFu] | ((uint32_t)s_lut[(w[d] >> 8) & 0xFFu] << 8) |
                                   ((uint32_t)s_lut[(w[d] >> 16) & 0xFFu] << 16) | ((uint32_t)s_lut[w[d] >> 24] << 24);
                    }
                }
                const uint4 ov = make_uint4(w[0], w[1], w[2], w[3]);
                __builtin_memcpy(dst + x, &ov, 16);
            } else {
                for (uint32_t k = x; k < m; ++k) {
                    const uint8_t c = minus ? from[m - 1u - k] : from[k];
                    dst[k] = (minus && map) ? s_lut[c] : c;
                }
            }
        }
    };
    slice(a, r.seq, true);
    const uint32_t q0 = a + m + 3u;
    if (gl == 0) {
        if (mine(a + m)) o[a + m] = '\n';
        if (mine(a + m + 1u)) o[a + m + 1u] = '+';
        if (mine(a + m + 2u)) o[a + m + 2u] = '\n';
        if (mine(q0 + m)) o[q0 + m] = '\n';
    }
    slice(q0, r.qual, false);
}

}  // namespace

hipError_t launch_fa2fq_match(const uint8_t* buf, const RecordTable& t, const Fa2FqParams& P, uint32_t* ent, uint32_t* pos,
                              uint32_t* out_len, uint32_t* list, hipStream_t st) {
    if (t.n == 0) return hipSuccess;
    const uint64_t blocks = (t.n + 255) / 256;
    hipLaunchKernelGGL(k_fa2fq_match, dim3((unsigned)blocks), dim3(256), 0, st, buf, t, P, ent, pos, out_len, list);
    // (the number of listed records is only known on the device: a fixed grid walks the list)
    const uint64_t wblocks = std::min<uint64_t>((t.n + 3) / 4, 2048);
    hipLaunchKernelGGL(k_fa2fq_match_wave, dim3((unsigned)wblocks), dim3(256), 0, st, buf, t, P, ent, pos, out_len, list);
    return hipGetLastError();
}

hipError_t launch_fa2fq_emit(const uint8_t* buf, const RecordTable& t, const Fa2FqParams& P, const uint32_t* ent,
                             const uint32_t* pos, const uint32_t* out_len, const uint64_t* out_off, uint8_t* out,
                             const uint32_t* long_list, uint64_t long_count, uint64_t long_max, uint32_t long_thresh,
                             hipStream_t st) {
    if (t.n == 0) return hipSuccess;
    if (!(long_list && long_count)) long_thresh = 0u;
    const uint64_t blocks = (t.n * 16 + 255) / 256;
    hipLaunchKernelGGL((k_fa2fq_emit<false>), dim3((unsigned)blocks), dim3(256), 0, st, buf, t, P, ent, pos, out_len, out_off, out,
                       long_list, long_thresh);
    if (long_thresh) {
        const unsigned chunks = (unsigned)((long_max + FA2FQ_LONG_CH - 1) / FA2FQ_LONG_CH);
        hipLaunchKernelGGL((k_fa2fq_emit<true>), dim3(chunks, (unsigned)long_count), dim3(256), 0, st, buf, t, P, ent, pos, out_len,
                           out_off, out, long_list, long_thresh);
    }
    return hipGetLastError();
}

}  // namespace bsk
