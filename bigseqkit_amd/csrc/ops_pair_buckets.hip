// `pair` in buckets of the key: what a match bucket decides, the rank step and the table passes of the order buckets (see
// ops_pair_buckets.hpp).  The comparison has the shape of k_renb_verify (ops_rename_buckets.hip): 32 records per block, 8 lanes
// each, the lanes of a record meet in one LDS word.  Everything else is one lane per record, or per word of a bitmap.
#include <hip/hip_runtime.h>

#include "bucket_hist_dev.hpp"
#include "ops_pair_buckets.hpp"
#include "ops_records.hpp"  // ERR_RECORD_TOO_LARGE
#include "record_text_dev.hpp"

namespace bsk {
namespace {

constexpr uint32_t CMP_LANES = 8;         // lanes per record of the comparison
constexpr uint32_t CMP_STEP = 16u * CMP_LANES;

__device__ __forceinline__ bool bit_of(const uint32_t* __restrict__ bits, uint64_t g) {
    return (bits[g >> 5] >> (uint32_t)(g & 31u)) & 1u;
}
__device__ __forceinline__ void set_bit(uint32_t* __restrict__ bits, uint64_t g) {
    atomicOr(&bits[g >> 5], 1u << (uint32_t)(g & 31u));  // (two records of a bucket can share a word)
}
// the set bits in front of bit g
__device__ __forceinline__ uint64_t rank_of(const uint32_t* __restrict__ bits, const uint16_t* __restrict__ wpre,
                                            const uint64_t* __restrict__ base, uint64_t g) {
    const uint64_t w = g >> 5;
    return base[w / PAIRB_RANK_WORDS] + wpre[w] + (uint64_t)__popc(bits[w] & ((1u << (uint32_t)(g & 31u)) - 1u));
}

// the members of a block take their places in the list with ONE atomic of the block: the order of the list is free, the sort
// behind it orders by (first, index)
__global__ __launch_bounds__(256) void k_pairb_verify(const uint8_t* __restrict__ acc, const uint64_t* __restrict__ a_off,
                                                      const uint32_t* __restrict__ a_len, const uint32_t* __restrict__ first,
                                                      uint64_t n, uint64_t* __restrict__ members,
                                                      unsigned long long* __restrict__ n_members, uint32_t* __restrict__ flagged,
                                                      uint32_t cap) {
    constexpr uint32_t PER_BLOCK = 256 / CMP_LANES;
    __shared__ uint32_t s_diff[PER_BLOCK];
    __shared__ uint32_t s_count;
    __shared__ unsigned long long s_base;
    const uint32_t grp = threadIdx.x / CMP_LANES, gl = threadIdx.x & (CMP_LANES - 1u);
    if (threadIdx.x < PER_BLOCK) s_diff[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * PER_BLOCK + grp;
    uint32_t f = 0;
    bool later = false;
    if (i < n) {
        f = first[i];
        later = f != i;
    }
    if (later) {
        const uint32_t la = a_len[i];
        uint32_t d = la ^ a_len[f];
        if (!d) {
            const uint8_t* pa = acc + a_off[i];
            const uint8_t* pb = acc + a_off[f];
            for (uint32_t q = 16u * gl; q + 16u <= la && !d; q += CMP_STEP) {
                uint4 x, y;
                __builtin_memcpy(&x, pa + q, 16);
                __builtin_memcpy(&y, pb + q, 16);
                d = (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
            }
            if (gl == 0u)
                for (uint32_t q = la & ~15u; q < la; ++q) d |= (uint32_t)(pa[q] ^ pb[q]);
        }
        if (d) atomicOr(&s_diff[grp], 1u);
    }
    __syncthreads();
    uint32_t slot = 0;
    bool member = false;
    if (i < n && gl == 0u) {
        if (later && s_diff[grp]) {
            const uint32_t pos = atomicAdd(&flagged[0], 1u);  // (the count stays exact beyond the cap)
            if (pos < cap) flagged[1 + pos] = (uint32_t)i;
        } else {  // the head of the group, or a record with its bytes
            member = true;
            slot = atomicAdd(&s_count, 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_count) s_base = atomicAdd(n_members, (unsigned long long)s_count);
    __syncthreads();
    if (member) members[s_base + slot] = ((uint64_t)f << 32) | (uint64_t)(uint32_t)i;
}

__global__ __launch_bounds__(256) void k_pairb_scatter(const uint8_t* __restrict__ state, const uint32_t* __restrict__ partner,
                                                       const uint64_t* __restrict__ a_gidx, uint64_t n, uint64_t n1,
                                                       uint32_t* __restrict__ bits1, uint32_t* __restrict__ bits2,
                                                       uint64_t* __restrict__ mates, unsigned long long* __restrict__ n_pairs) {
    __shared__ uint32_t s_pairs;
    if (threadIdx.x == 0) s_pairs = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const uint32_t s = state[i];
        const uint64_t g = a_gidx[i];
        if (s == 1u && g < n1) {
            set_bit(bits1, g);
            atomicAdd(&s_pairs, 1u);
        } else if (s == 2u && g >= n1) {
            set_bit(bits2, g - n1);
            mates[g - n1] = a_gidx[partner[i]];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_pairs) atomicAdd(n_pairs, (unsigned long long)s_pairs);
}

__global__ __launch_bounds__(256) void k_pairb_set(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, uint64_t m,
                                                   uint64_t n1, uint32_t* __restrict__ bits1, uint32_t* __restrict__ bits2,
                                                   uint64_t* __restrict__ mates) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const uint64_t ga = a[j], gb = b[j] - n1;
    set_bit(bits1, ga);
    set_bit(bits2, gb);
    mates[gb] = ga;
}

// one word per lane, one rank block per block of the grid: the inclusive scan of the popcounts in LDS (eight steps)
__global__ __launch_bounds__(256) void k_pairb_count(const uint32_t* __restrict__ bits, uint64_t words, uint16_t* __restrict__ wpre,
                                                     uint32_t* __restrict__ cnt) {
    static_assert(PAIRB_RANK_WORDS == 256, "one word per lane of the block");
    __shared__ uint32_t s_sum[PAIRB_RANK_WORDS];
    const uint64_t w = (uint64_t)blockIdx.x * PAIRB_RANK_WORDS + threadIdx.x;
    const uint32_t pc = w < words ? (uint32_t)__popc(bits[w]) : 0u;
    s_sum[threadIdx.x] = pc;
    __syncthreads();
    for (uint32_t d = 1; d < PAIRB_RANK_WORDS; d <<= 1) {
        const uint32_t v = threadIdx.x >= d ? s_sum[threadIdx.x - d] : 0u;
        __syncthreads();
        s_sum[threadIdx.x] += v;
        __syncthreads();
    }
    const uint32_t incl = s_sum[threadIdx.x];
    if (w < words) wpre[w] = (uint16_t)(incl - pc);  // (< 32 * 256)
    if (threadIdx.x == PAIRB_RANK_WORDS - 1u) cnt[blockIdx.x] = incl;
}

__global__ __launch_bounds__(256) void k_pairb_rank(const uint32_t* __restrict__ bits1, const uint16_t* __restrict__ wpre1,
                                                    const uint64_t* __restrict__ base1, const uint32_t* __restrict__ bits2,
                                                    const uint16_t* __restrict__ wpre2, const uint64_t* __restrict__ base2,
                                                    uint64_t n2, uint64_t* __restrict__ mates,
                                                    unsigned long long* __restrict__ n_disorder) {
    __shared__ uint32_t s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n2 && bit_of(bits2, j)) {
        const uint64_t pos = rank_of(bits1, wpre1, base1, mates[j]);
        mates[j] = pos;
        if (pos != rank_of(bits2, wpre2, base2, j)) atomicAdd(&s_bad, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_bad) atomicAdd(n_disorder, (unsigned long long)s_bad);
}

__global__ __launch_bounds__(256) void k_pairb_pos(uint64_t first, uint64_t count, uint64_t n1, const uint32_t* __restrict__ bits1,
                                                   const uint16_t* __restrict__ wpre1, const uint64_t* __restrict__ base1,
                                                   const uint32_t* __restrict__ bits2, const uint64_t* __restrict__ mates,
                                                   uint64_t* __restrict__ pos) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const uint64_t g = first + j;
    uint64_t p = ~0ull;
    if (g < n1) {
        if (bit_of(bits1, g)) p = rank_of(bits1, wpre1, base1, g);
    } else if (bit_of(bits2, g - n1)) {
        p = mates[g - n1];
    }
    pos[j] = p;
}

// bytes (text + '\n') and records per order bin (bucket_hist_dev.hpp): the bin of a paired record of file 2 is pos >> shift
__global__ __launch_bounds__(256) void k_pairb_order_hist(const uint8_t* __restrict__ buf, uint64_t buf_n, RecordTable t, int fastq,
                                                          uint64_t j0, const uint32_t* __restrict__ bits2,
                                                          const uint64_t* __restrict__ mates, uint32_t shift,
                                                          unsigned long long* __restrict__ g_bytes,
                                                          unsigned long long* __restrict__ g_records) {
    bucket_hist(t.n, g_bytes, g_records, [&](uint64_t i) {
        const uint64_t j = j0 + i;
        if (!bit_of(bits2, j)) return BinBytes{BUCKET_BINS, 0ull};  // (counted nowhere)
        const uint64_t bin = mates[j] >> shift;
        return BinBytes{(uint32_t)(bin < BUCKET_BINS ? bin : BUCKET_BINS), record_text_len(buf, buf_n, t, fastq, i) + 1u};
    });
}

__global__ __launch_bounds__(256) void k_pairb_order_pick(const uint8_t* __restrict__ buf, uint64_t buf_n, RecordTable t, int fastq,
                                                          uint64_t j0, const uint32_t* __restrict__ bits2,
                                                          const uint64_t* __restrict__ mates, uint64_t pos_lo, uint64_t pos_hi,
                                                          uint32_t* __restrict__ out_len, uint32_t* __restrict__ keep,
                                                          uint64_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.n) return;
    const uint64_t j = j0 + i;
    uint64_t bytes = 0;
    if (bit_of(bits2, j)) {
        const uint64_t pos = mates[j];
        if (pos_lo <= pos && pos < pos_hi) bytes = record_text_len(buf, buf_n, t, fastq, i) + 1u;
    }
    if (bytes > 0xFFFFFFFFull) {
        atomicOr((unsigned long long*)&status[0], (unsigned long long)ERR_RECORD_TOO_LARGE);
        bytes = 0;
    }
    out_len[i] = (uint32_t)bytes;
    keep[i] = bytes ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_pairb_order_append(uint64_t n, uint64_t j0, const uint64_t* __restrict__ mates,
                                                            const uint32_t* __restrict__ out_len, const uint64_t* __restrict__ out_off,
                                                            const uint64_t* __restrict__ keep_off, uint64_t n0, uint64_t bytes0,
                                                            uint64_t* __restrict__ acc_pos, uint64_t* __restrict__ acc_off,
                                                            uint32_t* __restrict__ acc_len) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t len = out_len[i];
    if (len == 0) return;
    const uint64_t k = n0 + keep_off[i];
    acc_pos[k] = mates[j0 + i];
    acc_off[k] = bytes0 + out_off[i];
    acc_len[k] = len;
}

__global__ __launch_bounds__(256) void k_pairb_order_slots(const uint64_t* __restrict__ pos, const uint32_t* __restrict__ len, uint64_t n,
                                                           uint64_t pos_lo, uint32_t* __restrict__ slots) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = pos[i] - pos_lo;
    if (k < n) slots[k] = len[i];
}

__global__ __launch_bounds__(256) void k_pairb_order_offsets(const uint64_t* __restrict__ pos, const uint32_t* __restrict__ len,
                                                             uint64_t n, uint64_t pos_lo, const uint32_t* __restrict__ slots,
                                                             const uint64_t* __restrict__ slot_off, uint64_t* __restrict__ off,
                                                             unsigned long long* __restrict__ n_bad) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = pos[i] - pos_lo;
    if (k < n && slots[k] == len[i]) {
        off[i] = slot_off[k];
    } else {
        off[i] = 0;
        atomicAdd(n_bad, 1ull);  // (never, unless the bucket did not receive the shards of file 2 it was planned for)
    }
}

__global__ __launch_bounds__(256) void k_pairb_apply(const uint32_t* __restrict__ bits, uint64_t j0, const uint32_t* __restrict__ fmt_len,
                                                     uint64_t n, uint32_t* __restrict__ len_set, uint32_t* __restrict__ len_clear,
                                                     unsigned long long* __restrict__ tot) {
    __shared__ unsigned long long s_bytes[2];
    __shared__ uint32_t s_recs[2];
    if (threadIdx.x < 2) { s_bytes[threadIdx.x] = 0; s_recs[threadIdx.x] = 0; }
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const bool set = bit_of(bits, j0 + i);
        const uint32_t len = fmt_len[i];
        len_set[i] = set ? len : 0u;
        len_clear[i] = set ? 0u : len;
        atomicAdd(&s_bytes[set ? 0 : 1], (unsigned long long)len);
        atomicAdd(&s_recs[set ? 0 : 1], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_recs[threadIdx.x]) {
        atomicAdd(&tot[threadIdx.x], s_bytes[threadIdx.x]);
        atomicAdd(&tot[2 + threadIdx.x], (unsigned long long)s_recs[threadIdx.x]);
    }
}

inline dim3 grid_of(uint64_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

hipError_t launch_pairb_verify(const uint8_t* acc, const uint64_t* a_off, const uint32_t* a_len, const uint32_t* first, uint64_t n,
                               uint64_t* members, uint64_t* n_members, uint32_t* flagged, uint32_t cap, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pairb_verify, grid_of(n * CMP_LANES), dim3(256), 0, st, acc, a_off, a_len, first, n, members,
                       (unsigned long long*)n_members, flagged, cap);
    return hipGetLastError();
}

hipError_t launch_pairb_scatter(const uint8_t* state, const uint32_t* partner, const uint64_t* a_gidx, uint64_t n, uint64_t n1,
                                uint32_t* bits1, uint32_t* bits2, uint64_t* mates, uint64_t* n_pairs, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pairb_scatter, grid_of(n), dim3(256), 0, st, state, partner, a_gidx, n, n1, bits1, bits2, mates,
                       (unsigned long long*)n_pairs);
    return hipGetLastError();
}

hipError_t launch_pairb_set(const uint64_t* a, const uint64_t* b, uint64_t m, uint64_t n1, uint32_t* bits1, uint32_t* bits2,
                            uint64_t* mates, hipStream_t st) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pairb_set, grid_of(m), dim3(256), 0, st, a, b, m, n1, bits1, bits2, mates);
    return hipGetLastError();
}

hipError_t launch_pairb_count(const uint32_t* bits, uint64_t words, uint16_t* wpre, uint32_t* cnt, hipStream_t st) {
    if (words == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pairb_count, dim3((unsigned)((words + PAIRB_RANK_WORDS - 1) / PAIRB_RANK_WORDS)), dim3(PAIRB_RANK_WORDS), 0, st, bits,
                       words, wpre, cnt);
    return hipGetLastError();
}

hipError_t launch_pairb_rank(const uint32_t* bits1, const uint16_t* wpre1, const uint64_t* base1, const uint32_t* bits2,
                             const uint16_t* wpre2, const uint64_t* base2, uint64_t n2, uint64_t* mates, uint64_t* n_disorder,
                             hipStream_t st) {
    if (n2 == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pairb_rank, grid_of(n2), dim3(256), 0, st, bits1, wpre1, base1, bits2, wpre2, base2, n2, mates,
                       (unsigned long long*)n_disorder);
    return hipGetLastError();
}

hipError_t launch_pairb_pos(uint64_t first, uint64_t count, uint64_t n1, const uint32_t* bits1, const uint16_t* wpre1,
                            const uint64_t* base1, const uint32_t* bits2, const uint64_t* mates, uint64_t* pos, hipStream_t st) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pairb_pos, grid_of(count), dim3(256), 0, st, first, count, n1, bits1, wpre1, base1, bits2, mates, pos);
    return hipGetLastError();
}

hipError_t launch_pairb_order_hist(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, int fastq, uint64_t j0, const uint32_t* bits2,
                                   const uint64_t* mates, uint32_t shift, uint64_t* bytes, uint64_t* records, int num_cus, hipStream_t st) {
    if (t.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pairb_order_hist, dim3(bucket_hist_blocks(t.n, num_cus)), dim3(256), 0, st, buf, buf_n, t, fastq, j0, bits2, mates, shift,
                       (unsigned long long*)bytes, (unsigned long long*)records);
    return hipGetLastError();
}

hipError_t launch_pairb_order_pick(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, int fastq, uint64_t j0, const uint32_t* bits2,
                                   const uint64_t* mates, uint64_t pos_lo, uint64_t pos_hi, uint32_t* out_len, uint32_t* keep,
                                   uint64_t* status, hipStream_t st) {
    if (t.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pairb_order_pick, grid_of(t.n), dim3(256), 0, st, buf, buf_n, t, fastq, j0, bits2, mates, pos_lo, pos_hi, out_len, keep,
                       status);
    return hipGetLastError();
}

hipError_t launch_pairb_order_append(uint64_t n, uint64_t j0, const uint64_t* mates, const uint32_t* out_len, const uint64_t* out_off,
                                     const uint64_t* keep_off, uint64_t n0, uint64_t bytes0, uint64_t* acc_pos, uint64_t* acc_off,
                                     uint32_t* acc_len, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pairb_order_append, grid_of(n), dim3(256), 0, st, n, j0, mates, out_len, out_off, keep_off, n0, bytes0, acc_pos,
                       acc_off, acc_len);
    return hipGetLastError();
}

hipError_t launch_pairb_order_slots(const uint64_t* pos, const uint32_t* len, uint64_t n, uint64_t pos_lo, uint32_t* slots, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pairb_order_slots, grid_of(n), dim3(256), 0, st, pos, len, n, pos_lo, slots);
    return hipGetLastError();
}

hipError_t launch_pairb_order_offsets(const uint64_t* pos, const uint32_t* len, uint64_t n, uint64_t pos_lo, const uint32_t* slots,
                                      const uint64_t* slot_off, uint64_t* off, uint64_t* n_bad, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pairb_order_offsets, grid_of(n), dim3(256), 0, st, pos, len, n, pos_lo, slots, slot_off, off,
                       (unsigned long long*)n_bad);
    return hipGetLastError();
}

hipError_t launch_pairb_apply(const uint32_t* bits, uint64_t j0, const uint32_t* fmt_len, uint64_t n, uint32_t* len_set,
                              uint32_t* len_clear, uint64_t* tot, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pairb_apply, grid_of(n), dim3(256), 0, st, bits, j0, fmt_len, n, len_set, len_clear, (unsigned long long*)tot);
    return hipGetLastError();
}

}  // namespace bsk
