// `concat` in buckets of the key: what a match bucket decides and the table passes of the join phase (see
// ops_concat_buckets.hpp).  The comparison has the shape of k_renb_verify (ops_rename_buckets.hip): 32 records per block, 8 lanes
// each, the lanes of a record meet in one LDS word.  Everything else is one lane per record.
#include <hip/hip_runtime.h>

#include "bucket_hist_dev.hpp"
#include "ops_concat_buckets.hpp"
#include "ops_records.hpp"  // ERR_RECORD_TOO_LARGE
#include "record_text_dev.hpp"

namespace bsk {
namespace {

constexpr uint32_t CMP_LANES = 8;         // lanes per record of the comparison
constexpr uint32_t CMP_STEP = 16u * CMP_LANES;

__device__ __forceinline__ bool bit_of(const uint32_t* __restrict__ bits, uint64_t g) {
    return (bits[g >> 5] >> (uint32_t)(g & 31u)) & 1u;
}

__global__ __launch_bounds__(256) void k_catb_verify(const uint8_t* __restrict__ acc, const uint64_t* __restrict__ a_off,
                                                     const uint32_t* __restrict__ a_len, const uint64_t* __restrict__ a_gidx,
                                                     const uint32_t* __restrict__ first, uint64_t n, uint64_t n1,
                                                     uint64_t* __restrict__ head, uint32_t* __restrict__ flagged, uint32_t cap,
                                                     unsigned long long* __restrict__ n_matched) {
    constexpr uint32_t PER_BLOCK = 256 / CMP_LANES;
    __shared__ uint32_t s_diff[PER_BLOCK];
    __shared__ uint32_t s_count;
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
    if (i < n && gl == 0u) {
        if (later && s_diff[grp]) {
            const uint32_t pos = atomicAdd(&flagged[0], 1u);  // (the count stays exact beyond the cap)
            if (pos < cap) flagged[1 + pos] = (uint32_t)i;
        } else {  // the first of the group, or a record with its bytes: file 1 comes first, so the first is the lowest g
            const uint64_t gf = a_gidx[f];
            const bool in1 = gf < n1;
            head[a_gidx[i]] = in1 ? gf : CATB_NONE;
            if (in1) atomicAdd(&s_count, 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_count) atomicAdd(n_matched, (unsigned long long)s_count);
}

__global__ __launch_bounds__(256) void k_catb_set(const uint64_t* __restrict__ g, const uint64_t* __restrict__ h, uint64_t m,
                                                  uint64_t* __restrict__ head) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < m) head[g[j]] = h[j];
}

// (the records of a heavy ID serialise on one address)
__global__ __launch_bounds__(256) void k_catb_weigh(const uint8_t* __restrict__ buf, uint64_t buf_n, RecordTable t, int fastq, uint64_t g0,
                                                    const uint64_t* __restrict__ head, unsigned long long* __restrict__ W,
                                                    unsigned long long* __restrict__ C) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.n) return;
    const uint64_t h = head[g0 + i];
    if (h == CATB_NONE) return;
    atomicAdd(&W[h], (unsigned long long)(record_text_len(buf, buf_n, t, fastq, i) + 1u));
    atomicAdd(&C[h], 1ull);
}

__global__ __launch_bounds__(256) void k_catb_hist(const uint8_t* __restrict__ buf, uint64_t buf_n, RecordTable t, int fastq, uint64_t a0,
                                                   const uint64_t* __restrict__ head, const uint64_t* __restrict__ W,
                                                   const uint64_t* __restrict__ C, uint32_t shift,
                                                   unsigned long long* __restrict__ g_bytes, unsigned long long* __restrict__ g_records) {
    bucket_hist(t.n, g_bytes, g_records, [&](uint64_t i) {
        const uint64_t a = a0 + i, bin = a >> shift, h = head[a];
        const unsigned long long ta = record_text_len(buf, buf_n, t, fastq, i) + 1u;
        const unsigned long long cost = h == CATB_NONE ? ta : ta * (1ull + C[h]) + 2ull * W[h];
        return BinBytes{(uint32_t)(bin < BUCKET_BINS ? bin : BUCKET_BINS), cost};
    });
}

__global__ __launch_bounds__(256) void k_catb_mark(const uint8_t* __restrict__ buf, uint64_t buf_n, RecordTable t, int fastq, uint64_t a0,
                                                   const uint64_t* __restrict__ head, uint32_t shift, uint32_t lo_bin, uint32_t hi_bin,
                                                   uint32_t* __restrict__ mark, uint32_t* __restrict__ out_len,
                                                   uint32_t* __restrict__ keep, uint64_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.n) return;
    const uint64_t a = a0 + i, bin = a >> shift;
    uint64_t bytes = 0;
    if (lo_bin <= bin && bin < hi_bin) {
        bytes = record_text_len(buf, buf_n, t, fastq, i) + 1u;
        if (bytes > 0xFFFFFFFFull) {
            atomicOr((unsigned long long*)&status[0], (unsigned long long)ERR_RECORD_TOO_LARGE);
            bytes = 0;
        } else {
            const uint64_t h = head[a];
            if (h != CATB_NONE) atomicOr(&mark[h >> 5], 1u << (uint32_t)(h & 31u));  // (two records can share a word)
        }
    }
    out_len[i] = (uint32_t)bytes;
    keep[i] = bytes ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_catb_pick(const uint8_t* __restrict__ buf, uint64_t buf_n, RecordTable t, int fastq, uint64_t g0,
                                                   const uint64_t* __restrict__ head, const uint32_t* __restrict__ mark,
                                                   uint32_t* __restrict__ out_len, uint32_t* __restrict__ keep,
                                                   uint64_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.n) return;
    const uint64_t h = head[g0 + i];
    uint64_t bytes = 0;
    if (h != CATB_NONE && bit_of(mark, h)) bytes = record_text_len(buf, buf_n, t, fastq, i) + 1u;
    if (bytes > 0xFFFFFFFFull) {
        atomicOr((unsigned long long*)&status[0], (unsigned long long)ERR_RECORD_TOO_LARGE);
        bytes = 0;
    }
    out_len[i] = (uint32_t)bytes;
    keep[i] = bytes ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_catb_tail(const uint64_t* __restrict__ head, uint64_t g0, uint64_t n,
                                                   uint32_t* __restrict__ out_len) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && head[g0 + i] != CATB_NONE) out_len[i] = 0;
}

inline dim3 grid_of(uint64_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

hipError_t launch_catb_verify(const uint8_t* acc, const uint64_t* a_off, const uint32_t* a_len, const uint64_t* a_gidx, const uint32_t* first,
                              uint64_t n, uint64_t n1, uint64_t* head, uint32_t* flagged, uint32_t cap, uint64_t* n_matched, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_catb_verify, grid_of(n * CMP_LANES), dim3(256), 0, st, acc, a_off, a_len, a_gidx, first, n, n1, head, flagged, cap,
                       (unsigned long long*)n_matched);
    return hipGetLastError();
}

hipError_t launch_catb_set(const uint64_t* g, const uint64_t* h, uint64_t m, uint64_t* head, hipStream_t st) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_catb_set, grid_of(m), dim3(256), 0, st, g, h, m, head);
    return hipGetLastError();
}

hipError_t launch_catb_weigh(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, int fastq, uint64_t g0, const uint64_t* head,
                             uint64_t* W, uint64_t* C, hipStream_t st) {
    if (t.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_catb_weigh, grid_of(t.n), dim3(256), 0, st, buf, buf_n, t, fastq, g0, head, (unsigned long long*)W,
                       (unsigned long long*)C);
    return hipGetLastError();
}

hipError_t launch_catb_hist(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, int fastq, uint64_t a0, const uint64_t* head,
                            const uint64_t* W, const uint64_t* C, uint32_t shift, uint64_t* bytes, uint64_t* records, int num_cus,
                            hipStream_t st) {
    if (t.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_catb_hist, dim3(bucket_hist_blocks(t.n, num_cus)), dim3(256), 0, st, buf, buf_n, t, fastq, a0, head, W, C, shift,
                       (unsigned long long*)bytes, (unsigned long long*)records);
    return hipGetLastError();
}

hipError_t launch_catb_mark(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, int fastq, uint64_t a0, const uint64_t* head,
                            uint32_t shift, uint32_t lo_bin, uint32_t hi_bin, uint32_t* mark, uint32_t* out_len, uint32_t* keep,
                            uint64_t* status, hipStream_t st) {
    if (t.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_catb_mark, grid_of(t.n), dim3(256), 0, st, buf, buf_n, t, fastq, a0, head, shift, lo_bin, hi_bin, mark, out_len,
                       keep, status);
    return hipGetLastError();
}

hipError_t launch_catb_pick(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, int fastq, uint64_t g0, const uint64_t* head,
                            const uint32_t* mark, uint32_t* out_len, uint32_t* keep, uint64_t* status, hipStream_t st) {
    if (t.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_catb_pick, grid_of(t.n), dim3(256), 0, st, buf, buf_n, t, fastq, g0, head, mark, out_len, keep, status);
    return hipGetLastError();
}

hipError_t launch_catb_tail(const uint64_t* head, uint64_t g0, uint64_t n, uint32_t* out_len, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_catb_tail, grid_of(n), dim3(256), 0, st, head, g0, n, out_len);
    return hipGetLastError();
}

}  // namespace bsk
