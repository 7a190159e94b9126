// `common` in buckets of the key: what a bucket decides (see ops_common_buckets.hpp).  The comparison has the shape of
// k_renb_verify (ops_rename_buckets.hip): 32 records per block, 8 lanes each, the lanes of a record meet in one LDS word.
#include <hip/hip_runtime.h>

#include "ops_common_buckets.hpp"

namespace bsk {
namespace {

constexpr uint32_t CMP_LANES = 8;         // lanes per record of the comparison
constexpr uint32_t CMP_STEP = 16u * CMP_LANES;

// the file of global record index g: the number of running sums that are <= g (n_files <= COMMON_MAX_FILES; an empty file
// repeats the sum in front of it and is skipped by it)
__device__ __forceinline__ uint32_t file_of(const uint64_t* s_sums, uint32_t n_files, uint64_t g) {
    uint32_t f = 0;
    for (uint32_t k = 0; k < n_files; ++k) f += s_sums[k] <= g ? 1u : 0u;
    return f;
}

// one 64-bit atomicOr per record on the mask of its head: the records of a key that fills many blocks meet on one address
__global__ __launch_bounds__(256) void k_comb_verify(const uint8_t* __restrict__ acc, const uint64_t* __restrict__ a_off,
                                                     const uint32_t* __restrict__ a_len, const uint64_t* __restrict__ a_gidx,
                                                     const uint32_t* __restrict__ first, uint64_t n,
                                                     const uint64_t* __restrict__ file_sums, uint32_t n_files,
                                                     unsigned long long* __restrict__ masks, uint32_t* __restrict__ flagged,
                                                     uint32_t cap) {
    constexpr uint32_t PER_BLOCK = 256 / CMP_LANES;
    __shared__ uint64_t s_sums[COMMON_MAX_FILES];
    __shared__ uint32_t s_diff[PER_BLOCK];
    const uint32_t grp = threadIdx.x / CMP_LANES, gl = threadIdx.x & (CMP_LANES - 1u);
    if (threadIdx.x < PER_BLOCK) s_diff[threadIdx.x] = 0;
    if (threadIdx.x < COMMON_MAX_FILES) s_sums[threadIdx.x] = threadIdx.x < n_files ? file_sums[threadIdx.x] : ~0ull;
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
        } else {
            // a head (f == i) or a member of its group: the file of this record joins the mask of the head
            const uint32_t file = file_of(s_sums, n_files, a_gidx[i]);
            if (file < n_files) atomicOr(&masks[f], 1ull << file);
        }
    }
}

__global__ __launch_bounds__(256) void k_comb_decide(const uint32_t* __restrict__ first, const uint64_t* __restrict__ a_gidx,
                                                     const unsigned long long* __restrict__ masks, uint64_t n,
                                                     unsigned long long full, uint64_t first_file_records,
                                                     uint32_t* __restrict__ bits, unsigned long long* __restrict__ n_kept) {
    __shared__ uint32_t s_kept;
    if (threadIdx.x == 0) s_kept = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && first[i] == (uint32_t)i && masks[i] == full) {
        const uint64_t g = a_gidx[i];
        if (g < first_file_records) {  // (a full mask holds file 1, whose records have the lowest indices: the head lies in it)
            atomicOr(&bits[g >> 5], 1u << (uint32_t)(g & 31u));  // (two heads can share a word)
            atomicAdd(&s_kept, 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_kept) atomicAdd(n_kept, (unsigned long long)s_kept);
}

__global__ __launch_bounds__(256) void k_comb_set(const uint64_t* __restrict__ g, uint64_t m, uint32_t* __restrict__ bits) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const uint64_t v = g[j];
    atomicOr(&bits[v >> 5], 1u << (uint32_t)(v & 31u));
}

__global__ __launch_bounds__(256) void k_comb_apply(const uint32_t* __restrict__ bits, uint64_t first_record, uint64_t n,
                                                    uint32_t* __restrict__ out_len) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t g = first_record + i;
    if (!((bits[g >> 5] >> (uint32_t)(g & 31u)) & 1u)) out_len[i] = 0u;
}

inline dim3 grid_of(uint64_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

hipError_t launch_comb_verify(const uint8_t* acc, const uint64_t* a_off, const uint32_t* a_len, const uint64_t* a_gidx,
                              const uint32_t* first, uint64_t n, const uint64_t* file_sums, uint32_t n_files, uint64_t* masks,
                              uint32_t* flagged, uint32_t cap, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (n_files == 0 || n_files > COMMON_MAX_FILES) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_comb_verify, grid_of(n * CMP_LANES), dim3(256), 0, st, acc, a_off, a_len, a_gidx, first, n, file_sums, n_files,
                       (unsigned long long*)masks, flagged, cap);
    return hipGetLastError();
}

hipError_t launch_comb_decide(const uint32_t* first, const uint64_t* a_gidx, const uint64_t* masks, uint64_t n, uint64_t full,
                              uint64_t first_file_records, uint32_t* bits, uint64_t* n_kept, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_comb_decide, grid_of(n), dim3(256), 0, st, first, a_gidx, (const unsigned long long*)masks, n,
                       (unsigned long long)full, first_file_records, bits, (unsigned long long*)n_kept);
    return hipGetLastError();
}

hipError_t launch_comb_set(const uint64_t* g, uint64_t m, uint32_t* bits, hipStream_t st) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_comb_set, grid_of(m), dim3(256), 0, st, g, m, bits);
    return hipGetLastError();
}

hipError_t launch_comb_apply(const uint32_t* bits, uint64_t first_record, uint64_t n, uint32_t* out_len, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_comb_apply, grid_of(n), dim3(256), 0, st, bits, first_record, n, out_len);
    return hipGetLastError();
}

}  // namespace bsk
