// `rename` in buckets of the key: what a bucket decides (see ops_rename_buckets.hpp).  The comparison has the shape of
// k_rdb_verify (ops_rmdup_buckets.hip): 32 records per block, 8 lanes each, the lanes of a record meet in one LDS word.
#include <hip/hip_runtime.h>

#include "ops_rename_buckets.hpp"

namespace bsk {
namespace {

constexpr uint32_t CMP_LANES = 8;         // lanes per record of the comparison
constexpr uint32_t CMP_STEP = 16u * CMP_LANES;

// the members of a block take their places in the list with ONE atomic of the block: the order of the list is free, the sort
// behind it orders by (first, index)
__global__ __launch_bounds__(256) void k_renb_verify(const uint8_t* __restrict__ acc, const uint64_t* __restrict__ a_off,
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
    if (later && gl == 0u) {
        if (s_diff[grp]) {
            const uint32_t pos = atomicAdd(&flagged[0], 1u);  // (the count stays exact beyond the cap)
            if (pos < cap) flagged[1 + pos] = (uint32_t)i;
        } else {
            member = true;
            slot = atomicAdd(&s_count, 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_count) s_base = atomicAdd(n_members, (unsigned long long)s_count);
    __syncthreads();
    if (member) members[s_base + slot] = ((uint64_t)f << 32) | (uint64_t)(uint32_t)i;
}

__global__ __launch_bounds__(256) void k_renb_scatter(const uint32_t* __restrict__ ord_bucket, const uint64_t* __restrict__ a_gidx,
                                                      uint64_t n, uint32_t* __restrict__ ord_global) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = ord_bucket[i];
    if (k) ord_global[a_gidx[i]] = k;
}

__global__ __launch_bounds__(256) void k_renb_set(const uint64_t* __restrict__ g, const uint32_t* __restrict__ v, uint64_t m,
                                                  uint32_t* __restrict__ ord_global) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < m) ord_global[g[j]] = v[j];
}

inline dim3 grid_of(uint64_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

hipError_t launch_renb_verify(const uint8_t* acc, const uint64_t* a_off, const uint32_t* a_len, const uint32_t* first, uint64_t n,
                              uint64_t* members, uint64_t* n_members, uint32_t* flagged, uint32_t cap, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_renb_verify, grid_of(n * CMP_LANES), dim3(256), 0, st, acc, a_off, a_len, first, n, members,
                       (unsigned long long*)n_members, flagged, cap);
    return hipGetLastError();
}

hipError_t launch_renb_scatter(const uint32_t* ord_bucket, const uint64_t* a_gidx, uint64_t n, uint32_t* ord_global, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_renb_scatter, grid_of(n), dim3(256), 0, st, ord_bucket, a_gidx, n, ord_global);
    return hipGetLastError();
}

hipError_t launch_renb_set(const uint64_t* g, const uint32_t* v, uint64_t m, uint32_t* ord_global, hipStream_t st) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_renb_set, grid_of(m), dim3(256), 0, st, g, v, m, ord_global);
    return hipGetLastError();
}

}  // namespace bsk
