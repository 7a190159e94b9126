// The lane policy of the gzip walks on the device (gzip_spec_dev.hpp "A lane policy"): the 64 lanes of one wave.  Device code only:
// ops_gzip.hip and ops_gzip_stream.hip include it.
#pragma once
#include <hip/hip_runtime.h>

#include "gzip_spec_dev.hpp"

namespace bsk {
namespace gz {

// the 64 lanes of a wave that walks a chunk
struct GzWaveLane {
    static constexpr uint32_t LANES = 64;
    const uint8_t* __restrict__ comp;  // a multiple of 8
    uint64_t n;
    uint2 held;                        // bytes [4 * held_base + 8 * lane, + 8)
    uint32_t held_base;                // in units of 512 bytes
    // (the lane is taken anew wherever it is asked for: what depends on it alone -- `lane < 16`, `lane < nlit` as 64-bit lane masks
    // in scalar registers -- is otherwise computed once in front of the walk's one big loop and stays live, or spilled, through it)
    __device__ __forceinline__ uint32_t lane() const {
        uint32_t l = threadIdx.x;
        asm volatile("" : "+v"(l));
        return l;
    }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ __forceinline__ uint64_t uni64(uint64_t v) const { return (uint64_t)uni((uint32_t)v) | (uint64_t)uni((uint32_t)(v >> 32)) << 32; }
    __device__ __forceinline__ uint64_t vec64(uint64_t v) const {
        uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
        asm volatile("" : "+v"(lo), "+v"(hi));
        return (uint64_t)lo | (uint64_t)hi << 32;
    }
    __device__ __forceinline__ uint32_t word(uint64_t w) {
        const uint32_t cb = (uint32_t)(w >> 7);
        if (cb != held_base) {
            held_base = cb;
            const uint64_t at = (uint64_t)cb * 512u + threadIdx.x * 8u;
            uint2 v = make_uint2(0u, 0u);
            if (at + 8u <= n) v = *reinterpret_cast<const uint2*>(comp + at);
            else {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const uint32_t x = at + k < n ? (uint32_t)comp[at + k] << (8 * (k & 3)) : 0u;
                    if (k < 4) v.x |= x; else v.y |= x;
                }
            }
            held = v;
        }
        const int j = (int)(w & 127u);
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)held.x, j >> 1), hi = (uint32_t)__builtin_amdgcn_readlane((int)held.y, j >> 1);
        return (j & 1) ? hi : lo;
    }
    __device__ __forceinline__ uint8_t in_byte(uint64_t a) const { return comp[a]; }
    // symbols [a, b) of the chunk: single ones up to the first 16-byte boundary of the buffer and behind the last, 8 a lane between
    // ((out + q) is a multiple of 16 bytes where (shift + q) is one of 8)
    __device__ __forceinline__ void store(const uint16_t* ring, uint16_t* __restrict__ out, uint32_t shift, uint64_t a, uint64_t b) const {
        const uint32_t l = threadIdx.x;
        uint64_t h = a + ((8u - ((shift + (uint32_t)a) & 7u)) & 7u);
        if (h > b) h = b;
        if (a + l < h) out[a + l] = ring[(shift + (uint32_t)(a + l)) & RING_MASK];
        uint64_t t = b - ((shift + (uint32_t)b) & 7u);
        if (t < h || t > b) t = h;
        for (uint64_t q = h + 8u * l; q < t; q += 8u * LANES)
            *reinterpret_cast<uint4*>(out + q) = *reinterpret_cast<const uint4*>(ring + ((shift + (uint32_t)q) & RING_MASK));
        if (t + l < b) out[t + l] = ring[(shift + (uint32_t)(t + l)) & RING_MASK];
    }
};

}  // namespace gz
}  // namespace bsk
