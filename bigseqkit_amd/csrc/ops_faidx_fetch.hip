// `faidx -d`: the fetch kernel -- one block of 256 lanes per tile of fai::FETCH_T output bases, the tile itself is
// fai::fetch_tile (fai_fetch_dev.hpp, shared with the host).  DESIGN.md f21.
#include <hip/hip_runtime.h>

#include "ops_faidx_fetch.hpp"

namespace bsk {
namespace {

struct DevicePolicy {
    static constexpr uint32_t LANES = 256;
    const uint8_t* buf;
    uint8_t* out;
    unsigned long long* status;
    __device__ __forceinline__ uint32_t lane() const { return threadIdx.x; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ fai::Vec16 load16(uint64_t i) const {
        const uint4 v = *reinterpret_cast<const uint4*>(buf + i);
        return fai::Vec16{{v.x, v.y, v.z, v.w}};
    }
    __device__ __forceinline__ uint8_t byte(uint64_t i) const { return buf[i]; }
    __device__ __forceinline__ void store16(uint64_t o, const fai::Vec16& v) const {
        *reinterpret_cast<uint4*>(out + o) = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
    }
    __device__ __forceinline__ void store8(uint64_t o, uint8_t b) const { out[o] = b; }
    __device__ __forceinline__ void fail(uint64_t word) const { atomicMin(status, (unsigned long long)word); }
};

__global__ __launch_bounds__(256) void k_faidx_fetch(const uint8_t* __restrict__ buf, const fai::FetchHit* __restrict__ hits,
                                                      const fai::FetchTile* __restrict__ tiles, uint32_t ntiles, uint32_t line_width,
                                                      const uint8_t* __restrict__ comp, const uint8_t* __restrict__ headers,
                                                      uint8_t* __restrict__ out, unsigned long long* status) {
    __shared__ fai::FetchShared S;
    DevicePolicy p{buf, out, status};
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const fai::FetchTile tl = tiles[t];
        fai::fetch_tile(p, S, hits[tl.hit], t, tl.q0, line_width, comp, headers);
    }
}

}  // namespace

hipError_t launch_faidx_fetch(const uint8_t* buf, const fai::FetchHit* hits, const fai::FetchTile* tiles, uint32_t ntiles,
                              uint32_t line_width, const uint8_t* comp, const uint8_t* headers, uint8_t* out, uint64_t* status,
                              int num_cus, hipStream_t st) {
    if (ntiles == 0) return hipSuccess;
    const uint32_t cap = (uint32_t)(num_cus > 0 ? num_cus : 256) * 8u;
    const uint32_t grid = ntiles < cap ? ntiles : cap;
    hipLaunchKernelGGL(k_faidx_fetch, dim3(grid), dim3(256), 0, st, buf, hits, tiles, ntiles, line_width, comp, headers, out,
                       reinterpret_cast<unsigned long long*>(status));
    return hipGetLastError();
}

}  // namespace bsk
