// The fine-bin histogram of the bucket passes (shuffle in buckets of the draw, sort and rmdup in buckets of the key), written
// once: k_shuffle_hist, k_sort_hist and k_rdb_hist are this body with their own (bin, bytes) of a record.  bsk_shuffle_plan
// plans all three, so there is one bin count.
#pragma once
#include <algorithm>
#include <cstdint>

namespace bsk {

constexpr uint32_t BUCKET_BINS = 4096;

// the grid of a histogram kernel over n records: three blocks of 48 KiB fit the LDS of a CU
inline unsigned bucket_hist_blocks(uint64_t n, int num_cus) {
    return (unsigned)std::min<uint64_t>((n + 255) / 256, (uint64_t)std::max(1, num_cus) * 3);
}

#ifdef __HIPCC__
struct BinBytes { uint32_t bin; unsigned long long bytes; };

// bytes and records per fine bin, privatised per block: 4096 x (u64 + u32) = 48 KiB of LDS, merged with one global atomic per
// counter and non-empty bin.  A block walks many records (grid-stride) so that the zeroing and the merge of its 48 KiB are
// paid once.  of(i) = BinBytes of record i; bin = BUCKET_BINS: the record is not counted.
template <class F>
__device__ __forceinline__ void bucket_hist(uint64_t n, unsigned long long* __restrict__ g_bytes, unsigned long long* __restrict__ g_records,
                                            F of) {
    __shared__ unsigned long long s_bytes[BUCKET_BINS];
    __shared__ uint32_t s_records[BUCKET_BINS];
    for (uint32_t b = threadIdx.x; b < BUCKET_BINS; b += blockDim.x) { s_bytes[b] = 0; s_records[b] = 0; }
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const BinBytes r = of(i);
        if (r.bin >= BUCKET_BINS) continue;  // (a record that counts nowhere: the unpaired ones of pair's order histogram)
        atomicAdd(&s_bytes[r.bin], r.bytes);
        atomicAdd(&s_records[r.bin], 1u);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < BUCKET_BINS; b += blockDim.x) {
        const uint32_t r = s_records[b];
        if (r == 0) continue;
        atomicAdd(&g_bytes[b], s_bytes[b]);
        atomicAdd(&g_records[b], (unsigned long long)r);
    }
}
#endif

}  // namespace bsk
