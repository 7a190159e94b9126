// sample / shuffle: the table passes (see ops_sample.hpp).  One lane per record, 8-24 bytes of table per record; the text
// itself is moved by the segmented copy.
#include <hip/hip_runtime.h>

#include "ops_records.hpp"  // ERR_RECORD_TOO_LARGE
#include "ops_sample.hpp"
#include "record_text_dev.hpp"
#include "sample_dev.hpp"

namespace bsk {
namespace {

__global__ __launch_bounds__(256) void k_sample_size(const uint8_t* __restrict__ buf, uint64_t buf_n, RecordTable t, int fastq,
                                                     uint64_t first_record, uint64_t key, uint64_t threshold,
                                                     uint32_t* __restrict__ out_len, uint64_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.n) return;
    uint64_t bytes = 0;
    if (sample_keeps(key, first_record + i, threshold)) bytes = record_text_len(buf, buf_n, t, fastq, i) + 1u;
    if (bytes > 0xFFFFFFFFull) {
        atomicOr((unsigned long long*)&status[0], (unsigned long long)ERR_RECORD_TOO_LARGE);
        bytes = 0;
    }
    out_len[i] = (uint32_t)bytes;
}

__global__ __launch_bounds__(256) void k_shuffle_keys(uint64_t n, uint64_t key, uint64_t* __restrict__ keys) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = sample_draw(key, i);
}

__global__ __launch_bounds__(256) void k_shuffle_segments(const uint8_t* __restrict__ buf, uint64_t buf_n, RecordTable t,
                                                          const uint32_t* __restrict__ out_len, const uint32_t* __restrict__ perm,
                                                          uint64_t* __restrict__ seg_src, uint32_t* __restrict__ len_perm,
                                                          unsigned long long* __restrict__ n_other) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= t.n) return;
    const uint32_t i = perm[j];
    const uint32_t n = out_len[i];
    uint64_t s = 0;
    if (n) {
        const uint64_t st = t.start[i];
        if (st + n <= buf_n && buf[st + n - 1] == '\n') s = (uint64_t)(uintptr_t)(buf + st);
        else atomicAdd(n_other, 1ull);  // the last record of a shard without a final newline
    }
    seg_src[j] = s;
    len_perm[j] = n;
}

__global__ __launch_bounds__(256) void k_shuffle_fix(const uint8_t* __restrict__ buf, RecordTable t, const uint32_t* __restrict__ perm,
                                                     const uint32_t* __restrict__ len_perm, const uint64_t* __restrict__ seg_off,
                                                     const uint64_t* __restrict__ seg_src, uint8_t* __restrict__ out, int all) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= t.n) return;
    const uint32_t n = len_perm[j];
    if (n == 0 || (!all && seg_src[j] != 0)) return;
    const uint8_t* s = buf + t.start[perm[j]];
    uint8_t* o = out + seg_off[j];
    for (uint32_t k = 0; k + 1 < n; ++k) o[k] = s[k];
    o[n - 1] = (uint8_t)'\n';
}

inline dim3 grid_of(uint64_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

hipError_t launch_sample_size(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, const SampleParams& P, uint32_t* out_len,
                              uint64_t* status, hipStream_t st) {
    if (t.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sample_size, grid_of(t.n), dim3(256), 0, st, buf, buf_n, t, P.fastq, P.first_record, sample_key(P.seed),
                       P.threshold, out_len, status);
    return hipGetLastError();
}

hipError_t launch_shuffle_keys(uint64_t n, int64_t seed, uint64_t* keys, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_shuffle_keys, grid_of(n), dim3(256), 0, st, n, sample_key(seed), keys);
    return hipGetLastError();
}

hipError_t launch_shuffle_segments(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, const uint32_t* out_len,
                                   const uint32_t* perm, uint64_t* seg_src, uint32_t* len_perm, uint64_t* n_other, hipStream_t st) {
    if (t.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_shuffle_segments, grid_of(t.n), dim3(256), 0, st, buf, buf_n, t, out_len, perm, seg_src, len_perm,
                       (unsigned long long*)n_other);
    return hipGetLastError();
}

hipError_t launch_shuffle_fix(const uint8_t* buf, const RecordTable& t, const uint32_t* perm, const uint32_t* len_perm,
                              const uint64_t* seg_off, const uint64_t* seg_src, uint8_t* out, bool all, hipStream_t st) {
    if (t.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_shuffle_fix, grid_of(t.n), dim3(256), 0, st, buf, t, perm, len_perm, seg_off, seg_src, out, all ? 1 : 0);
    return hipGetLastError();
}

}  // namespace bsk
