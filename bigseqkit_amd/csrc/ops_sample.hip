// sample / shuffle: the table passes (see ops_sample.hpp).  One lane per record, 8-24 bytes of table per record; the text
// itself is moved by the segmented copy.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ops_records.hpp"  // ERR_RECORD_TOO_LARGE
#include "ops_sample.hpp"
#include "record_text_dev.hpp"
#include "sample_dev.hpp"

namespace bsk {
namespace {

// the verdict of a closed interval of the draw: out_len[i] = text + '\n' of record i when lo <= draw <= hi, else 0, and -- with a
// keep array -- keep[i] = 1 / 0.  `sample` passes the interval of its threshold (sample_interval), a bucket of `shuffle` its own.
__global__ __launch_bounds__(256) void k_sample_size(const uint8_t* __restrict__ buf, uint64_t buf_n, RecordTable t, int fastq,
                                                     uint64_t first_record, uint64_t key, uint64_t lo, uint64_t hi,
                                                     uint32_t* __restrict__ out_len, uint32_t* __restrict__ keep,
                                                     uint64_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.n) return;
    const uint64_t d = sample_draw(key, first_record + i);
    uint64_t bytes = 0;
    if (lo <= d && d <= hi) bytes = record_text_len(buf, buf_n, t, fastq, i) + 1u;
    if (bytes > 0xFFFFFFFFull) {
        atomicOr((unsigned long long*)&status[0], (unsigned long long)ERR_RECORD_TOO_LARGE);
        bytes = 0;
    }
    out_len[i] = (uint32_t)bytes;
    if (keep) keep[i] = bytes ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_shuffle_keys(uint64_t n, uint64_t key, uint64_t* __restrict__ keys) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = sample_draw(key, i);
}

// segment j = record perm[j] of the n records (off[], len[]) that lie in base[0, extent).  With a counter n_other the byte
// behind the text is looked at: a record that is not followed by its '\n' gets source 0 and is counted (k_shuffle_fix writes
// it); without one (the texts of an accumulation all end in their newline) no text byte is read.
__global__ __launch_bounds__(256) void k_shuffle_segments(uint64_t n, const uint8_t* __restrict__ base, uint64_t extent,
                                                          const uint64_t* __restrict__ off, const uint32_t* __restrict__ len,
                                                          const uint32_t* __restrict__ perm, uint64_t* __restrict__ seg_src,
                                                          uint32_t* __restrict__ len_perm, unsigned long long* __restrict__ n_other) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = perm[j];
    const uint32_t m = len[i];
    uint64_t s = 0;
    if (m) {
        const uint64_t at = off[i];
        if (!n_other || (at + m <= extent && base[at + m - 1] == '\n')) s = (uint64_t)(uintptr_t)(base + at);
        else atomicAdd(n_other, 1ull);  // the last record of a shard without a final newline
    }
    seg_src[j] = s;
    len_perm[j] = m;
}

// segment j byte by byte: len_perm[j] - 1 bytes from base + off[perm[j]], then '\n'.  all = 0: only the segments the copy
// left out (source 0)
__global__ __launch_bounds__(256) void k_shuffle_fix(uint64_t n, const uint8_t* __restrict__ base, const uint64_t* __restrict__ off,
                                                     const uint32_t* __restrict__ perm, const uint32_t* __restrict__ len_perm,
                                                     const uint64_t* __restrict__ seg_off, const uint64_t* __restrict__ seg_src,
                                                     uint8_t* __restrict__ out, int all) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t m = len_perm[j];
    if (m == 0 || (!all && seg_src[j] != 0)) return;
    const uint8_t* s = base + off[perm[j]];
    uint8_t* o = out + seg_off[j];
    for (uint32_t k = 0; k + 1 < m; ++k) o[k] = s[k];
    o[m - 1] = (uint8_t)'\n';
}

// ---- shuffle in buckets of the draw (PARITY.md SHUF): the 64-bit draw range is cut into BUCKET_BINS fine bins, a bucket is a run
// of consecutive bins, the output is bucket 0 sorted by draw, then bucket 1, ...

// bytes (text + '\n') and records per fine bin (bucket_hist_dev.hpp); the bin is the upper 12 bits of the draw
__global__ __launch_bounds__(256) void k_shuffle_hist(const uint8_t* __restrict__ buf, uint64_t buf_n, RecordTable t, int fastq,
                                                      uint64_t first_record, uint64_t key, unsigned long long* __restrict__ g_bytes,
                                                      unsigned long long* __restrict__ g_records) {
    bucket_hist(t.n, g_bytes, g_records, [&](uint64_t i) {
        return BinBytes{(uint32_t)(sample_draw(key, first_record + i) >> SHUFFLE_BIN_SHIFT), record_text_len(buf, buf_n, t, fastq, i) + 1u};
    });
}

// the kept records of the shard join the accumulation, in shard order: (draw, byte offset, length) at n0 + keep_off[i]
__global__ __launch_bounds__(256) void k_shuffle_append(uint64_t n, uint64_t first_record, uint64_t key, const uint32_t* __restrict__ out_len,
                                                        const uint64_t* __restrict__ out_off, const uint64_t* __restrict__ keep_off,
                                                        uint64_t n0, uint64_t bytes0, uint64_t* __restrict__ acc_draw,
                                                        uint64_t* __restrict__ acc_off, uint32_t* __restrict__ acc_len) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t len = out_len[i];
    if (len == 0) return;
    const uint64_t j = n0 + keep_off[i];
    acc_draw[j] = sample_draw(key, first_record + i);
    acc_off[j] = bytes0 + out_off[i];
    acc_len[j] = len;
}

inline dim3 grid_of(uint64_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

void sample_draw_interval(uint64_t threshold, uint64_t* lo, uint64_t* hi) {
    const DrawInterval I = sample_interval(threshold);
    *lo = I.lo;
    *hi = I.hi;
}

hipError_t launch_sample_size(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, const SampleParams& P, uint32_t* out_len,
                              uint32_t* keep, uint64_t* status, hipStream_t st) {
    if (t.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sample_size, grid_of(t.n), dim3(256), 0, st, buf, buf_n, t, P.fastq, P.first_record, sample_key(P.seed), P.lo,
                       P.hi, out_len, keep, status);
    return hipGetLastError();
}

hipError_t launch_shuffle_keys(uint64_t n, int64_t seed, uint64_t* keys, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_shuffle_keys, grid_of(n), dim3(256), 0, st, n, sample_key(seed), keys);
    return hipGetLastError();
}

hipError_t launch_shuffle_segments(uint64_t n, const uint8_t* base, uint64_t extent, const uint64_t* off, const uint32_t* len,
                                   const uint32_t* perm, uint64_t* seg_src, uint32_t* len_perm, uint64_t* n_other, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_shuffle_segments, grid_of(n), dim3(256), 0, st, n, base, extent, off, len, perm, seg_src, len_perm,
                       (unsigned long long*)n_other);
    return hipGetLastError();
}

hipError_t launch_shuffle_fix(uint64_t n, const uint8_t* base, const uint64_t* off, const uint32_t* perm, const uint32_t* len_perm,
                              const uint64_t* seg_off, const uint64_t* seg_src, uint8_t* out, bool all, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_shuffle_fix, grid_of(n), dim3(256), 0, st, n, base, off, perm, len_perm, seg_off, seg_src, out, all ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_shuffle_hist(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, int fastq, uint64_t first_record, int64_t seed,
                               uint64_t* bytes, uint64_t* records, int num_cus, hipStream_t st) {
    if (t.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_shuffle_hist, dim3(bucket_hist_blocks(t.n, num_cus)), dim3(256), 0, st, buf, buf_n, t, fastq, first_record, sample_key(seed),
                       (unsigned long long*)bytes, (unsigned long long*)records);
    return hipGetLastError();
}

hipError_t launch_shuffle_append(uint64_t n, uint64_t first_record, int64_t seed, const uint32_t* out_len, const uint64_t* out_off,
                                 const uint64_t* keep_off, uint64_t n0, uint64_t bytes0, uint64_t* acc_draw, uint64_t* acc_off,
                                 uint32_t* acc_len, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_shuffle_append, grid_of(n), dim3(256), 0, st, n, first_record, sample_key(seed), out_len, out_off, keep_off, n0,
                       bytes0, acc_draw, acc_off, acc_len);
    return hipGetLastError();
}

}  // namespace bsk
