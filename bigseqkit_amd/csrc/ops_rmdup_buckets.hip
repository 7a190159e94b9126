// `rmdup` in buckets of the key: the table passes (see ops_rmdup_buckets.hpp).  The subject of a record comes from the accessor
// that the hash and the comparisons of `rmdup` use (rmdup_subject_dev.hpp); the grouping of a bucket is the radix-bucket pass
// of ops_rmdup.hip on the accumulated keys.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ops_rmdup_buckets.hpp"
#include "rmdup_subject_dev.hpp"

namespace bsk {
namespace {

constexpr uint32_t PACK_LANES = 8;        // lanes per record of the pack and of the comparison
constexpr uint32_t PACK_STEP = 16u * PACK_LANES;

// bytes (subject + RMDUP_BUCKET_RECORD_BYTES) and records per fine bin (bucket_hist_dev.hpp); the bin is the upper 12 bits of k1
__global__ __launch_bounds__(256) void k_rdb_hist(const uint8_t* __restrict__ buf, RecordTable t, TextTable tt, RmDupParams P,
                                                  const uint64_t* __restrict__ keys, unsigned long long* __restrict__ g_bytes,
                                                  unsigned long long* __restrict__ g_records) {
    bucket_hist(t.n, g_bytes, g_records, [&](uint64_t i) {
        return BinBytes{(uint32_t)(keys[i] >> RMDUP_BIN_SHIFT), (unsigned long long)subject_of(buf, t, tt, P, i).len + RMDUP_BUCKET_RECORD_BYTES};
    });
}

__global__ __launch_bounds__(256) void k_rdb_pick(const uint8_t* __restrict__ buf, RecordTable t, TextTable tt, RmDupParams P,
                                                  const uint64_t* __restrict__ keys, uint32_t lo, uint32_t hi,
                                                  uint32_t* __restrict__ sub_len, uint32_t* __restrict__ keep) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.n) return;
    const uint32_t bin = (uint32_t)(keys[i] >> RMDUP_BIN_SHIFT);
    const bool in = lo <= bin && bin < hi;
    sub_len[i] = in ? subject_of(buf, t, tt, P, i).len : 0u;
    keep[i] = in ? 1u : 0u;
}

// the bytes of subject `a` to dst, by lane `gl` of `lanes`: 16 bytes per lane and step where the subject is contiguous text
// that leaves unfolded, byte by byte through the accessor otherwise (-i; wrapped FASTA)
__device__ __forceinline__ void copy_subject(const Subject& a, uint8_t* __restrict__ dst, uint32_t gl, uint32_t lanes) {
    const uint32_t len = a.len;
    if (!a.fold && !(a.seq && a.T.W)) {
        const uint8_t* src = a.seq ? a.T.p : a.h;
        for (uint32_t q = 16u * gl; q + 16u <= len; q += 16u * lanes) {
            uint4 v;
            __builtin_memcpy(&v, src + q, 16);
            __builtin_memcpy(dst + q, &v, 16);
        }
        if (gl == 0u)
            for (uint32_t q = len & ~15u; q < len; ++q) dst[q] = src[q];
    } else {
        for (uint32_t q = gl; q < len; q += lanes) dst[q] = a.at(q);
    }
}

__global__ __launch_bounds__(256) void k_rdb_pack(const uint8_t* __restrict__ buf, RecordTable t, TextTable tt, RmDupParams P,
                                                  const uint64_t* __restrict__ keys, const uint32_t* __restrict__ sub_len,
                                                  const uint64_t* __restrict__ sub_off, const uint32_t* __restrict__ keep,
                                                  const uint64_t* __restrict__ keep_off, uint64_t first_record, uint64_t n0,
                                                  uint64_t bytes0, uint8_t* __restrict__ acc, uint64_t* __restrict__ a_key,
                                                  uint64_t* __restrict__ a_gidx, uint64_t* __restrict__ a_off,
                                                  uint32_t* __restrict__ a_len) {
    const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / PACK_LANES;
    const uint32_t gl = threadIdx.x & (PACK_LANES - 1u);
    if (i >= t.n || !keep[i]) return;
    const uint32_t len = sub_len[i];
    const uint64_t at = bytes0 + sub_off[i];
    if (gl == 0u) {
        const uint64_t j = n0 + keep_off[i];
        a_key[j] = keys[i];
        a_gidx[j] = first_record + i;
        a_off[j] = at;
        a_len[j] = len;
    }
    if (len >= RMDUP_PACK_LONG) return;  // (a block of k_rdb_pack_long copies it)
    copy_subject(subject_of(buf, t, tt, P, i), acc + at, gl, PACK_LANES);
}

// one block per long subject (a chromosome under -s)
__global__ __launch_bounds__(256) void k_rdb_pack_long(const uint8_t* __restrict__ buf, RecordTable t, TextTable tt, RmDupParams P,
                                                       const uint32_t* __restrict__ sub_len, const uint64_t* __restrict__ sub_off,
                                                       uint64_t bytes0, uint8_t* __restrict__ acc,
                                                       const uint32_t* __restrict__ long_list) {
    const uint64_t i = long_list[blockIdx.x];
    if (i >= t.n || sub_len[i] < RMDUP_PACK_LONG) return;
    copy_subject(subject_of(buf, t, tt, P, i), acc + bytes0 + sub_off[i], threadIdx.x, blockDim.x);
}

// 32 records per block, PACK_LANES lanes each; the lanes of a record meet in one LDS word
__global__ __launch_bounds__(256) void k_rdb_verify(const uint8_t* __restrict__ acc, const uint64_t* __restrict__ a_off,
                                                    const uint32_t* __restrict__ a_len, const uint64_t* __restrict__ a_gidx,
                                                    const uint32_t* __restrict__ first, uint64_t n, uint32_t* __restrict__ bits,
                                                    uint32_t* __restrict__ flagged, uint32_t cap,
                                                    unsigned long long* __restrict__ n_removed) {
    constexpr uint32_t PER_BLOCK = 256 / PACK_LANES;
    __shared__ uint32_t s_diff[PER_BLOCK];
    __shared__ uint32_t s_removed;
    const uint32_t grp = threadIdx.x / PACK_LANES, gl = threadIdx.x & (PACK_LANES - 1u);
    if (threadIdx.x < PER_BLOCK) s_diff[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_removed = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * PER_BLOCK + grp;
    uint32_t f = 0;
    bool dup = false;
    if (i < n) {
        f = first[i];
        dup = f != i;
    }
    if (dup) {
        const uint32_t la = a_len[i];
        uint32_t d = la ^ a_len[f];
        if (!d) {
            const uint8_t* pa = acc + a_off[i];
            const uint8_t* pb = acc + a_off[f];
            for (uint32_t q = 16u * gl; q + 16u <= la && !d; q += PACK_STEP) {
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
    if (dup && gl == 0u) {
        if (s_diff[grp]) {
            const uint32_t pos = atomicAdd(&flagged[0], 1u);  // (the count stays exact beyond the cap)
            if (pos < cap) flagged[1 + pos] = (uint32_t)i;
        } else {
            const uint64_t g = a_gidx[i];
            atomicOr(&bits[g >> 5], 1u << (uint32_t)(g & 31u));  // (many lanes hit one word)
            atomicAdd(&s_removed, 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_removed) atomicAdd(n_removed, (unsigned long long)s_removed);
}

// the packed subjects of the records list[j] (j < m) back to back: record list[j] to out + dst_off[j]
__global__ __launch_bounds__(256) void k_rdb_gather(const uint8_t* __restrict__ acc, const uint64_t* __restrict__ a_off,
                                                    const uint32_t* __restrict__ a_len, const uint32_t* __restrict__ list,
                                                    const uint64_t* __restrict__ dst_off, uint32_t m, uint8_t* __restrict__ out) {
    const uint32_t j = (blockIdx.x * blockDim.x + threadIdx.x) / PACK_LANES;
    const uint32_t gl = threadIdx.x & (PACK_LANES - 1u);
    if (j >= m) return;
    const uint32_t i = list[j];
    const uint8_t* src = acc + a_off[i];
    uint8_t* dst = out + dst_off[j];
    const uint32_t len = a_len[i];
    for (uint32_t q = gl; q < len; q += PACK_LANES) dst[q] = src[q];
}

__global__ __launch_bounds__(256) void k_rdb_mark(const uint64_t* __restrict__ g, uint64_t m, uint32_t* __restrict__ bits) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const uint64_t v = g[j];
    atomicOr(&bits[v >> 5], 1u << (uint32_t)(v & 31u));
}

__global__ __launch_bounds__(256) void k_rdb_apply(RecordTable t, RmDupParams P, const uint32_t* __restrict__ bits,
                                                   uint64_t first_record, uint32_t* __restrict__ out_len) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.n) return;
    const uint64_t g = first_record + i;
    const bool removed = (bits[g >> 5] >> (uint32_t)(g & 31u)) & 1u;
    const uint32_t lh = t.l_head[i];
    out_len[i] = removed ? 0u : format_len(lh > 0 ? lh - 1 : 0, t.l_seq[i], P.fastq, P.line_width);
}

__global__ __launch_bounds__(256) void k_rdb_narrow(const uint64_t* __restrict__ src, uint64_t n, uint32_t* __restrict__ dst) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (uint32_t)src[i];
}

inline dim3 grid_of(uint64_t n) { return dim3((unsigned)((n + 255) / 256)); }
inline TextTable dev_tt(const TextTableH& tt) { return TextTable{tt.text_w, tt.lin_off, tt.lin, tt.lin_n}; }

}  // namespace

hipError_t launch_rdb_hist(const uint8_t* buf, const RecordTable& t, const TextTableH& tt, const RmDupParams& P, const uint64_t* keys,
                           uint64_t* bytes, uint64_t* records, int num_cus, hipStream_t st) {
    if (t.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rdb_hist, dim3(bucket_hist_blocks(t.n, num_cus)), dim3(256), 0, st, buf, t, dev_tt(tt), P, keys, (unsigned long long*)bytes,
                       (unsigned long long*)records);
    return hipGetLastError();
}

hipError_t launch_rdb_pick(const uint8_t* buf, const RecordTable& t, const TextTableH& tt, const RmDupParams& P, const uint64_t* keys,
                           uint32_t lo, uint32_t hi, uint32_t* sub_len, uint32_t* keep, hipStream_t st) {
    if (t.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rdb_pick, grid_of(t.n), dim3(256), 0, st, buf, t, dev_tt(tt), P, keys, lo, hi, sub_len, keep);
    return hipGetLastError();
}

hipError_t launch_rdb_pack(const uint8_t* buf, const RecordTable& t, const TextTableH& tt, const RmDupParams& P, const uint64_t* keys,
                           const uint32_t* sub_len, const uint64_t* sub_off, const uint32_t* keep, const uint64_t* keep_off,
                           uint64_t first_record, uint64_t n0, uint64_t bytes0, uint8_t* acc, uint64_t* a_key, uint64_t* a_gidx,
                           uint64_t* a_off, uint32_t* a_len, hipStream_t st) {
    if (t.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rdb_pack, grid_of(t.n * PACK_LANES), dim3(256), 0, st, buf, t, dev_tt(tt), P, keys, sub_len, sub_off, keep,
                       keep_off, first_record, n0, bytes0, acc, a_key, a_gidx, a_off, a_len);
    return hipGetLastError();
}

hipError_t launch_rdb_pack_long(const uint8_t* buf, const RecordTable& t, const TextTableH& tt, const RmDupParams& P,
                                const uint32_t* sub_len, const uint64_t* sub_off, uint64_t bytes0, uint8_t* acc,
                                const uint32_t* long_list, uint64_t long_count, hipStream_t st) {
    if (long_count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rdb_pack_long, dim3((unsigned)long_count), dim3(256), 0, st, buf, t, dev_tt(tt), P, sub_len, sub_off, bytes0,
                       acc, long_list);
    return hipGetLastError();
}

hipError_t launch_rdb_verify(const uint8_t* acc, const uint64_t* a_off, const uint32_t* a_len, const uint64_t* a_gidx,
                             const uint32_t* first, uint64_t n, uint32_t* bits, uint32_t* flagged, uint32_t cap, uint64_t* n_removed,
                             hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rdb_verify, grid_of(n * PACK_LANES), dim3(256), 0, st, acc, a_off, a_len, a_gidx, first, n, bits, flagged, cap,
                       (unsigned long long*)n_removed);
    return hipGetLastError();
}

hipError_t launch_rdb_gather(const uint8_t* acc, const uint64_t* a_off, const uint32_t* a_len, const uint32_t* list,
                             const uint64_t* dst_off, uint32_t m, uint8_t* out, hipStream_t st) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rdb_gather, grid_of((uint64_t)m * PACK_LANES), dim3(256), 0, st, acc, a_off, a_len, list, dst_off, m, out);
    return hipGetLastError();
}

hipError_t launch_rdb_mark(const uint64_t* g, uint64_t m, uint32_t* bits, hipStream_t st) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rdb_mark, grid_of(m), dim3(256), 0, st, g, m, bits);
    return hipGetLastError();
}

hipError_t launch_rdb_apply(const RecordTable& t, const RmDupParams& P, const uint32_t* bits, uint64_t first_record, uint32_t* out_len,
                            hipStream_t st) {
    if (t.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rdb_apply, grid_of(t.n), dim3(256), 0, st, t, P, bits, first_record, out_len);
    return hipGetLastError();
}

hipError_t launch_rdb_narrow(const uint64_t* src, uint64_t n, uint32_t* dst, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rdb_narrow, grid_of(n), dim3(256), 0, st, src, n, dst);
    return hipGetLastError();
}

}  // namespace bsk
