// `sort` in buckets of the key: the table passes (see ops_sort_buckets.hpp).  One lane per record; the key bytes come from
// the accessors that the radix passes use (sort_key_dev.hpp), the text itself is moved by the segmented copy.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ops_records.hpp"  // ERR_RECORD_TOO_LARGE
#include "ops_sort_buckets.hpp"
#include "record_text_dev.hpp"
#include "sample_dev.hpp"
#include "sort_key_dev.hpp"

namespace bsk {
namespace {

struct KeySourceDev {
    const uint8_t* buf;
    uint64_t buf_n;
    TextTable tt;
    SortParams P;
    const uint64_t* int_keys;
};

// ---- the sample: a function of the global record index alone (the draw of sample_dev.hpp under a fixed key), so the same
// records are taken however the input is cut into shards
__global__ __launch_bounds__(256) void k_sort_sample_size(KeySourceDev S, RecordTable t, uint64_t first_record, uint64_t key, uint64_t hi,
                                                          uint32_t* __restrict__ key_len, uint32_t* __restrict__ take) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.n) return;
    uint32_t len = 0, tk = 0;
    if (sample_draw(key, first_record + i) <= hi) {
        const SortKeyView K = sort_key_view(S.buf, t, S.tt, S.P, S.int_keys, i);
        len = K.len < SORT_SAMPLE_KEY_BYTES ? K.len : SORT_SAMPLE_KEY_BYTES;
        tk = 1;
    }
    key_len[i] = len;
    take[i] = tk;
}

__global__ __launch_bounds__(256) void k_sort_sample_keys(KeySourceDev S, RecordTable t, uint64_t first_record, uint64_t key,
                                                          const uint32_t* __restrict__ key_len, const uint64_t* __restrict__ key_off,
                                                          const uint32_t* __restrict__ take, const uint64_t* __restrict__ take_off,
                                                          uint8_t* __restrict__ keys, uint64_t* __restrict__ draws,
                                                          uint32_t* __restrict__ lens) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.n || !take[i]) return;
    const uint32_t len = key_len[i];
    const SortKeyView K = sort_key_view(S.buf, t, S.tt, S.P, S.int_keys, i);
    uint8_t* o = keys + key_off[i];
    for (uint32_t k = 0; k < len; ++k) o[k] = K.at(k);
    const uint64_t j = take_off[i];
    draws[j] = sample_draw(key, first_record + i);
    lens[j] = len;
}

// splitter <= key under the padded comparison?  The two are known to agree on their first `from` padded bytes; the walk leaves
// at the first differing byte and reports in *lcp a number of leading bytes on which they agree.  Behind the shorter string
// only the longer one's first non-zero byte counts, so a key longer than the splitter (a chromosome under -s) is not walked to
// its end: it is at or above its splitter whatever follows.
__device__ __forceinline__ bool splitter_le_key(const uint8_t* __restrict__ s, uint32_t sl, const SortKeyView& K, uint32_t from,
                                                uint32_t* lcp) {
    const uint32_t m = sl < K.len ? sl : K.len;
    for (uint32_t j = from; j < m; ++j) {
        const uint8_t a = K.at(j), b = s[j];
        if (a != b) { *lcp = j; return b < a; }
    }
    const uint32_t t = from > m ? from : m;
    for (uint32_t j = t; j < sl; ++j)
        if (s[j]) { *lcp = j; return false; }  // the splitter goes on with a byte above the key's padding
    *lcp = t > sl ? t : sl;                    // equal under padding up to here, or the key goes on
    return true;
}

// The splitters are sorted, so the key shares with every splitter of [lo, hi) at least the bytes it shares with BOTH ends of
// the interval (the splitter below lo, which is <= key, and the one at hi, which is above it): a step starts its walk
// there.  Keys with a long common prefix (SRR1234567.1, .2, ...) are then walked about once, not once per step.
__global__ __launch_bounds__(256) void k_sort_bins(KeySourceDev S, RecordTable t, const uint8_t* __restrict__ sp_bytes,
                                                   const uint32_t* __restrict__ sp_off, uint32_t k, uint16_t* __restrict__ bins) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.n) return;
    uint32_t lo = 0, hi = k;  // the bin lies in [lo, hi]: splitters below lo are <= key, those from hi on are above it
    if (k) {
        const SortKeyView K = sort_key_view(S.buf, t, S.tt, S.P, S.int_keys, i);
        uint32_t lcp_lo = 0, lcp_hi = 0;  // agreed bytes with the splitters lo - 1 and hi (0 while there is none)
        while (lo < hi) {  // at most 12 steps for 4095 splitters
            const uint32_t mid = (lo + hi) >> 1;
            const uint32_t a = sp_off[mid];
            uint32_t lcp;
            if (splitter_le_key(sp_bytes + a, sp_off[mid + 1] - a, K, lcp_lo < lcp_hi ? lcp_lo : lcp_hi, &lcp)) { lo = mid + 1; lcp_lo = lcp; }
            else { hi = mid; lcp_hi = lcp; }
        }
    }
    bins[i] = (uint16_t)lo;
}

// bytes (text + '\n') and records per fine bin (bucket_hist_dev.hpp), fed by the array of k_sort_bins: the bucket passes need
// that kernel on its own, and a search fused in here would carry its registers into a kernel whose occupancy the LDS already
// caps at three blocks per CU.
__global__ __launch_bounds__(256) void k_sort_hist(const uint8_t* __restrict__ buf, uint64_t buf_n, RecordTable t, int fastq,
                                                   const uint16_t* __restrict__ bins, unsigned long long* __restrict__ g_bytes,
                                                   unsigned long long* __restrict__ g_records) {
    bucket_hist(t.n, g_bytes, g_records, [&](uint64_t i) {
        return BinBytes{bins[i] & (BUCKET_BINS - 1u), record_text_len(buf, buf_n, t, fastq, i) + 1u};
    });
}

__global__ __launch_bounds__(256) void k_sort_pick(const uint8_t* __restrict__ buf, uint64_t buf_n, RecordTable t, int fastq,
                                                   const uint16_t* __restrict__ bins, uint32_t lo, uint32_t hi,
                                                   uint32_t* __restrict__ out_len, uint32_t* __restrict__ keep,
                                                   uint64_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.n) return;
    const uint32_t bin = bins[i];
    uint64_t bytes = 0;
    if (lo <= bin && bin < hi) bytes = record_text_len(buf, buf_n, t, fastq, i) + 1u;
    if (bytes > 0xFFFFFFFFull) {
        atomicOr((unsigned long long*)&status[0], (unsigned long long)ERR_RECORD_TOO_LARGE);
        bytes = 0;
    }
    out_len[i] = (uint32_t)bytes;
    keep[i] = bytes ? 1u : 0u;
}

inline dim3 grid_of(uint64_t n) { return dim3((unsigned)((n + 255) / 256)); }

inline KeySourceDev dev_of(const SortKeySource& S) {
    KeySourceDev D;
    D.buf = S.buf;
    D.buf_n = S.buf_n;
    D.tt = TextTable{S.tt.text_w, S.tt.lin_off, S.tt.lin};
    D.P = S.P;
    D.int_keys = S.int_keys;
    return D;
}

}  // namespace

hipError_t launch_sort_sample_size(const SortKeySource& S, const RecordTable& t, uint64_t first_record, uint64_t hi, uint32_t* key_len,
                                   uint32_t* take, hipStream_t st) {
    if (t.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sort_sample_size, grid_of(t.n), dim3(256), 0, st, dev_of(S), t, first_record, sample_key(SORT_SAMPLE_SEED), hi,
                       key_len, take);
    return hipGetLastError();
}

hipError_t launch_sort_sample_emit(const SortKeySource& S, const RecordTable& t, uint64_t first_record, const uint32_t* key_len,
                                   const uint64_t* key_off, const uint32_t* take, const uint64_t* take_off, uint8_t* keys, uint64_t* draws,
                                   uint32_t* lens, hipStream_t st) {
    if (t.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sort_sample_keys, grid_of(t.n), dim3(256), 0, st, dev_of(S), t, first_record, sample_key(SORT_SAMPLE_SEED),
                       key_len, key_off, take, take_off, keys, draws, lens);
    return hipGetLastError();
}

hipError_t launch_sort_bins(const SortKeySource& S, const RecordTable& t, const SortSplitters& sp, uint16_t* bins, hipStream_t st) {
    if (t.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sort_bins, grid_of(t.n), dim3(256), 0, st, dev_of(S), t, sp.bytes, sp.off, sp.k, bins);
    return hipGetLastError();
}

hipError_t launch_sort_hist(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, int fastq, const uint16_t* bins, uint64_t* bytes,
                            uint64_t* records, int num_cus, hipStream_t st) {
    if (t.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sort_hist, dim3(bucket_hist_blocks(t.n, num_cus)), dim3(256), 0, st, buf, buf_n, t, fastq, bins, (unsigned long long*)bytes,
                       (unsigned long long*)records);
    return hipGetLastError();
}

hipError_t launch_sort_pick(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, int fastq, const uint16_t* bins, uint32_t lo,
                            uint32_t hi, uint32_t* out_len, uint32_t* keep, uint64_t* status, hipStream_t st) {
    if (t.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sort_pick, grid_of(t.n), dim3(256), 0, st, buf, buf_n, t, fastq, bins, lo, hi, out_len, keep, status);
    return hipGetLastError();
}

}  // namespace bsk
