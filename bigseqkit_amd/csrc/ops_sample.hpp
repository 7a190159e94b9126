// `sample` and `shuffle`: seeded selection / permutation of whole records (draw: sample_dev.hpp; PARITY.md SAMPLE, SHUF).
// Both are table passes in front of the verbatim copy of range / head (ops_segcopy.hip): the element is the record text
// as PlainFile + ReadFixer hand it over (RECTEXT; record_text_dev.hpp), written back followed by '\n'.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "bucket_hist_dev.hpp"
#include "index.hpp"

namespace bsk {

struct SampleParams {
    int fastq;
    uint64_t first_record;  // index of record 0 of this shard (or chunk) in the whole input
    int64_t seed;
    uint64_t lo, hi;        // record g is kept iff lo <= draw(seed, g) <= hi
};
// `sample`: (draw >> 11) < threshold, threshold = ceil(fraction * 2^53), as that interval (sample_dev.hpp sample_interval)
void sample_draw_interval(uint64_t threshold, uint64_t* lo, uint64_t* hi);

// out_len[i] = text + '\n' of record i when it is kept, else 0; keep (may be null): keep[i] = 1 / 0.  `sample` and the collect
// pass of a bucket of `shuffle` (stages k_sample_size, k_shuffle_pick)
hipError_t launch_sample_size(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, const SampleParams& P, uint32_t* out_len,
                              uint32_t* keep, uint64_t* status, hipStream_t st);
// keys[i] = draw(seed, i)
hipError_t launch_shuffle_keys(uint64_t n, int64_t seed, uint64_t* keys, hipStream_t st);
// The n records (off[i], len[i]: text + '\n') of the text base[0, extent) in the order perm: segment j = record perm[j],
// len_perm[j] = len[perm[j]], seg_src[j] = base + off[perm[j]].  n_other != null: only when the byte after the text is the
// '\n' -- else 0, counted in *n_other and written by launch_shuffle_fix; null: the texts all end in their newline
hipError_t launch_shuffle_segments(uint64_t n, const uint8_t* base, uint64_t extent, const uint64_t* off, const uint32_t* len,
                                   const uint32_t* perm, uint64_t* seg_src, uint32_t* len_perm, uint64_t* n_other, hipStream_t st);
// text + '\n' of the segments the copy left out, byte by byte (all: of every segment -- the path without the segmented copy)
hipError_t launch_shuffle_fix(uint64_t n, const uint8_t* base, const uint64_t* off, const uint32_t* perm, const uint32_t* len_perm,
                              const uint64_t* seg_off, const uint64_t* seg_src, uint8_t* out, bool all, hipStream_t st);

// ---- shuffle in buckets of the draw: BUCKET_BINS fine bins = the upper 12 bits of the draw; a bucket is a run of bins
constexpr int SHUFFLE_BIN_SHIFT = 52;
// bytes[bin] += text + '\n', records[bin] += 1 for every record of the table (bin of draw(seed, first_record + i)); the
// counters accumulate over the calls
hipError_t launch_shuffle_hist(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, int fastq, uint64_t first_record, int64_t seed,
                               uint64_t* bytes, uint64_t* records, int num_cus, hipStream_t st);
// kept record i -> entry n0 + keep_off[i] of the accumulation: its draw, bytes0 + out_off[i], out_len[i]
hipError_t launch_shuffle_append(uint64_t n, uint64_t first_record, int64_t seed, const uint32_t* out_len, const uint64_t* out_off,
                                 const uint64_t* keep_off, uint64_t n0, uint64_t bytes0, uint64_t* acc_draw, uint64_t* acc_off,
                                 uint32_t* acc_len, hipStream_t st);

}  // namespace bsk
