// `sample` and `shuffle`: seeded selection / permutation of whole records (draw: sample_dev.hpp; PARITY.md SAMPLE, SHUF).
// Both are table passes in front of the verbatim copy of range / head (ops_segcopy.hip): the element is the record text
// as PlainFile + ReadFixer hand it over (RECTEXT; record_text_dev.hpp), written back followed by '\n'.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "index.hpp"

namespace bsk {

struct SampleParams {
    int fastq;
    uint64_t first_record;  // index of record 0 of this shard (or chunk) in the whole input
    int64_t seed;
    uint64_t threshold;     // ceil(fraction * 2^53): record g is kept iff (draw(seed, g) >> 11) < threshold
};

// out_len[i] = text + '\n' of record i when it is kept, else 0
hipError_t launch_sample_size(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, const SampleParams& P, uint32_t* out_len,
                              uint64_t* status, hipStream_t st);
// keys[i] = draw(seed, i)
hipError_t launch_shuffle_keys(uint64_t n, int64_t seed, uint64_t* keys, hipStream_t st);
// segment j = record perm[j]: len_perm[j] = out_len[perm[j]], seg_src[j] = its address in the shard when the byte after the
// text is the '\n' (else 0, counted in *n_other and written by launch_shuffle_fix)
hipError_t launch_shuffle_segments(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, const uint32_t* out_len,
                                   const uint32_t* perm, uint64_t* seg_src, uint32_t* len_perm, uint64_t* n_other, hipStream_t st);
// text + '\n' of the segments the copy left out, byte by byte (all: of every segment -- the path without the segmented copy)
hipError_t launch_shuffle_fix(const uint8_t* buf, const RecordTable& t, const uint32_t* perm, const uint32_t* len_perm,
                              const uint64_t* seg_off, const uint64_t* seg_src, uint8_t* out, bool all, hipStream_t st);

// ---- shuffle in buckets of the draw: SHUFFLE_BINS fine bins = the upper 12 bits of the draw; a bucket is a run of bins
constexpr uint32_t SHUFFLE_BINS = 4096;
constexpr int SHUFFLE_BIN_SHIFT = 52;
// bytes[bin] += text + '\n', records[bin] += 1 for every record of the table (bin of draw(seed, first_record + i)); the
// counters accumulate over the calls
hipError_t launch_shuffle_hist(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, int fastq, uint64_t first_record, int64_t seed,
                               uint64_t* bytes, uint64_t* records, int num_cus, hipStream_t st);
// out_len[i] = text + '\n' of record i when lo <= draw <= hi (both inclusive), else 0; keep[i] = 1 / 0
hipError_t launch_shuffle_pick(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, int fastq, uint64_t first_record, int64_t seed,
                               uint64_t lo, uint64_t hi, uint32_t* out_len, uint32_t* keep, uint64_t* status, hipStream_t st);
// kept record i -> entry n0 + keep_off[i] of the accumulation: its draw, bytes0 + out_off[i], out_len[i]
hipError_t launch_shuffle_append(uint64_t n, uint64_t first_record, int64_t seed, const uint32_t* out_len, const uint64_t* out_off,
                                 const uint64_t* keep_off, uint64_t n0, uint64_t bytes0, uint64_t* acc_draw, uint64_t* acc_off,
                                 uint32_t* acc_len, hipStream_t st);
// segment j = accumulated record perm[j]: seg_src[j] = acc + acc_off[perm[j]], len_perm[j] = acc_len[perm[j]]
hipError_t launch_shuffle_bucket_segments(uint64_t n, const uint8_t* acc, const uint64_t* acc_off, const uint32_t* acc_len,
                                          const uint32_t* perm, uint64_t* seg_src, uint32_t* len_perm, hipStream_t st);
// out[seg_off[j], seg_off[j + 1]) = the bytes at seg_src[j], byte by byte (the path without the segmented copy)
hipError_t launch_shuffle_bucket_bytes(uint64_t n, const uint64_t* seg_src, const uint64_t* seg_off, uint8_t* out, hipStream_t st);

}  // namespace bsk
