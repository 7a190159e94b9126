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

}  // namespace bsk
