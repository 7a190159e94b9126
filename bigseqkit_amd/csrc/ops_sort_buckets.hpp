// `sort` in buckets of the key (PARITY.md SORT, "Buckets"): the table passes.  The canonical key of a record (sort_key_dev.hpp)
// is mapped to a fine bin by a search among at most SORT_MAX_SPLITTERS splitter keys -- bin = number of splitters <= key, so
// equal keys share a bin and the bin is monotone in the key; a bucket is a run of consecutive bins.  One lane per record.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "bucket_hist_dev.hpp"
#include "index.hpp"
#include "ops_sort.hpp"
#include "ops_translate.hpp"  // TextTableH

namespace bsk {

constexpr uint32_t SORT_MAX_SPLITTERS = BUCKET_BINS - 1;  // (bucket_hist_dev.hpp: the counters of the histogram)
constexpr uint32_t SORT_SAMPLE_KEY_BYTES = 256;    // a sample key is cut here: a truncated key is still a valid splitter
constexpr int64_t SORT_SAMPLE_SEED = 0x534F5254;   // the fixed key of the sample's draw (sample_dev.hpp)

// the packed splitters on the device: splitter j = bytes[off[j], off[j + 1]), strictly ascending under the padded comparison
struct SortSplitters {
    const uint8_t* bytes;
    const uint32_t* off;  // [k + 1]
    uint32_t k;
};

// what the passes read of a shard: its table and text view, the key parameters, and for -l / -b the numbers of
// launch_sort_intkeys (null for the string keys)
struct SortKeySource {
    const uint8_t* buf;
    uint64_t buf_n;
    TextTableH tt;
    SortParams P;
    const uint64_t* int_keys;
};

// the sample: record i is taken when sample_draw(fixed key, first_record + i) <= hi.  Size pass: key_len[i] = bytes of its
// key, cut at SORT_SAMPLE_KEY_BYTES (0 when not taken), take[i] = 1 / 0.  Emit pass, after the scans of both: the key bytes at
// key_off[i], and (draw, length) at take_off[i]
hipError_t launch_sort_sample_size(const SortKeySource& S, const RecordTable& t, uint64_t first_record, uint64_t hi, uint32_t* key_len,
                                   uint32_t* take, hipStream_t st);
hipError_t launch_sort_sample_emit(const SortKeySource& S, const RecordTable& t, uint64_t first_record, const uint32_t* key_len,
                                   const uint64_t* key_off, const uint32_t* take, const uint64_t* take_off, uint8_t* keys, uint64_t* draws,
                                   uint32_t* lens, hipStream_t st);
// bins[i] = number of splitters <= key of record i
hipError_t launch_sort_bins(const SortKeySource& S, const RecordTable& t, const SortSplitters& sp, uint16_t* bins, hipStream_t st);
// bytes (text + '\n') and records per fine bin, added to bytes[BUCKET_BINS] / records[BUCKET_BINS]
hipError_t launch_sort_hist(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, int fastq, const uint16_t* bins, uint64_t* bytes,
                            uint64_t* records, int num_cus, hipStream_t st);
// the pick of a bucket: out_len[i] = text + '\n' of record i when lo <= bins[i] < hi, else 0; keep[i] = 1 / 0
hipError_t launch_sort_pick(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, int fastq, const uint16_t* bins, uint32_t lo,
                            uint32_t hi, uint32_t* out_len, uint32_t* keep, uint64_t* status, hipStream_t st);

}  // namespace bsk
