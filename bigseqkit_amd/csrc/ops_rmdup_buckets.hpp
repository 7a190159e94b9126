// `rmdup` in buckets of the key (PARITY.md RMDUPB): the table passes.  The fine bin of a record is the upper 12 bits of
// k1 = XXH64(subject, seed 0) (launch_rmdup_hash), so equal subjects share a bin; a bucket is a run of consecutive bins and
// accumulates the SUBJECTS of its records -- not their text -- with (k1, global index, offset, length) per record.  A bucket
// ends in a verdict: one bit per record of the whole input, set for the records that have an earlier record with the same
// subject bytes.  One lane per record unless a kernel says otherwise.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "../../include/bsk.h"
#include "bucket_hist_dev.hpp"
#include "index.hpp"
#include "ops_rmdup.hpp"
#include "ops_translate.hpp"  // TextTableH

namespace bsk {

constexpr uint32_t RMDUP_BIN_SHIFT = 52;
// what a record costs the accumulation next to its subject bytes: k1 (8), global index (8), offset (8), length (4), rounded
// up to a multiple of 8
constexpr uint64_t RMDUP_BUCKET_RECORD_BYTES = BSK_RMDUP_BUCKET_RECORD_BYTES;  // (include/bsk.h)
// a subject of at least this many bytes is packed by a block of its own (launch_find_long on the pick's lengths)
constexpr uint32_t RMDUP_PACK_LONG = 1u << 16;

// subject bytes + RMDUP_BUCKET_RECORD_BYTES and records per fine bin (bin = keys[i] >> 52), added to bytes[BUCKET_BINS] /
// records[BUCKET_BINS]
hipError_t launch_rdb_hist(const uint8_t* buf, const RecordTable& t, const TextTableH& tt, const RmDupParams& P, const uint64_t* keys,
                           uint64_t* bytes, uint64_t* records, int num_cus, hipStream_t st);
// the pick of a bucket: sub_len[i] = bytes of the subject of record i when lo <= bin < hi, else 0; keep[i] = 1 / 0 (an empty
// subject is kept with no bytes)
hipError_t launch_rdb_pick(const uint8_t* buf, const RecordTable& t, const TextTableH& tt, const RmDupParams& P, const uint64_t* keys,
                           uint32_t lo, uint32_t hi, uint32_t* sub_len, uint32_t* keep, hipStream_t st);
// after the scans of both: the subject of every kept record (folded with -i, wrapped FASTA flattened) to acc + bytes0 +
// sub_off[i], and at n0 + keep_off[i] its key, global index first_record + i, offset and length; 8 lanes per record.  The
// records of long_list (subjects of RMDUP_PACK_LONG bytes or more) are left to launch_rdb_pack_long, a block each
hipError_t launch_rdb_pack(const uint8_t* buf, const RecordTable& t, const TextTableH& tt, const RmDupParams& P, const uint64_t* keys,
                           const uint32_t* sub_len, const uint64_t* sub_off, const uint32_t* keep, const uint64_t* keep_off,
                           uint64_t first_record, uint64_t n0, uint64_t bytes0, uint8_t* acc, uint64_t* a_key, uint64_t* a_gidx,
                           uint64_t* a_off, uint32_t* a_len, hipStream_t st);
hipError_t launch_rdb_pack_long(const uint8_t* buf, const RecordTable& t, const TextTableH& tt, const RmDupParams& P,
                                const uint32_t* sub_len, const uint64_t* sub_off, uint64_t bytes0, uint8_t* acc,
                                const uint32_t* long_list, uint64_t long_count, hipStream_t st);
// every accumulated record i with first[i] != i is compared with first[i] on the packed subjects (8 lanes per record): equal
// -- bit gidx[i] of `bits` set, *n_removed counted; different -- i appended to flagged[1..] (flagged[0] = their exact number,
// zeroed by the caller; entries beyond cap are dropped)
hipError_t launch_rdb_verify(const uint8_t* acc, const uint64_t* a_off, const uint32_t* a_len, const uint64_t* a_gidx,
                             const uint32_t* first, uint64_t n, uint32_t* bits, uint32_t* flagged, uint32_t cap, uint64_t* n_removed,
                             hipStream_t st);
// the packed subjects of the accumulated records list[j] (j < m), record list[j] to out + dst_off[j] (the flagged records on
// their way to the host)
hipError_t launch_rdb_gather(const uint8_t* acc, const uint64_t* a_off, const uint32_t* a_len, const uint32_t* list,
                             const uint64_t* dst_off, uint32_t m, uint8_t* out, hipStream_t st);
// bit g[j] of `bits` set for j < m (the flagged records that lose on the host)
hipError_t launch_rdb_mark(const uint64_t* g, uint64_t m, uint32_t* bits, hipStream_t st);
// out_len[i] = formatted size of record i when bit first_record + i is clear, else 0 (the twin of launch_rmdup_apply)
hipError_t launch_rdb_apply(const RecordTable& t, const RmDupParams& P, const uint32_t* bits, uint64_t first_record, uint32_t* out_len,
                            hipStream_t st);
// dst[i] = (uint32_t)src[i] (the table path's 64-bit survivors as first[])
hipError_t launch_rdb_narrow(const uint64_t* src, uint64_t n, uint32_t* dst, hipStream_t st);

}  // namespace bsk
