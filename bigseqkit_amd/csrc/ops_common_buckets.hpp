// `common` in buckets of the key (PARITY.md COMB): what a bucket decides, and the sizes of the emit.  The histogram, the pick,
// the pack and the key grouping are those of `rmdup` in buckets of the key (ops_rmdup_buckets.hpp; the subject and XXH64 are
// the same) over the union of the files; a bucket of `common` ends in one KEEP bit per record of the FIRST file: set for the
// first occurrence of a subject that every file holds.  The file of a record follows from its global index and the running
// sums of the records per file (at most COMMON_MAX_FILES entries, read into LDS); all index arithmetic is 64-bit.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>


namespace bsk {

constexpr uint32_t COMMON_MAX_FILES = 64;  // one bit of a 64-bit mask per file

// masks[i] (n words, zeroed by the caller) of the HEAD i of a key group (first[i] == i) collects the files of the group: the
// head ORs the bit of its own file, and every accumulated record i with first[i] != i is compared with first[i] on the packed
// subjects (8 lanes per record, 16-byte loads): equal -- the bit of its file ORed into masks[first[i]]; different -- i appended
// to flagged[1..] (flagged[0] = their exact number, zeroed by the caller; entries beyond cap are dropped).  The file of record
// i = the number of file_sums[0 .. n_files) that are <= a_gidx[i]
hipError_t launch_comb_verify(const uint8_t* acc, const uint64_t* a_off, const uint32_t* a_len, const uint64_t* a_gidx,
                              const uint32_t* first, uint64_t n, const uint64_t* file_sums, uint32_t n_files, uint64_t* masks,
                              uint32_t* flagged, uint32_t cap, hipStream_t st);
// keep bit a_gidx[i] of `bits` set for every head i whose mask equals `full` and whose global index lies below first_file_records;
// *n_kept (zeroed by the caller) counts them.  Two heads can share a word: atomicOr
hipError_t launch_comb_decide(const uint32_t* first, const uint64_t* a_gidx, const uint64_t* masks, uint64_t n, uint64_t full,
                              uint64_t first_file_records, uint32_t* bits, uint64_t* n_kept, hipStream_t st);
// keep bit g[j] of `bits` set for j < m (the flagged records that the host has settled)
hipError_t launch_comb_set(const uint64_t* g, uint64_t m, uint32_t* bits, hipStream_t st);
// out_len[i] = 0 for every record i < n of the shard whose keep bit first_record + i is clear (the inverse sense of
// launch_rdb_apply; the sizes of the kept records are those launch_seq_size wrote, as in common_run_device)
hipError_t launch_comb_apply(const uint32_t* bits, uint64_t first_record, uint64_t n, uint32_t* out_len, hipStream_t st);

}  // namespace bsk
