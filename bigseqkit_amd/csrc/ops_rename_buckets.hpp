// `rename` in buckets of the key (PARITY.md RENB): what a bucket decides.  The histogram, the pick, the pack and the key
// grouping are those of `rmdup` in buckets of the key (ops_rmdup_buckets.hpp; the subject and XXH64 are the same); a bucket of
// `rename` ends in the ORDINAL of every record inside its group of equal subjects -- one uint32_t per record of the whole
// input -- where a bucket of `rmdup` ends in one bit.  The ordinals of the members come from launch_group_sort /
// launch_group_ordinals (ops_group.hpp) on the list written here.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace bsk {

// every accumulated record i with first[i] != i is compared with first[i] on the packed subjects (8 lanes per record, 16-byte
// loads): equal -- (first[i] << 32 | i) appended to members[] (any order), *n_members counted; different -- i appended to
// flagged[1..] (flagged[0] = their exact number; entries beyond cap are dropped).  Both counters are zeroed by the caller;
// members[] holds n entries
hipError_t launch_renb_verify(const uint8_t* acc, const uint64_t* a_off, const uint32_t* a_len, const uint32_t* first, uint64_t n,
                              uint64_t* members, uint64_t* n_members, uint32_t* flagged, uint32_t cap, hipStream_t st);
// ord_global[a_gidx[i]] = ord_bucket[i] for every accumulated record i < n with ord_bucket[i] != 0 (a global index belongs to one
// bucket only: plain stores)
hipError_t launch_renb_scatter(const uint32_t* ord_bucket, const uint64_t* a_gidx, uint64_t n, uint32_t* ord_global, hipStream_t st);
// ord_global[g[j]] = v[j] for j < m (the flagged records that the host has ranked)
hipError_t launch_renb_set(const uint64_t* g, const uint32_t* v, uint64_t m, uint32_t* ord_global, hipStream_t st);

}  // namespace bsk
