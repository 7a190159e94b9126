// `concat` in buckets of the key (PARITY.md CONB): what a match bucket decides, the weights of the heads, the window histogram,
// the two picks of a window and the sizes of the tail.  The histogram, the pick, the pack and the key grouping of the match
// phase are those of `rmdup` in buckets of the key (ops_rmdup_buckets.hpp) over file 1 followed by file 2.  The verdict is one
// 64-bit word per record of either file, over the global index g: head[g] = the lowest record of file 1 (n1 records) with the
// subject bytes of g, CATB_NONE when file 1 has none.  W[h] / C[h], over the index inside file 1, are the text bytes / the number
// of the records of file 2 whose head is h; the mark bits, one per record of file 1, name the heads of the records of the open
// window.  All index arithmetic is 64-bit.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "index.hpp"

namespace bsk {

constexpr uint64_t CATB_NONE = ~0ull;

// every accumulated record i < n is compared with first[i] on the packed subjects (8 lanes per record, 16-byte loads): the head
// of a key group (first[i] == i) and every record equal to it get head[a_gidx[i]] = a_gidx[first[i]] when that lies in file 1,
// else CATB_NONE -- one writer per word --, *n_matched (zeroed by the caller) counts the words other than CATB_NONE; a record
// that differs is appended to flagged[1..] (flagged[0] = their exact number, zeroed by the caller; entries beyond cap are dropped)
hipError_t launch_catb_verify(const uint8_t* acc, const uint64_t* a_off, const uint32_t* a_len, const uint64_t* a_gidx, const uint32_t* first,
                              uint64_t n, uint64_t n1, uint64_t* head, uint32_t* flagged, uint32_t cap, uint64_t* n_matched, hipStream_t st);
// the heads that the host has settled: head[g[j]] = h[j], j < m
hipError_t launch_catb_set(const uint64_t* g, const uint64_t* h, uint64_t m, uint64_t* head, hipStream_t st);
// a shard of file 2 whose first record has global index g0: W[head] += text + '\n', C[head] += 1 for every record with a head
hipError_t launch_catb_weigh(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, int fastq, uint64_t g0, const uint64_t* head,
                             uint64_t* W, uint64_t* C, hipStream_t st);
// the window histogram of a shard of file 1 whose first record has index a0: (a >> shift, t(a) * (1 + C[h]) + 2 * W[h]) with
// h = head[a] (bucket_hist_dev.hpp)
hipError_t launch_catb_hist(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, int fastq, uint64_t a0, const uint64_t* head,
                            const uint64_t* W, const uint64_t* C, uint32_t shift, uint64_t* bytes, uint64_t* records, int num_cus,
                            hipStream_t st);
// a shard of file 1: out_len[i] = text + '\n' of record a = a0 + i when lo_bin <= a >> shift < hi_bin, else 0; keep[i] = 1 / 0;
// a kept record sets the mark bit of its head (two records can share a word of the bits: atomicOr)
hipError_t launch_catb_mark(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, int fastq, uint64_t a0, const uint64_t* head,
                            uint32_t shift, uint32_t lo_bin, uint32_t hi_bin, uint32_t* mark, uint32_t* out_len, uint32_t* keep,
                            uint64_t* status, hipStream_t st);
// a shard of file 2: out_len[i] = text + '\n' of record g0 + i when it has a head whose mark bit is set, else 0; keep[i] = 1 / 0
hipError_t launch_catb_pick(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, int fastq, uint64_t g0, const uint64_t* head,
                            const uint32_t* mark, uint32_t* out_len, uint32_t* keep, uint64_t* status, hipStream_t st);
// the sizes of the tail: out_len[i] = 0 where record g0 + i, i < n, has a head
hipError_t launch_catb_tail(const uint64_t* head, uint64_t g0, uint64_t n, uint32_t* out_len, hipStream_t st);

}  // namespace bsk
