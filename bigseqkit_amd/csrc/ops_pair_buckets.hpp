// `pair` in buckets of the key (PARITY.md PAIRB): what a match bucket decides, the rank step, the table passes of the order
// buckets and the sizes of the emit.  The histogram, the pick, the pack and the key grouping of the match phase are those of
// `rmdup` in buckets of the key (ops_rmdup_buckets.hpp) over file 1 followed by file 2; the classification of a sorted member
// list is launch_pair_classify (ops_group.hpp), which the one-call path uses.  The verdict is one PAIRED bit per record of
// either file -- bits1 over the index inside file 1, bits2 over the index inside file 2 -- and one 64-bit word per record of
// file 2: the global index of its mate until the rank step, the output position `pos` afterwards.  All index arithmetic is
// 64-bit.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "index.hpp"

namespace bsk {

// the rank step counts the paired bits in blocks of PAIRB_RANK_WORDS words of the bitmap: one 32-bit count per block (scanned
// into 64-bit bases) and one 16-bit prefix per word inside its block, n / 16 bytes per file
constexpr uint32_t PAIRB_RANK_WORDS = 256;
constexpr uint32_t PAIRB_RANK_RECORDS = 32u * PAIRB_RANK_WORDS;

// every accumulated record i < n is compared with first[i] on the packed subjects (8 lanes per record, 16-byte loads): the
// head of a key group (first[i] == i) and every record equal to it join members[] as (first << 32 | i), *n_members (zeroed by
// the caller) counts them; a record that differs is appended to flagged[1..] (flagged[0] = their exact number, zeroed by the
// caller; entries beyond cap are dropped)
hipError_t launch_pairb_verify(const uint8_t* acc, const uint64_t* a_off, const uint32_t* a_len, const uint32_t* first, uint64_t n,
                               uint64_t* members, uint64_t* n_members, uint32_t* flagged, uint32_t cap, hipStream_t st);
// state[i] / partner[i] as launch_pair_classify leaves them for the n accumulated records (0: not a member), a_gidx[i] = the
// global index: state 1 sets bit a_gidx[i] of bits1, state 2 sets bit a_gidx[i] - n1 of bits2 and stores the global index of the
// mate there in mates[]; *n_pairs (zeroed by the caller) counts the records of state 1.  Two records can share a word of the
// bits: atomicOr; a mate word has one writer
hipError_t launch_pairb_scatter(const uint8_t* state, const uint32_t* partner, const uint64_t* a_gidx, uint64_t n, uint64_t n1,
                                uint32_t* bits1, uint32_t* bits2, uint64_t* mates, uint64_t* n_pairs, hipStream_t st);
// the pairs that the host has settled: a[j] of file 1 and b[j] of file 2 (global indices), j < m
hipError_t launch_pairb_set(const uint64_t* a, const uint64_t* b, uint64_t m, uint64_t n1, uint32_t* bits1, uint32_t* bits2,
                            uint64_t* mates, hipStream_t st);
// the counts of the rank step over `words` words of a bitmap: wpre[w] = the set bits of the words of w's block in front of w,
// cnt[b] = the set bits of block b
hipError_t launch_pairb_count(const uint32_t* bits, uint64_t words, uint16_t* wpre, uint32_t* cnt, hipStream_t st);
// every mate word of a paired record j < n2 of file 2 becomes pos = the paired records of file 1 in front of its mate;
// *n_disorder (zeroed by the caller) counts the records whose pos differs from the paired records of file 2 in front of them
hipError_t launch_pairb_rank(const uint32_t* bits1, const uint16_t* wpre1, const uint64_t* base1, const uint32_t* bits2,
                             const uint16_t* wpre2, const uint64_t* base2, uint64_t n2, uint64_t* mates, uint64_t* n_disorder,
                             hipStream_t st);
// pos[j] of the global records first + j, j < count (after the rank step): ~0 for an unpaired one
hipError_t launch_pairb_pos(uint64_t first, uint64_t count, uint64_t n1, const uint32_t* bits1, const uint16_t* wpre1,
                            const uint64_t* base1, const uint32_t* bits2, const uint64_t* mates, uint64_t* pos, hipStream_t st);
// the order histogram of a shard of file 2 whose first record has index j0 inside the file: (pos >> shift, text + '\n') of the
// paired records (bucket_hist_dev.hpp); unpaired records count nowhere
hipError_t launch_pairb_order_hist(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, int fastq, uint64_t j0, const uint32_t* bits2,
                                   const uint64_t* mates, uint32_t shift, uint64_t* bytes, uint64_t* records, int num_cus, hipStream_t st);
// out_len[i] = text + '\n' of record i when it is paired and pos_lo <= pos < pos_hi, else 0; keep[i] = 1 / 0
hipError_t launch_pairb_order_pick(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, int fastq, uint64_t j0, const uint32_t* bits2,
                                   const uint64_t* mates, uint64_t pos_lo, uint64_t pos_hi, uint32_t* out_len, uint32_t* keep,
                                   uint64_t* status, hipStream_t st);
// the kept records of the shard join the accumulation, in shard order: (pos, byte offset, length) at n0 + keep_off[i]
hipError_t launch_pairb_order_append(uint64_t n, uint64_t j0, const uint64_t* mates, const uint32_t* out_len, const uint64_t* out_off,
                                     const uint64_t* keep_off, uint64_t n0, uint64_t bytes0, uint64_t* acc_pos, uint64_t* acc_off,
                                     uint32_t* acc_len, hipStream_t st);
// the finish of an order bucket of n records whose positions are pos_lo .. pos_lo + n - 1, each once: slots[pos[i] - pos_lo] =
// len[i] (slots zeroed by the caller) ...
hipError_t launch_pairb_order_slots(const uint64_t* pos, const uint32_t* len, uint64_t n, uint64_t pos_lo, uint32_t* slots, hipStream_t st);
// ... and, behind the scan of the slots, off[i] = slot_off[pos[i] - pos_lo].  *n_bad (zeroed by the caller) counts the records
// whose slot lies outside the bucket or holds another length: nothing is emitted then
hipError_t launch_pairb_order_offsets(const uint64_t* pos, const uint32_t* len, uint64_t n, uint64_t pos_lo, const uint32_t* slots,
                                      const uint64_t* slot_off, uint64_t* off, uint64_t* n_bad, hipStream_t st);
// the sizes of the emit: record i < n of the shard has bit j0 + i of `bits`; len_set[i] = fmt_len[i] when it is set, else 0,
// len_clear[i] the other way round; tot[0 .. 4) += bytes set, bytes clear, records set, records clear (zeroed by the caller)
hipError_t launch_pairb_apply(const uint32_t* bits, uint64_t j0, const uint32_t* fmt_len, uint64_t n, uint32_t* len_set,
                              uint32_t* len_clear, uint64_t* tot, hipStream_t st);

}  // namespace bsk
