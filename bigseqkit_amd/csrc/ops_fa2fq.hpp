// `fa2fq` (bigseqkit-lib/fa2fq.go:59-120, behaviour as decided in PARITY.md FA2FQ) on the record table: the record's ID
// is looked up in a table of FASTA records, the FASTA sequence is searched in the read on both strands, and the hit is
// written as a FASTQ record sliced to it.
//   k_fa2fq_match      : one lane per record -- FNV-1a probe, byte verification, then the search when the read leaves at
//                        most FA2FQ_LANE_POS start positions; longer searches are listed
//   k_fa2fq_match_wave : one wave per listed record, 64 start positions per step
//   (finish_sizes: the scan over the output lengths)
//   k_fa2fq_emit       : 16 lanes per record, 16 output bytes per lane and step; records of a MiB or more by whole blocks
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "index.hpp"

namespace bsk {

// start positions (l_seq - needle + 1) up to which one lane searches a record; above, a wave does
constexpr uint32_t FA2FQ_LANE_POS = 64;
constexpr uint32_t FA2FQ_NONE = 0xFFFFFFFFu;   // ent[i]: the record has no output
constexpr uint32_t FA2FQ_MINUS = 0x80000000u;  // ent[i]: the hit is on the reverse-complemented read
// an output record stays below 2^32 bytes (sizes are placed in u32, offsets in u64)
constexpr uint64_t FA2FQ_RECORD_MAX = 0xFFFFFFFFull;

struct Fa2FqParams {  // device pointers
    const uint64_t* keys;      // open addressing on fnv1a64 of the full FASTA name, 0 = empty
    const uint32_t* idx;       // slot -> entry
    uint64_t mask;
    const uint64_t* name_off;  // name of entry e: names[name_off[e], name_off[e + 1])
    const uint8_t* names;
    const uint64_t* seq_off;   // sequence of entry e: seqs[seq_off[e], seq_off[e + 1]); the block is padded by 16 bytes
    const uint8_t* seqs;
    const uint8_t* comp;       // complement map of the partition's alphabet (256 bytes)
    int only_plus;
    int id_mode;
    const uint8_t* buf_end;
    unsigned long long* ctl;   // [0] listed records, [1] lowest record whose output would reach 2^32 bytes (~0: none)
};

// ent[i] = entry | strand, or FA2FQ_NONE; pos[i] = i of the hit in the (reversed) read; out_len[i] = bytes of the output
hipError_t launch_fa2fq_match(const uint8_t* buf, const RecordTable& t, const Fa2FqParams& P, uint32_t* ent, uint32_t* pos,
                              uint32_t* out_len, uint32_t* list, hipStream_t st);
hipError_t launch_fa2fq_emit(const uint8_t* buf, const RecordTable& t, const Fa2FqParams& P, const uint32_t* ent,
                             const uint32_t* pos, const uint32_t* out_len, const uint64_t* out_off, uint8_t* out,
                             const uint32_t* long_list, uint64_t long_count, uint64_t long_max, uint32_t long_thresh,
                             hipStream_t st);

}  // namespace bsk
