// `replace` (bigseqkit-lib/replace.go:127-179) on the record table: Go's Regexp.ReplaceAll with template expansion
// (regex_vm.hpp), one lane per record.
//   name (default): k_repl_heads<.., false> sizes every new head, a scan places them, k_repl_heads<.., true> writes
//                   them into a staging buffer, and k_seq_size / k_seq_emit take the head from there (SeqParams.rep_*).
//   sequence (-s, FASTA only): k_repl_seq sizes and writes whole records; a pattern that is one byte class takes a
//                   per-byte path instead of the matcher.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "index.hpp"
#include "regex_vm.hpp"

namespace bsk {

constexpr uint32_t REPL_TMPL_MAX = 1024;  // bytes of one record's template after {nr} / {kv} (longer: refused)
enum : int { REPL_ERR_NONASCII = 0, REPL_ERR_MULTI = 1, REPL_ERR_CAPT = 2, REPL_ERR_TMPL = 3, REPL_ERR_SIZE = 4, REPL_ERR_KINDS = 5 };
// a record's output (and so a staged head) stays below 2^32 bytes: the emit path sizes and places records in u32
constexpr uint64_t REPL_RECORD_MAX = 0xFFFFFFFFull;

struct ReplParams {  // device pointers
    const VmProgram* prog;
    const uint8_t* tmpl;          // -r as given
    uint32_t tmpl_len;
    const uint8_t* names;         // group names: names[name_off[g], name_off[g + 1]) for g = 0..ngroups
    const uint32_t* name_off;
    uint32_t ngroups;
    int nr_width;
    uint64_t nr_base;             // {nr} of record i = nr_base + i + 1
    int kv, keep_untouch, keep_key, icase, capt_idx, capt_over;
    const uint64_t* kv_keys;      // open addressing on fnv1a64 of the key (lower-cased with -i), 0 = empty
    const uint32_t* kv_idx;       // slot -> pair
    uint64_t kv_mask;
    const uint8_t* kv_blob;       // key of pair e: [kv_off[2e], kv_off[2e + 1]), value: [kv_off[2e + 1], kv_off[2e + 2])
    const uint64_t* kv_off;
    const uint8_t* miss;          // --key-miss-repl
    uint32_t miss_len;
    // -s
    int line_width;
    int byte_class;               // the pattern is one byte class (no anchors, not nullable): per-byte path
    int class_group1;             // ... and group 1 is that byte (else no group is referenced)
    int fastq;                    // (name path: the record's output size is checked against the u32 limit)
    uint32_t cls[8];
    unsigned long long* err;      // [REPL_ERR_KINDS] lowest offending record of each kind (~0: none)
};

// rep_len[i] = new head bytes + 1, or 0 when the head stays; WRITE: the head at stage + rep_off[i]
hipError_t launch_repl_heads(int ncap, bool write, const uint8_t* buf, const RecordTable& t, const ReplParams& R,
                             uint32_t* rep_len, const uint64_t* rep_off, uint8_t* stage, hipStream_t st);
// -s: out_len[i] = bytes of the whole output record (size pass) / the record at out + out_off[i] (write pass)
hipError_t launch_repl_seq(int ncap, bool write, const uint8_t* buf, const RecordTable& t, const uint32_t* text_w,
                           const uint64_t* lin_off, const uint8_t* lin, const ReplParams& R, uint32_t* out_len,
                           const uint64_t* out_off, uint8_t* out, hipStream_t st);

}  // namespace bsk
