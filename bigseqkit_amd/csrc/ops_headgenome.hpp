// head-genome (bigseqkit-lib/head_genome.go:53-108; PARITY.md HEADG): the records of the first genome.  The sequential early
// exit of the loop is restated as a verdict per record and "the first index where ...":
//   k_hg_counts   one lane per record: the words of Desc against the prefix words -> n_i (HG_NO_DESC: len(Desc) == 0)
//   k_hg_cut      block-wise minimum + one atomicMin per block: the first record that cuts, the first without a description
//   k_hg_finish   one lane: the byte where the cut record starts, n_1 of this call, where the record without description sits
// Nothing here reads the sequence text: 12 bytes of table and the header line per record.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "index.hpp"

namespace bsk {

constexpr uint32_t HG_NO_DESC = 0xFFFFFFFFu;
constexpr uint64_t HG_NONE = ~0ull;  // no record cuts / none lacks a description

// the prefix: the words of the first record's Desc, back to back in `bytes`; word k = bytes[off[k], off[k + 1])
struct HgPrefix {
    const uint8_t* bytes;
    const uint32_t* off;
    uint32_t nwords;
};

// what a window reports, device words (u64 each)
enum { HG_CUT = 0, HG_NODESC = 1, HG_N1 = 2, HG_CUT_BYTE = 3, HG_ND_START = 4, HG_ND_LHEAD = 5, HG_ND_IDOFF = 6, HG_ND_IDLEN = 7,
       HG_END = 8, HG_WORDS = 9 };

// n_i of the records [0, n_use) of the table (record `skip`, if < n_use, is the record the prefix came from: only its
// description is looked for)
hipError_t launch_hg_counts(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, uint64_t n_use, int id_mode, const HgPrefix& P,
                            uint64_t skip, uint32_t* counts, hipStream_t st);
// res[HG_CUT] / res[HG_NODESC] (both HG_NONE before) = lowest record >= first_cmp that cuts / lowest record without description;
// n_1 = n1 if n1_known, else counts[first_cmp] (the first compared record of the call)
hipError_t launch_hg_cut(const uint32_t* counts, uint64_t n_use, uint64_t first_cmp, int n1_known, uint32_t n1, uint32_t min_words,
                         uint64_t* res, hipStream_t st);
hipError_t launch_hg_finish(const uint8_t* buf, const RecordTable& t, const uint32_t* counts, uint64_t n_use, uint64_t first_cmp,
                            int id_mode, uint64_t* res, hipStream_t st);
// res[HG_END] = the first start of a 4-line FASTQ record at or behind `from` (anchor.hpp; n: none before the end)
hipError_t launch_hg_fastq_start(const uint8_t* buf, uint64_t n, uint64_t from, uint64_t* res, hipStream_t st);

}  // namespace bsk
