// BGZF input (PARITY.md BGZF): a compressed buffer in device memory becomes the text it holds, one block per wavefront
// (ops_bgzf.hip), and the same decoder on host threads.  The entry points of the C ABI (capi.cpp) are thin shells of these.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace bsk {

// the blocks of a file, in file order: offset and size of the whole block, and the bytes it holds (ISIZE)
struct BgzfIndex {
    std::vector<uint64_t> coff;
    std::vector<uint32_t> csize, xlen, usize;
};

// Every function returns a BSK_* code and leaves the text of a failure in `err`.
// d_comp[0, n) in the memory of `device` -> a new buffer *d_text of *n_text bytes (hipFree).  index (may be null) receives the blocks.
int bgzf_inflate_device(const void* d_comp, size_t n, int device, void** d_text, size_t* n_text, BgzfIndex* index, bool index_only, std::string& err);
// A worker's shard of a BGZF file (PARITY.md BGZF "workers"): the text [voff_lo, voff_hi) of the open file `fd`, both virtual
// offsets as bgzf_cuts.hpp names them.  The compressed bytes from coffset(voff_lo) to the end of the block that holds the last
// byte come in by bsk_shard_load, the chain is walked from there and every block is written into place behind
// BGZF_SHARD_FRONT bytes of room, so *d_text = *d_base + BGZF_SHARD_FRONT (a multiple of 256) is the shard's first byte and
// there is no second copy; *d_base is what hipFree takes.  The chain must pass through coffset(voff_hi) -- the join check:
// BSK_ERR_UNSUPPORTED where it steps over it.  The text does not fit next to the compressed bytes: BSK_ERR_CAPACITY
constexpr size_t BGZF_SHARD_FRONT = 65536;
int bgzf_shard_load(int fd, uint64_t voff_lo, uint64_t voff_hi, int device, int threads, void** d_base, void** d_text, size_t* n_text,
                    std::string& err);
// the same decoder on `threads` host threads.  cap == 0: only *n_out is set
int bgzf_inflate_host(const void* comp, size_t n, void* out, size_t cap, size_t* n_out, int threads, std::string& err);
// 0: not gzip, 1: BGZF, 2: gzip that is not BGZF
int bgzf_probe(const void* head, size_t n);
// CRC32 of data[0, n), n <= 65536, the way the kernel takes it: chunks of `chunk` bytes measured from the end, folded with the
// advance operator (the tests compare it with zlib's)
uint32_t bgzf_crc_chunked(const uint8_t* data, uint32_t n, uint32_t chunk);

// what k_bgzf_inflate needs of a block: where it lies in the compressed buffer, where its text goes, and what the trailer says
struct BgzfBlockDesc {
    uint64_t coff, ooff;
    uint32_t csize, xlen, usize, crc;
};
// The streaming reader (bgzf_stream.hpp, ops_bgzf_stream.hip) launches the same kernel on a chunk of a file: the blocks
// d_desc[0, nb) of d_comp[0, n) (a multiple of 8) are written into place at d_text + ooff, d_text a multiple of 16 -- the
// kernel's aligned 16-byte stores follow the address, whatever ooff is.  d_mat: bgzf_crc_matrix in device memory; *d_status:
// ~0 before the launch, afterwards the least index << 8 | code of a block that was refused.  `stream` is a hipStream_t;
// returns a hipError_t.
int bgzf_launch_inflate(const void* d_comp, uint64_t n, const BgzfBlockDesc* d_desc, uint64_t nb, void* d_text, const uint32_t* d_mat,
                        unsigned long long* d_status, void* stream);
void bgzf_crc_matrix(uint32_t mat[32]);
// (stages for bsk_profile_dump, through codec_host.hpp: "bgzf_find", "bgzf_sizes", "bgzf_inflate", and of the reader "bgzf_stream_cut")

}  // namespace bsk
