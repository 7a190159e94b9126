// Plain gzip input (PARITY.md GZIP): a gzip file of any number of members in device memory becomes the text it holds, by
// speculative chunked inflate (gzip_spec_dev.hpp, ops_gzip.hip), and the same method with one lane on the host.  The entry
// points of the C ABI (capi.cpp) are thin shells of these.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace bsk {

// Every function returns a BSK_* code and leaves the text of a failure in `err`.
// d_comp[0, n) in the memory of `device` -> a new buffer *d_text of *n_text bytes (hipFree).  chunk_bytes 0: BSK_GZIP_CHUNK_BYTES,
// or the compressed size over four times the resident waves of the decode kernel, at least 256 KiB.  Any size is raised to 1 KiB
int gzip_inflate_device(const void* d_comp, size_t n, int device, size_t chunk_bytes, void** d_text, size_t* n_text, std::string& err);
// the same method with one host lane.  chunk_bytes 0: one piece.  cap == 0: only *n_out is set
int gzip_inflate_host(const void* comp, size_t n, void* out, size_t cap, size_t* n_out, size_t chunk_bytes, std::string& err);
// the numbers of the last call on this thread: chunks, chunks with a candidate, chunks on the chain, candidates that were not on
// the chain, members, text bytes, bytes decoded by chunks that were dropped, chunk size used
void gzip_last_plan(uint64_t out[8]);
// for the tests: S_k of every chunk from the library's predicate on the host (~0: none; cand[0] is ~0), and the predicate at one bit
void gzip_find_host(const void* comp, size_t n, size_t chunk_bytes, uint64_t* cand, size_t nchunks);
int gzip_header_ok_host(const void* comp, size_t n, uint64_t bit);

// a chain chunk for the kernels behind the chain
struct ChainDesc {
    uint64_t k, text_off, text, member0;
    uint32_t marker_lo, members;
};
namespace gz {
struct Geometry;
struct ChunkResult;
struct MemberRec;
struct Piece;
}
// The segment reader (gzip_stream.hpp, ops_gzip_stream.hip) launches the same kernels on a segment of a file.  Every pointer is
// device memory, d_comp a multiple of 16, `stream` a hipStream_t; each returns a hipError_t.
//   find       cand[1, nchunks) of d_comp[0, n) cut into chunks of chunk_bytes (the caller has set all of cand to ~0)
//   size       res[0, nchunks) by *d_geo, chunk 0 from the member header at byte 0
//   decode     the chain chunks d_chain[0, nchain) to d_sym, the members that end in them to d_mem + member0, res per chain chunk
//   windows    d_W[j] for j = 1 .. nchain - 1 from d_W[0], which the caller has written
//   translate  d_text[0, total) (a multiple of 16); *d_status: ~0 before, afterwards the least chain index with a marker in front
//              of its member
//   crc        d_out[i] of the text d_pieces[i] names; d_mat: the advance operator of gz::CRC_CHUNK bytes
int gzip_launch_find(const void* d_comp, uint64_t n, uint64_t chunk_bytes, uint64_t nchunks, uint64_t* d_cand, void* stream);
int gzip_launch_size(const void* d_comp, const gz::Geometry* d_geo, uint64_t nchunks, gz::ChunkResult* d_res, void* stream);
int gzip_launch_decode(const void* d_comp, const gz::Geometry* d_geo, const ChainDesc* d_chain, uint64_t nchain, uint16_t* d_sym, gz::MemberRec* d_mem,
                       gz::ChunkResult* d_res, void* stream);
int gzip_launch_windows(const ChainDesc* d_chain, uint64_t nchain, const uint16_t* d_sym, uint8_t* d_W, void* stream);
int gzip_launch_translate(const ChainDesc* d_chain, uint64_t nchain, const uint16_t* d_sym, const uint8_t* d_W, uint8_t* d_text, uint64_t total,
                          unsigned long long* d_status, void* stream);
int gzip_launch_crc(const uint8_t* d_text, const gz::Piece* d_pieces, uint64_t npieces, const uint32_t* d_mat, uint32_t* d_out, void* stream);

}  // namespace bsk
