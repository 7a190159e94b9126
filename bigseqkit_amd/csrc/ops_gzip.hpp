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

}  // namespace bsk
