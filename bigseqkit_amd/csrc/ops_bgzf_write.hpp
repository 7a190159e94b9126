// BGZF output (PARITY.md BGZFW): a text in device memory becomes the BGZF file that holds it, one block per wavefront
// (ops_bgzf_write.hip), and the same encoder on host threads, with the same bytes.  The entry points of the C ABI (capi.cpp)
// are thin shells of these.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace bsk {

// Every function returns a BSK_* code and leaves the text of a failure in `err`.
// block_text_bytes: the text of a block, 0 = 65 280, at most 65 280
// the most bytes the text can become: every block stored, and the EOF block
size_t bgzf_deflate_bound(size_t n_text, uint32_t block_text_bytes);
// d_text[0, n) in the memory of `device` -> a new buffer *d_comp of *n_comp bytes (hipFree); eof: the 28-byte EOF block follows
int bgzf_deflate_device(const void* d_text, size_t n, int device, uint32_t block_text_bytes, bool eof, void** d_comp, size_t* n_comp,
                        std::string& err);
// the same encoder on `threads` host threads (<= 0: 8).  *n_out is what the file needs, also when `cap` is too small
int bgzf_deflate_host(const void* text, size_t n, uint32_t block_text_bytes, bool eof, void* out, size_t cap, size_t* n_out, int threads,
                      std::string& err);
// the EOF block
void bgzf_eof_block(uint8_t out[28]);
// (stages for bsk_profile_dump, through codec_host.hpp: "bgzf_deflate", "bgzf_pack")

}  // namespace bsk
