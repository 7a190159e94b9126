// BGZF input on the device (see ops_bgzf.hpp).
//   k_bgzf_find     every byte position of the compressed buffer is tried as the start of a block header; the few that look like
//                   one go to a list, which the host sorts and walks from offset 0 (next = position + BSIZE + 1)
//   k_bgzf_sizes    ISIZE and CRC32 of every block of the chain; launch_scan_u32 turns the sizes into output offsets
//   k_bgzf_inflate  one block per wavefront, bgzf_inflate_dev.hpp with 64 lanes: the decode is uniform (bit buffer and table
//                   entries in scalar registers), the lanes share the copies, the table fills and the CRC.  The compressed
//                   bytes come 512 at a time, 8 per lane, and are handed out with v_readlane; the window is a 32 KiB ring in
//                   LDS, from which finished bytes leave in aligned 16-byte stores.  No match ever reads global memory.
// A worker's shard of a file under --devices (bgzf_shard_load; row f20) is the same three kernels on the blocks of its range:
// the walk starts at the shard's first block and must pass through the next worker's (the join check), and k_bgzf_desc moves
// the text offsets so that the shard's first byte lands behind 64 KiB of room, a multiple of 256.
#include <hip/hip_runtime.h>

#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>

#include "../../include/bsk.h"
#include "bgzf_inflate_dev.hpp"
#include "codec_host.hpp"
#include "index.hpp"  // launch_scan_u32
#include "ops_bgzf.hpp"

namespace bsk {
namespace {

using bgzf::BgzfLds;

constexpr uint32_t HDR_MAGIC = 0x04088b1fu;  // 1f 8b 08 04
constexpr uint32_t HDR_BC = 0x00024342u;     // 'B' 'C' 02 00

// thread t looks at the positions [16 t, 16 t + 16): two 16-byte loads hold every byte the magic and the subfield tag of
// those positions can lie in; the four bytes XLEN and BSIZE of a hit are fetched on their own (about one hit per 64 KiB)
__global__ __launch_bounds__(256) void k_bgzf_find(const uint8_t* __restrict__ comp, uint64_t n, uint64_t* __restrict__ pos,
                                                   uint32_t* __restrict__ info, uint64_t cap, unsigned long long* __restrict__ count) {
    const uint64_t base = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16u;
    if (base >= n) return;
    uint32_t w[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint64_t at = base + 16u * h;
        uint32_t a = 0, b = 0, c = 0, d = 0;
        if (at + 16u <= n) {
            const uint4 v = *reinterpret_cast<const uint4*>(comp + at);
            a = v.x; b = v.y; c = v.z; d = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const uint32_t x = at + k < n ? (uint32_t)comp[at + k] << (8 * (k & 3)) : 0u;
                if (k < 4) a |= x; else if (k < 8) b |= x; else if (k < 12) c |= x; else d |= x;
            }
        }
        w[4 * h] = a; w[4 * h + 1] = b; w[4 * h + 2] = c; w[4 * h + 3] = d;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int s = 8 * (j & 3);
        const uint32_t m = s ? (w[j >> 2] >> s) | (w[(j >> 2) + 1] << (32 - s)) : w[j >> 2];
        if (m != HDR_MAGIC) continue;
        const uint32_t t = s ? (w[(j >> 2) + 3] >> s) | (w[(j >> 2) + 4] << (32 - s)) : w[(j >> 2) + 3];
        const uint64_t q = base + j;
        if (t != HDR_BC || q + 18u > n) continue;
        const uint32_t xlen = comp[q + 10] | (uint32_t)comp[q + 11] << 8, bsize = comp[q + 16] | (uint32_t)comp[q + 17] << 8;
        const unsigned long long slot = atomicAdd(count, 1ull);
        if (slot < cap) {
            pos[slot] = q;
            info[slot] = xlen << 16 | bsize;
        }
    }
}

// the trailer of block i: CRC32 and ISIZE (the host has checked that the block lies in the buffer and holds a trailer)
__global__ __launch_bounds__(256) void k_bgzf_sizes(const uint8_t* __restrict__ comp, const uint64_t* __restrict__ coff,
                                                    const uint32_t* __restrict__ csize, uint64_t nb, uint32_t* __restrict__ usize,
                                                    uint32_t* __restrict__ crc, unsigned long long* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb) return;
    const uint8_t* t = comp + coff[i] + csize[i] - 8u;
    crc[i] = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
    uint32_t v = t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
    if (v > bgzf::MAX_ISIZE) {
        atomicMin(status, (unsigned long long)(i << 8 | (uint64_t)bgzf::ERR_ISIZE));
        v = 0;
    }
    usize[i] = v;
}

// the 64 lanes of the wave that decodes a block
struct WaveLane {
    static constexpr uint32_t LANES = 64, CRC_CHUNK = 1024;
    const uint8_t* __restrict__ comp;  // the base of the block's positions: the 8-byte boundary in front of the block
    uint32_t n;                        // bytes from there to the end of the buffer (at most 2^31: more than a block ever needs)
    uint8_t* __restrict__ out;         // this block's output; (out + q) mod 16 == (shift + q) mod 16
    uint2 held;                        // bytes [4 * held_base + 8 * lane, + 8) from the base
    uint32_t held_base;
    __device__ __forceinline__ uint32_t lane() const { return threadIdx.x; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ __forceinline__ uint32_t word(uint32_t w) {
        const uint32_t cb = w & ~127u;
        if (cb != held_base) {
            held_base = cb;
            const uint32_t at = cb * 4u + threadIdx.x * 8u;
            uint2 v = make_uint2(0u, 0u);
            if (at + 8u <= n) v = *reinterpret_cast<const uint2*>(comp + at);
            else {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const uint32_t x = at + k < n ? (uint32_t)comp[at + k] << (8 * (k & 3)) : 0u;
                    if (k < 4) v.x |= x; else v.y |= x;
                }
            }
            held = v;
        }
        const int j = (int)(w & 127u);
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)held.x, j >> 1), hi = (uint32_t)__builtin_amdgcn_readlane((int)held.y, j >> 1);
        return (j & 1) ? hi : lo;
    }
    __device__ __forceinline__ uint8_t in_byte(uint32_t a) const { return comp[a]; }
    __device__ __forceinline__ uint32_t shfl(uint32_t v, uint32_t k) const { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)k); }
    // bytes [a, b) of the block: single bytes up to the first 16-byte boundary of the output and behind the last, 16 bytes a lane between
    __device__ __forceinline__ void store(const uint8_t* ring, uint32_t shift, uint32_t a, uint32_t b) const {
        const uint32_t l = threadIdx.x;
        uint32_t h = a + ((16u - ((shift + a) & 15u)) & 15u);
        if (h > b) h = b;
        if (a + l < h) out[a + l] = ring[(shift + a + l) & bgzf::RING_MASK];
        uint32_t t = b - ((shift + b) & 15u);
        if (t < h || t > b) t = h;
        for (uint32_t q = h + 16u * l; q < t; q += 16u * LANES)
            *reinterpret_cast<uint4*>(out + q) = *reinterpret_cast<const uint4*>(ring + ((shift + q) & bgzf::RING_MASK));
        if (t + l < b) out[t + l] = ring[(shift + t + l) & bgzf::RING_MASK];
    }
};

__device__ __forceinline__ uint64_t uni64(uint64_t v) {
    return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32;
}

// what k_bgzf_inflate needs of a block, in one place (k_bgzf_sizes and the scan fill usize, crc and ooff)
using BlockDesc = BgzfBlockDesc;

// one block of 64 lanes per BGZF block: nothing of the launch stays live while the block is decoded but its own description
__global__ __launch_bounds__(64) void k_bgzf_inflate(const uint8_t* __restrict__ comp, uint64_t n, const BlockDesc* __restrict__ desc,
                                                     uint8_t* __restrict__ text, const uint32_t* __restrict__ mat,
                                                     unsigned long long* __restrict__ status) {
    __shared__ BgzfLds S;
    if (threadIdx.x < 32u) S.crc_mat[threadIdx.x] = mat[threadIdx.x];
    __syncthreads();
    const uint64_t b = blockIdx.x;
    const BlockDesc d = desc[b];
    const uint64_t c0 = uni64(d.coff), o0 = uni64(d.ooff);
    const uint32_t cs = (uint32_t)__builtin_amdgcn_readfirstlane((int)d.csize), xl = (uint32_t)__builtin_amdgcn_readfirstlane((int)d.xlen);
    const uint32_t us = (uint32_t)__builtin_amdgcn_readfirstlane((int)d.usize), want = (uint32_t)__builtin_amdgcn_readfirstlane((int)d.crc);
    const uint32_t lead = (uint32_t)(c0 & 7u);
    const uint64_t rest = n - (c0 - lead);
    WaveLane io{comp + (c0 - lead), (uint32_t)(rest < 0x80000000ull ? rest : 0x80000000ull), text + o0, make_uint2(0u, 0u), ~0u};
    bgzf::Inflater<WaveLane> I(io, S);
    int rc = bgzf::ERR_TRUNCATED;
    if (cs >= 12u + xl + 8u && cs <= bgzf::MAX_ISIZE && c0 + cs <= n) rc = I.run(lead + 12u + xl, lead + cs - 8u, us, want, (uint32_t)(o0 & 15u));
    if (rc != bgzf::OK && threadIdx.x == 0) atomicMin(status, (unsigned long long)(b << 8 | (uint64_t)rc));
}

// usize, crc and the scanned offsets join the description.  obase: where the first block's text begins in the text buffer (a
// shard that begins inside its first block has that block's first bytes in the room in front of it: bgzf_shard_load)
__global__ __launch_bounds__(256) void k_bgzf_desc(uint64_t nb, const uint64_t* __restrict__ coff, const uint32_t* __restrict__ csize,
                                                   const uint32_t* __restrict__ xlen, const uint32_t* __restrict__ usize,
                                                   const uint32_t* __restrict__ crc, const uint64_t* __restrict__ ooff, uint64_t obase,
                                                   BlockDesc* __restrict__ desc) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb) return;
    desc[i] = BlockDesc{coff[i], obase + ooff[i], csize[i], xlen[i], usize[i], crc[i]};
}

// ---- host side

// How a block is named in a refusal.  A whole file: its number and its offset.  A shard (bgzf_shard_load) that begins at the file
// offset `base` > 0: its offset in the file, and its number counted from the shard's first block, said so
struct Naming {
    uint64_t base = 0;
    bool whole() const { return base == 0; }
};
std::string where(const Naming& nm, uint64_t block, uint64_t off) {
    if (nm.whole()) return "libbsk: bgzf: block " + std::to_string(block) + " at offset " + std::to_string(off) + ": ";
    return "libbsk: bgzf: block at offset " + std::to_string(nm.base + off) + " (number " + std::to_string(block) + " from the shard's first block at offset " +
           std::to_string(nm.base) + "): ";
}
constexpr uint64_t NO_JOIN = ~0ull;

// The chain of blocks from offset 0.  fetch(off, len, dst) brings bytes of the file; known(off, &h) answers from the list of
// k_bgzf_find where it can (a header whose only subfield is BC).  A header of any other shape is read through fetch.
// join (a shard's walk): an offset the chain must pass through -- the block start the next worker begins at.  A chain that steps
// over it began at, or ran through, something that is no block of the file: BSK_ERR_UNSUPPORTED, nothing is decoded
template <class Fetch, class Known>
int bgzf_walk(uint64_t n, Fetch fetch, Known known, BgzfIndex& ix, std::string& err, const Naming& nm = Naming(), uint64_t join = NO_JOIN) {
    auto where = [&nm](uint64_t block, uint64_t off) { return bsk::where(nm, block, off); };
    std::vector<uint8_t> hdr;
    for (uint64_t off = 0; off < n;) {
        const uint64_t k = ix.coff.size();
        bgzf::BlockHeader h{0, 0};
        if (!known(off, &h)) {
            const uint64_t have = n - off;
            hdr.resize((size_t)std::min<uint64_t>(have, 12));
            if (!fetch(off, (uint32_t)hdr.size(), hdr.data())) { err = "libbsk: bgzf: reading a block header back failed"; return BSK_ERR_HIP; }
            int r = bgzf::parse_header(hdr.data(), hdr.size(), &h);
            if (r == -1 && hdr.size() == 12) {
                const uint64_t full = 12ull + (hdr[10] | (uint32_t)hdr[11] << 8);
                if (full <= have) {
                    hdr.resize((size_t)full);
                    if (!fetch(off, (uint32_t)full, hdr.data())) { err = "libbsk: bgzf: reading a block header back failed"; return BSK_ERR_HIP; }
                    r = bgzf::parse_header(hdr.data(), hdr.size(), &h);
                }
            }
            if (r == -1) { err = where(k, off) + "truncated: the file ends inside the block header"; return BSK_ERR_FORMAT; }
            if (r != 1) {
                if (off == 0 && !nm.whole()) { err = where(k, off) + "the bytes there are not a block header"; return BSK_ERR_FORMAT; }
                if (off == 0 && r == 2) { err = "libbsk: bgzf: the input is gzip but not BGZF: one gzip stream cannot be cut into independent blocks; recompress it with bgzip"; return BSK_ERR_UNSUPPORTED; }
                if (off == 0) { err = "libbsk: bgzf: the input is not gzip"; return BSK_ERR_FORMAT; }
                err = where(k, off) + "the bytes after the last block are not a block header"; return BSK_ERR_FORMAT;
            }
        }
        if (h.bsize < 12u + h.xlen + 8u) { err = where(k, off) + "BSIZE is smaller than the header and the trailer"; return BSK_ERR_FORMAT; }
        if (join != NO_JOIN && off < join && off + h.bsize > join) {
            err = "libbsk: bgzf: offset " + std::to_string(nm.base + join) + " of the file is not a block start: the blocks from offset " + std::to_string(nm.base) +
                  " step over it (the block at " + std::to_string(nm.base + off) + " ends at " + std::to_string(nm.base + off + h.bsize) +
                  "), so a cut of --devices was placed on bytes that only look like a block -- the data of a block holds a whole BGZF block; "
                  "nothing was written: run the file on one device (--device N)";
            return BSK_ERR_UNSUPPORTED;
        }
        if (off + h.bsize > n) { err = where(k, off) + "truncated: BSIZE reaches past the end of the file"; return BSK_ERR_FORMAT; }
        ix.coff.push_back(off);
        ix.csize.push_back(h.bsize);
        ix.xlen.push_back(h.xlen);
        off += h.bsize;
    }
    return BSK_OK;
}

int decode_error(const BgzfIndex& ix, uint64_t packed, std::string& err, const Naming& nm = Naming()) {
    const uint64_t k = packed >> 8;
    err = where(nm, k, k < ix.coff.size() ? ix.coff[k] : 0) + bgzf::error_text((int)(packed & 255u));
    return BSK_ERR_FORMAT;
}

}  // namespace

void bgzf_crc_matrix(uint32_t mat[32]) { bgzf::crc_advance_matrix(mat, WaveLane::CRC_CHUNK); }

int bgzf_launch_inflate(const void* d_comp, uint64_t n, const BgzfBlockDesc* d_desc, uint64_t nb, void* d_text, const uint32_t* d_mat,
                        unsigned long long* d_status, void* stream) {
    if (nb == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(k_bgzf_inflate, dim3((unsigned)nb), dim3(64), 0, (hipStream_t)stream, (const uint8_t*)d_comp, n, d_desc, (uint8_t*)d_text,
                       d_mat, d_status);
    return (int)hipGetLastError();
}

int bgzf_probe(const void* head, size_t n) {
    if (!head) return 0;
    bgzf::BlockHeader h{0, 0};
    const int r = bgzf::parse_header((const uint8_t*)head, n, &h);
    // (a head that ends inside the extra field: gzip for certain, BGZF only if the BC subfield shows)
    return r == -1 ? 2 : r;
}

uint32_t bgzf_crc_chunked(const uint8_t* data, uint32_t n, uint32_t chunk) {
    uint32_t mat[32], tab[256];
    bgzf::crc_advance_matrix(mat, chunk);
    for (uint32_t i = 0; i < 256; ++i) tab[i] = bgzf::crc_table_entry(i);
    const uint32_t nchunks = (n + chunk - 1) / chunk;
    return bgzf::crc_fold(mat, nchunks, [&](uint32_t k) {
        const uint32_t ce = n - k * chunk, cs = ce > chunk ? ce - chunk : 0;
        uint32_t c = 0xFFFFFFFFu;
        for (uint32_t q = cs; q < ce; ++q) c = tab[(c ^ data[q]) & 255u] ^ (c >> 8);
        return ~c;
    });
}

namespace {
// What makes the buffer a shard of a file (bgzf_shard_load): d_comp[0] is the file's byte `base`, the text wanted begins `skip`
// bytes into the first block and ends `uhi` bytes into the block at `join` (uhi == 0: in front of it), and the chain must pass
// through `join`.  The text buffer then has BGZF_SHARD_FRONT bytes of room in front: *d_text is its base, the shard's first byte
// lies at base + BGZF_SHARD_FRONT, and *n_text counts the shard's bytes
struct Shard {
    uint64_t base = 0, join = NO_JOIN;
    uint32_t skip = 0, uhi = 0;
};

int inflate_device(const void* d_comp_, size_t n, int device, void** d_text, size_t* n_text, BgzfIndex* index, bool index_only, const Shard* sh,
                   std::string& err) {
    if (d_text) *d_text = nullptr;
    if (n_text) *n_text = 0;
    if (const int rc = select_device(device, kBgzf, err)) return rc;
    BgzfIndex local;
    BgzfIndex& ix = index ? *index : local;
    ix = BgzfIndex();
    Naming nm;
    if (sh) nm.base = sh->base;
    if (n == 0) {
        if (sh && (sh->skip || sh->uhi)) { err = "libbsk: bgzf: the virtual offsets of the shard do not lie in its blocks"; return BSK_ERR_INVALID_ARG; }
        if (!index_only) CODEC_HIP(kBgzf, hipMalloc(d_text, sh ? BGZF_SHARD_FRONT + 16 : 1));
        return BSK_OK;
    }
    const uint8_t* d_comp = (const uint8_t*)d_comp_;
    DevBuf aligned;  // (the kernels load 16 and 8 bytes at a time from multiples of 16 and 8 of the buffer)
    if (const int rc = align_input(d_comp, n, aligned, kBgzf, err)) return rc;
    // ---- the candidates
    std::vector<uint64_t> cpos;
    std::vector<uint32_t> cinfo;
    {
        CodecStage T("bgzf_find");
        uint64_t cap = n / 256 + 4096;
        for (int turn = 0; turn < 2; ++turn) {  // (a file of tiny blocks has more headers than the first list holds: once more, to size)
            DevBuf list;
            CODEC_HIP(kBgzf, list.alloc(cap * 12 + 16));
            unsigned long long* d_count = list.as<unsigned long long>();
            uint64_t* d_pos = list.as<uint64_t>() + 2;
            uint32_t* d_info = (uint32_t*)(d_pos + cap);
            CODEC_HIP(kBgzf, hipMemsetAsync(d_count, 0, 8, nullptr));
            const uint64_t threads = (n + 15) / 16;
            hipLaunchKernelGGL(k_bgzf_find, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, nullptr, d_comp, (uint64_t)n, d_pos, d_info, cap, d_count);
            CODEC_HIP(kBgzf, hipGetLastError());
            unsigned long long count = 0;
            CODEC_HIP(kBgzf, hipMemcpy(&count, d_count, 8, hipMemcpyDeviceToHost));
            if (count > cap) { cap = count; continue; }
            cpos.resize(count);
            cinfo.resize(count);
            if (count) {
                CODEC_HIP(kBgzf, hipMemcpy(cpos.data(), d_pos, count * 8, hipMemcpyDeviceToHost));
                CODEC_HIP(kBgzf, hipMemcpy(cinfo.data(), d_info, count * 4, hipMemcpyDeviceToHost));
            }
            break;
        }
    }
    // (the list comes in the order the waves reached their counter; sorted, it is in position order)
    std::vector<uint32_t> order(cpos.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (uint32_t)i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cpos[a] < cpos[b]; });
    size_t cur = 0;
    auto known = [&](uint64_t off, bgzf::BlockHeader* h) {
        while (cur < order.size() && cpos[order[cur]] < off) ++cur;  // (a candidate in front of the chain's next block is not on the chain)
        if (cur == order.size() || cpos[order[cur]] != off) return false;
        const uint32_t v = cinfo[order[cur]];
        if ((v >> 16) != 6u) return false;
        h->xlen = 6;
        h->bsize = (v & 0xFFFFu) + 1u;
        return true;
    };
    auto fetch = [&](uint64_t off, uint32_t len, uint8_t* dst) { return hipMemcpy(dst, d_comp + off, len, hipMemcpyDeviceToHost) == hipSuccess; };
    int rc = bgzf_walk(n, fetch, known, ix, err, nm, sh ? sh->join : NO_JOIN);
    if (rc != BSK_OK) return rc;
    const uint64_t nb = ix.coff.size();
    // ---- sizes and offsets
    const uint64_t scan_words = 2 * ((nb + 2047) / 2048) + 8;
    DevBuf arena;
    const size_t a_coff = 0, a_ooff = a_coff + 8 * nb, a_tmp = a_ooff + 8 * (nb + 1), a_ctl = a_tmp + 8 * scan_words, a_csize = a_ctl + 16,
                 a_xlen = a_csize + 4 * nb, a_usize = a_xlen + 4 * nb, a_crc = a_usize + 4 * nb, a_mat = a_crc + 4 * nb, a_desc = (a_mat + 128 + 15) & ~(size_t)15,
                 a_end = a_desc + sizeof(BlockDesc) * nb;
    CODEC_HIP(kBgzf, arena.alloc(a_end));
    uint8_t* A = arena.as<uint8_t>();
    unsigned long long* d_status = (unsigned long long*)(A + a_ctl);
    const unsigned long long clean = ~0ull;
    uint32_t mat[32];
    bgzf::crc_advance_matrix(mat, WaveLane::CRC_CHUNK);
    CODEC_HIP(kBgzf, hipMemcpy(A + a_coff, ix.coff.data(), 8 * nb, hipMemcpyHostToDevice));
    CODEC_HIP(kBgzf, hipMemcpy(A + a_csize, ix.csize.data(), 4 * nb, hipMemcpyHostToDevice));
    CODEC_HIP(kBgzf, hipMemcpy(A + a_xlen, ix.xlen.data(), 4 * nb, hipMemcpyHostToDevice));
    CODEC_HIP(kBgzf, hipMemcpy(d_status, &clean, 8, hipMemcpyHostToDevice));
    CODEC_HIP(kBgzf, hipMemcpy(A + a_mat, mat, 128, hipMemcpyHostToDevice));
    uint64_t total = 0;
    unsigned long long status = clean;
    {
        CodecStage T("bgzf_sizes");
        hipLaunchKernelGGL(k_bgzf_sizes, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, nullptr, d_comp, (const uint64_t*)(A + a_coff),
                           (const uint32_t*)(A + a_csize), nb, (uint32_t*)(A + a_usize), (uint32_t*)(A + a_crc), d_status);
        CODEC_HIP(kBgzf, hipGetLastError());
        CODEC_HIP(kBgzf, launch_scan_u32((const uint32_t*)(A + a_usize), (uint64_t*)(A + a_ooff), nb, (uint64_t*)(A + a_tmp), nullptr));
        CODEC_HIP(kBgzf, hipMemcpy(&total, A + a_ooff + 8 * nb, 8, hipMemcpyDeviceToHost));
        CODEC_HIP(kBgzf, hipMemcpy(&status, d_status, 8, hipMemcpyDeviceToHost));
    }
    if (status != clean) return decode_error(ix, status, err, nm);
    if (index) {
        ix.usize.resize(nb);
        CODEC_HIP(kBgzf, hipMemcpy(ix.usize.data(), A + a_usize, 4 * nb, hipMemcpyDeviceToHost));
    }
    if (index_only) return BSK_OK;
    // ---- the text (of a shard: behind the room, trimmed to its virtual offsets)
    uint64_t obase = 0, cut_front = 0, cut_back = 0;
    if (sh) {
        uint32_t first = 0, last = 0;
        CODEC_HIP(kBgzf, hipMemcpy(&first, A + a_usize, 4, hipMemcpyDeviceToHost));
        CODEC_HIP(kBgzf, hipMemcpy(&last, A + a_usize + 4 * (nb - 1), 4, hipMemcpyDeviceToHost));
        const bool in_last = sh->uhi != 0;  // (the walk has seen to it that the last block is then the one at `join`)
        if (sh->skip > first || (in_last && (ix.coff[nb - 1] != sh->join || sh->uhi > last)) || (uint64_t)sh->skip + (in_last ? last - sh->uhi : 0) > total) {
            err = "libbsk: bgzf: the virtual offsets of the shard do not lie in the text of their blocks";
            return BSK_ERR_INVALID_ARG;
        }
        cut_front = sh->skip;
        cut_back = in_last ? last - sh->uhi : 0;
        obase = BGZF_SHARD_FRONT - cut_front;
    }
    DevBuf text;
    if (!sh) {
        CODEC_HIP(kBgzf, text.alloc(total));
    } else if (text.alloc(BGZF_SHARD_FRONT + total + 16) != hipSuccess) {
        (void)hipGetLastError();
        err ="libbsk: bgzf: the shard's " + std::to_string(n) + " compressed bytes and its " + std::to_string(total) + " bytes of text do not fit the device side by side";
        return BSK_ERR_CAPACITY;
    }
    {
        CodecStage T("bgzf_inflate");
        hipLaunchKernelGGL(k_bgzf_desc, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, nullptr, nb, (const uint64_t*)(A + a_coff),
                           (const uint32_t*)(A + a_csize), (const uint32_t*)(A + a_xlen), (const uint32_t*)(A + a_usize),
                           (const uint32_t*)(A + a_crc), (const uint64_t*)(A + a_ooff), obase, (BlockDesc*)(A + a_desc));
        hipLaunchKernelGGL(k_bgzf_inflate, dim3((unsigned)nb), dim3(64), 0, nullptr, d_comp, (uint64_t)n, (const BlockDesc*)(A + a_desc),
                           text.as<uint8_t>(), (const uint32_t*)(A + a_mat), d_status);
        CODEC_HIP(kBgzf, hipGetLastError());
        CODEC_HIP(kBgzf, hipMemcpy(&status, d_status, 8, hipMemcpyDeviceToHost));
    }
    if (status != clean) return decode_error(ix, status, err, nm);
    *d_text = text.p;
    text.p = nullptr;
    *n_text = (size_t)(total - cut_front - cut_back);
    return BSK_OK;
}
}  // namespace

int bgzf_inflate_device(const void* d_comp, size_t n, int device, void** d_text, size_t* n_text, BgzfIndex* index, bool index_only,
                        std::string& err) {
    return inflate_device(d_comp, n, device, d_text, n_text, index, index_only, nullptr, err);
}

int bgzf_shard_load(int fd, uint64_t voff_lo, uint64_t voff_hi, int device, int threads, void** d_base, void** d_text, size_t* n_text,
                    std::string& err) {
    *d_base = *d_text = nullptr;
    *n_text = 0;
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) { err = "libbsk: bgzf: a shard is loaded from a regular file"; return BSK_ERR_INVALID_ARG; }
    const uint64_t size = (uint64_t)sb.st_size, clo = voff_lo >> 16, chi = voff_hi >> 16;
    Shard sh;
    sh.base = clo;
    sh.skip = (uint32_t)(voff_lo & 0xFFFFu);
    sh.uhi = (uint32_t)(voff_hi & 0xFFFFu);
    if (voff_hi < voff_lo || chi > size || (chi == size && sh.uhi)) { err = "libbsk: bgzf: bad virtual offsets of a shard"; return BSK_ERR_INVALID_ARG; }
    // the compressed bytes: from the block of the first byte to the end of the block that holds the last one
    uint64_t end = chi;
    if (sh.uhi) {
        std::vector<uint8_t> head((size_t)std::min<uint64_t>(size - chi, 65536));
        size_t at = 0;
        while (at < head.size()) {
            const ssize_t k = pread(fd, head.data() + at, head.size() - at, (off_t)(chi + at));
            if (k <= 0) { err = "libbsk: bgzf: reading the file failed"; return BSK_ERR_INVALID_ARG; }
            at += (size_t)k;
        }
        bgzf::BlockHeader h{0, 0};
        if (bgzf::parse_header(head.data(), head.size(), &h) != 1 || chi + h.bsize > size) {
            err = "libbsk: bgzf: offset " + std::to_string(chi) + " of the file, where the shard's last block should begin, holds no whole block: "
                  "the virtual offsets are not positions of this file";
            return BSK_ERR_INVALID_ARG;
        }
        end = chi + h.bsize;
    }
    if (chi < size) sh.join = chi - clo;  // (the last worker's chain ends with the file, under the rules of any BGZF file)
    const size_t n = (size_t)(end - clo);
    void* d_comp = nullptr;
    if (n) {
        const int rc = bsk_shard_load(fd, clo, n, device, threads, &d_comp);
        if (rc != BSK_OK) { err = bsk_global_error(); return rc; }
    }
    const int rc = inflate_device(d_comp, n, device, d_base, n_text, nullptr, false, &sh, err);
    if (d_comp) (void)hipFree(d_comp);
    if (rc != BSK_OK) return rc;
    *d_text = (uint8_t*)*d_base + BGZF_SHARD_FRONT;
    return BSK_OK;
}

int bgzf_inflate_host(const void* comp_, size_t n, void* out_, size_t cap, size_t* n_out, int threads, std::string& err) {
    const uint8_t* comp = (const uint8_t*)comp_;
    uint8_t* out = (uint8_t*)out_;
    if (n_out) *n_out = 0;
    BgzfIndex ix;
    auto fetch = [&](uint64_t off, uint32_t len, uint8_t* dst) { memcpy(dst, comp + off, len); return true; };
    auto known = [](uint64_t, bgzf::BlockHeader*) { return false; };
    const int rc = bgzf_walk(n, fetch, known, ix, err);
    if (rc != BSK_OK) return rc;
    const uint64_t nb = ix.coff.size();
    std::vector<uint64_t> ooff(nb + 1, 0);
    ix.usize.resize(nb);
    for (uint64_t i = 0; i < nb; ++i) {
        const uint8_t* t = comp + ix.coff[i] + ix.csize[i] - 4;
        const uint32_t v = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
        if (v > bgzf::MAX_ISIZE) return decode_error(ix, i << 8 | (uint64_t)bgzf::ERR_ISIZE, err);
        ix.usize[i] = v;
        ooff[i + 1] = ooff[i] + v;
    }
    if (n_out) *n_out = (size_t)ooff[nb];
    if (cap == 0) return BSK_OK;
    if (cap < ooff[nb] || !out) { err = "libbsk: bgzf: the output buffer holds " + std::to_string(cap) + " bytes, the text has " + std::to_string(ooff[nb]); return BSK_ERR_CAPACITY; }
    std::atomic<uint64_t> bad{~0ull};
    run_workers(threads, nb, [&](auto next) {
        std::unique_ptr<BgzfLds> S(new BgzfLds);
        memset(S->crc_mat, 0, sizeof S->crc_mat);  // (one chunk per block on the host: never applied)
        for (;;) {
            const uint64_t i = next();
            if (i >= nb) break;
            const uint8_t* t = comp + ix.coff[i] + ix.csize[i] - 8;
            const uint32_t want = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
            bgzf::HostLane io{comp + ix.coff[i], n - ix.coff[i], out + ooff[i]};
            bgzf::Inflater<bgzf::HostLane> I(io, *S);
            const int e = I.run(12u + ix.xlen[i], ix.csize[i] - 8u, ix.usize[i], want, 0);
            if (e != bgzf::OK) {
                const uint64_t mine = i << 8 | (uint64_t)e;
                uint64_t seen = bad.load();
                while (mine < seen && !bad.compare_exchange_weak(seen, mine)) {}
            }
        }
    });
    if (bad.load() != ~0ull) return decode_error(ix, bad.load(), err);
    return BSK_OK;
}

}  // namespace bsk
