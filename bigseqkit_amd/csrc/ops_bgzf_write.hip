// BGZF output on the device (see ops_bgzf_write.hpp).
//   k_bgzf_deflate  one block of text per wavefront, bgzf_deflate_dev.hpp with 64 lanes, grid-strided over the blocks.  The wave's
//                   LDS holds the hash table, the histograms, the codes and the bits of 64 tokens on their way out; the text is
//                   read where it lies (a block is 64 KiB: it stays in L2), the tokens go to a workspace of the wave in device
//                   memory, the member to a slot of a staging area.  A call goes in rounds of four blocks per resident wave, so
//                   tokens and slots are sized by the device, not by the text
//   launch_scan_u32 turns the member sizes into file offsets
//   k_bgzf_pack     moves the members from their slots into one contiguous file image; the EOF block follows when asked for
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/bsk.h"
#include "bgzf_deflate_dev.hpp"
#include "codec_host.hpp"
#include "index.hpp"  // launch_scan_u32
#include "ops_bgzf_write.hpp"

namespace bsk {
namespace {

using bgzf::DeflateLds;

constexpr uint32_t LDS_PER_CU = 160u * 1024u;
constexpr uint32_t WAVES_PER_CU = LDS_PER_CU / (uint32_t)sizeof(DeflateLds);
static_assert(WAVES_PER_CU >= 4, "the encoder's LDS is sized for four waves per CU");
constexpr uint32_t SLOTS_PER_WAVE = 4;  // blocks of a round per resident wave: 1 024 waves hold 256 MiB of text in their slots

// the 64 lanes of the wave that encodes a block
struct WaveDeflateLane {
    static constexpr uint32_t LANES = 64, CRC_CHUNK = 1024;
    const uint8_t* __restrict__ text;  // the block's text
    uint32_t* __restrict__ toks;       // the wave's tokens
    uint8_t* __restrict__ out;         // the block's slot, 16-byte aligned
    // (the lane number is handed out afresh at every use: a predicate such as lane < 8 is then computed where it is needed, and the
    // compiler does not keep dozens of 64-bit lane masks alive across the whole block loop, which it would spill)
    __device__ __forceinline__ uint32_t lane() const {
        uint32_t l = threadIdx.x;
        asm volatile("" : "+v"(l));
        return l;
    }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ __forceinline__ uint32_t shfl(uint32_t v, uint32_t k) const { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)k); }
    template <class F> __device__ __forceinline__ void for64(F f) const { f(lane()); }
    template <class F> __device__ __forceinline__ uint64_t ballot64(F f) const { return __ballot(f(lane()) ? 1 : 0); }
    __device__ __forceinline__ uint32_t scan64(uint32_t* a) const {
        const uint32_t l = lane(), v = a[l];
        uint32_t inc = v;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)inc, d, 64);
            if (l >= d) inc += t;
        }
        a[l] = inc - v;
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
        __syncthreads();
        return total;
    }
    __device__ __forceinline__ uint32_t reduce_add(uint32_t v) const {
#pragma unroll
        for (uint32_t d = 32; d > 0u; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
    }
    __device__ __forceinline__ void add(uint32_t* p, uint32_t v) const { atomicAdd(p, v); }
    __device__ __forceinline__ void or32(uint32_t* p, uint32_t v) const { atomicOr(p, v); }
    __device__ __forceinline__ void max32(uint32_t* p, uint32_t v) const { atomicMax(p, v); }
    __device__ __forceinline__ uint8_t text8(uint32_t q) const { return text[q]; }
    __device__ __forceinline__ uint32_t text32(uint32_t q) const {
        uint32_t v;
        __builtin_memcpy(&v, text + q, 4);
        return v;
    }
    __device__ __forceinline__ void tok(uint32_t i, uint32_t t) const { toks[i] = t; }
    __device__ __forceinline__ uint32_t tok_at(uint32_t i) const { return toks[i]; }
    __device__ __forceinline__ void out8(uint32_t a, uint8_t v) const { out[a] = v; }
    __device__ __forceinline__ void out32(uint32_t w, uint32_t v) const { reinterpret_cast<uint32_t*>(out)[w] = v; }
};

// what the launch is about, in device memory: the wave reads the few words a block needs when it starts that block (volatile: read
// there, not kept in scalar registers across the encoder, which has none to spare)
struct DeflateParams {
    const uint8_t* text;
    uint64_t n;
    uint32_t* toks;
    uint8_t* stage;
    uint32_t* sizes;
    uint32_t bt, nb, tok_stride, slot, waves;
    uint32_t mat[32];
};
template <class T> __device__ __forceinline__ T fresh(const T& v) { return *const_cast<const volatile T*>(&v); }

// block b is text[b * bt, min(n, (b + 1) * bt)); its member goes to stage + b * slot and its size to sizes[b].  Wave w of the
// `waves` of the grid owns toks + w * tok_stride and takes the blocks w, w + waves, ...
__global__ __launch_bounds__(64) void k_bgzf_deflate(const DeflateParams* __restrict__ P) {
    __shared__ DeflateLds S;
    if (threadIdx.x < 32u) S.crc_mat[threadIdx.x] = P->mat[threadIdx.x];
    WaveDeflateLane io{nullptr, nullptr, nullptr};
    bgzf::Deflater<WaveDeflateLane> D(io, S);
    D.init();
    for (uint32_t b = blockIdx.x; b < fresh(P->nb); b += fresh(P->waves)) {
        const uint32_t bt = fresh(P->bt);
        const uint64_t off = (uint64_t)b * bt, n = fresh(P->n);
        const uint32_t len = (uint32_t)(n - off < bt ? n - off : bt);
        io.text = fresh(P->text) + off;
        io.toks = fresh(P->toks) + (uint64_t)blockIdx.x * fresh(P->tok_stride);
        io.out = fresh(P->stage) + (uint64_t)b * fresh(P->slot);
        const uint32_t size = D.run(len);
        if (io.lane() == 0) fresh(P->sizes)[b] = size;
    }
}

// member b leaves its slot for out + off[b]: single bytes up to a 4-byte boundary of the file image and behind the last, words
// between (the slot is word-aligned and has room behind the member, so a word of the image is two words of the slot at the most)
__global__ __launch_bounds__(256) void k_bgzf_pack(const uint8_t* __restrict__ stage, uint32_t slot, const uint32_t* __restrict__ sizes,
                                                   const uint64_t* __restrict__ off, uint64_t nb, uint8_t* __restrict__ out) {
    const uint64_t b = blockIdx.x;
    const uint32_t t = threadIdx.x;
    if (b >= nb) {  // (the block behind the last: the EOF block)
        if (t < bgzf::EOF_BYTES) out[off[nb] + t] = bgzf::eof_byte(t);
        return;
    }
    const uint8_t* src = stage + b * slot;
    const uint32_t* W = reinterpret_cast<const uint32_t*>(src);
    uint8_t* dst = out + off[b];
    const uint32_t sz = sizes[b];
    uint32_t head = (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u;
    if (head > sz) head = sz;
    if (t < head) dst[t] = src[t];
    const uint32_t words = (sz - head) >> 2;
    for (uint32_t j = t; j < words; j += 256u) {
        const uint32_t s = head + 4u * j, w = s >> 2, sh = (s & 3u) * 8u;
        const uint32_t a = W[w];
        reinterpret_cast<uint32_t*>(dst + head)[j] = sh ? (a >> sh) | (W[w + 1u] << (32u - sh)) : a;
    }
    const uint32_t t0 = head + 4u * words;
    if (t0 + t < sz) dst[t0 + t] = src[t0 + t];
}

bool block_bytes_ok(uint32_t& bt, std::string& err) {
    if (bt == 0) bt = bgzf::BLOCK_TEXT;
    if (bt <= bgzf::BLOCK_TEXT) return true;
    err = "libbsk: bgzf: a block holds at most 65280 bytes of text, " + std::to_string(bt) + " asked for";
    return false;
}

}  // namespace

void bgzf_eof_block(uint8_t out[28]) {
    for (uint32_t i = 0; i < bgzf::EOF_BYTES; ++i) out[i] = bgzf::eof_byte(i);
}

size_t bgzf_deflate_bound(size_t n, uint32_t bt) {
    if (bt == 0 || bt > bgzf::BLOCK_TEXT) bt = bgzf::BLOCK_TEXT;
    const size_t nb = (n + bt - 1) / bt;
    return n + nb * bgzf::MEMBER_EXTRA + bgzf::EOF_BYTES;
}

int bgzf_deflate_device(const void* d_text, size_t n, int device, uint32_t bt, bool eof, void** d_comp, size_t* n_comp, std::string& err) {
    *d_comp = nullptr;
    *n_comp = 0;
    if (!block_bytes_ok(bt, err)) return BSK_ERR_INVALID_ARG;
    if (const int rc = select_device(device, kBgzf, err)) return rc;
    const uint64_t nb = ((uint64_t)n + bt - 1) / bt;
    if (nb >> 31) { err = "libbsk: bgzf: more than 2^31 blocks in one call"; return BSK_ERR_UNSUPPORTED; }
    DevBuf comp;
    if (nb == 0) {
        CODEC_HIP(kBgzf, comp.alloc(bgzf::EOF_BYTES));
        if (eof) {
            uint8_t e[28];
            bgzf_eof_block(e);
            CODEC_HIP(kBgzf, hipMemcpy(comp.p, e, sizeof e, hipMemcpyHostToDevice));
            *n_comp = sizeof e;
        }
        *d_comp = comp.p;
        comp.p = nullptr;
        return BSK_OK;
    }
    int cus = 0;
    CODEC_HIP(kBgzf, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    // The call goes in rounds of SLOTS_PER_WAVE blocks per resident wave, so the workspace -- the tokens of a wave, the slots the
    // members wait in until the scan says where they go -- is sized by the device, not by the text.  A text of one round (every
    // 64 MiB piece of a result is one) gets a buffer of exactly its size; a longer one a buffer of the bound, filled round by round.
    const uint64_t resident = (uint64_t)std::max(cus, 1) * WAVES_PER_CU, round_blocks = resident * SLOTS_PER_WAVE, rb = std::min<uint64_t>(nb, round_blocks);
    const uint32_t slot = bgzf::slot_bytes(bt), tok_stride = (bt + 1u + 3u) & ~3u;
    const uint64_t scan_words = 2 * ((rb + 2047) / 2048) + 8;
    // one arena: the staging slots (per block of a round), the tokens (per resident wave), the sizes, the offsets, the scan's words, the parameters
    const size_t a_stage = 0, a_toks = a_stage + (size_t)rb * slot, a_off = a_toks + (size_t)std::min<uint64_t>(rb, resident) * tok_stride * 4, a_tmp = a_off + 8 * (rb + 1),
                 a_sizes = a_tmp + 8 * scan_words, a_prm = (a_sizes + 4 * rb + 15) & ~(size_t)15, a_end = a_prm + sizeof(DeflateParams);
    DevBuf arena;
    CODEC_HIP(kBgzf, arena.alloc(a_end));
    uint8_t* A = arena.as<uint8_t>();
    DeflateParams prm{nullptr, 0, (uint32_t*)(A + a_toks), A + a_stage, (uint32_t*)(A + a_sizes), bt, 0, tok_stride, slot, 0, {}};
    bgzf::crc_advance_matrix(prm.mat, WaveDeflateLane::CRC_CHUNK);
    if (nb > rb) CODEC_HIP(kBgzf, comp.alloc(bgzf_deflate_bound(n, bt)));
    size_t bytes = 0;
    for (uint64_t b0 = 0; b0 < nb; b0 += rb) {
        const uint64_t nbr = std::min<uint64_t>(rb, nb - b0), t0 = b0 * bt;
        const bool last = b0 + nbr == nb;
        prm.text = (const uint8_t*)d_text + t0;
        prm.n = std::min<uint64_t>((uint64_t)n - t0, nbr * bt);
        prm.nb = (uint32_t)nbr;
        prm.waves = (uint32_t)std::min<uint64_t>(nbr, resident);
        // (a blocking copy on the null stream: the pack of the round before has read the slots by now)
        CODEC_HIP(kBgzf, hipMemcpy(A + a_prm, &prm, sizeof prm, hipMemcpyHostToDevice));
        uint64_t total = 0;
        {
            CodecStage T("bgzf_deflate");
            hipLaunchKernelGGL(k_bgzf_deflate, dim3(prm.waves), dim3(64), 0, nullptr, (const DeflateParams*)(A + a_prm));
            CODEC_HIP(kBgzf, hipGetLastError());
            CODEC_HIP(kBgzf, launch_scan_u32((const uint32_t*)(A + a_sizes), (uint64_t*)(A + a_off), nbr, (uint64_t*)(A + a_tmp), nullptr));
            CODEC_HIP(kBgzf, hipMemcpy(&total, A + a_off + 8 * nbr, 8, hipMemcpyDeviceToHost));
        }
        if (total > prm.n + nbr * bgzf::MEMBER_EXTRA) { err = "libbsk: bgzf: the encoder wrote more than its bound"; return BSK_ERR_HIP; }
        const bool tail = last && eof;
        if (!comp.p) CODEC_HIP(kBgzf, comp.alloc((size_t)total + (tail ? bgzf::EOF_BYTES : 0u)));
        {
            CodecStage T("bgzf_pack");
            hipLaunchKernelGGL(k_bgzf_pack, dim3((unsigned)(nbr + (tail ? 1u : 0u))), dim3(256), 0, nullptr, A + a_stage, slot, (const uint32_t*)(A + a_sizes),
                               (const uint64_t*)(A + a_off), nbr, comp.as<uint8_t>() + bytes);
            CODEC_HIP(kBgzf, hipGetLastError());
            if (last) CODEC_HIP(kBgzf, hipDeviceSynchronize());
        }
        bytes += (size_t)total + (tail ? bgzf::EOF_BYTES : 0u);
    }
    *d_comp = comp.p;
    comp.p = nullptr;
    *n_comp = bytes;
    return BSK_OK;
}

int bgzf_deflate_host(const void* text_, size_t n, uint32_t bt, bool eof, void* out_, size_t cap, size_t* n_out, int threads, std::string& err) {
    const uint8_t* text = (const uint8_t*)text_;
    uint8_t* out = (uint8_t*)out_;
    if (n_out) *n_out = 0;
    if (!block_bytes_ok(bt, err)) return BSK_ERR_INVALID_ARG;
    const uint64_t nb = ((uint64_t)n + bt - 1) / bt;
    const uint32_t slot = bgzf::slot_bytes(bt);
    std::vector<uint8_t> stage((size_t)nb * slot);
    std::vector<uint32_t> sizes(nb);
    run_workers(threads, nb, [&](auto next) {
        std::unique_ptr<DeflateLds> S(new DeflateLds);
        memset(S->crc_mat, 0, sizeof S->crc_mat);  // (one chunk per block on the host: never applied)
        std::vector<uint32_t> toks(bt + 1u);
        bgzf::HostDeflateLane io{text, toks.data(), stage.data()};
        bgzf::Deflater<bgzf::HostDeflateLane> D(io, *S);
        D.init();
        for (;;) {
            const uint64_t b = next();
            if (b >= nb) break;
            const uint64_t off = b * bt;
            io.text = text + off;
            io.out = stage.data() + b * slot;
            sizes[b] = D.run((uint32_t)(n - off < bt ? n - off : bt));
        }
    });
    uint64_t total = eof ? bgzf::EOF_BYTES : 0u;
    for (uint64_t b = 0; b < nb; ++b) total += sizes[b];
    if (n_out) *n_out = (size_t)total;
    if (cap < total || (!out && total)) { err = "libbsk: bgzf: the output buffer holds " + std::to_string(cap) + " bytes, the file has " + std::to_string(total); return BSK_ERR_CAPACITY; }
    uint64_t at = 0;
    for (uint64_t b = 0; b < nb; ++b) {
        memcpy(out + at, stage.data() + b * slot, sizes[b]);
        at += sizes[b];
    }
    if (eof) bgzf_eof_block(out + at);
    return BSK_OK;
}

}  // namespace bsk
