// Plain gzip input on the device (see ops_gzip.hpp, gzip_spec_dev.hpp).
//   k_gz_find       one workgroup per chunk behind the first, one lane per bit position: gz::header_ok in windows of 8 KiB of
//                   compressed bytes, the lowest hit of the first window that has one is S_k
//   k_gz_size       one wave per chunk that has a candidate, and chunk 0: gz::Walker without output; LDS holds the tables only
//   k_gz_decode     one wave per chain chunk: gz::Walker writing 16-bit symbols through a ring of 32 Ki symbols in LDS
//   k_gz_windows    ONE workgroup that walks the chain chunks in order, a barrier between two of them: the step is 32 KiB of
//                   work, so a launch per chunk would cost more in launches than in work
//   k_gz_translate  a thread per 16 bytes of text: symbols become bytes, markers through the chunk's window
//   k_gz_crc        one wave per piece of at most 64 KiB of text, lanes take 1 KiB chunks from the piece's end (bgzf::crc_fold)
// The host walks the chain between size and decode, and joins the CRC pieces of each member at the end: four read-backs a call.
// The lane policy of the walks is gzip_wave_dev.hpp; the launchers at the end of the host side hand the same kernels to the
// segment reader (ops_gzip_stream.hip), which runs them on a segment of a file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/bsk.h"
#include "codec_host.hpp"
#include "gzip_spec_dev.hpp"
#include "gzip_wave_dev.hpp"
#include "ops_gzip.hpp"

namespace bsk {
namespace {

using gz::ChunkResult;
using gz::GzWaveLane;
using gz::MemberRec;

__device__ __forceinline__ uint32_t load_word(const uint8_t* __restrict__ comp, uint64_t n, uint64_t w) {
    const uint64_t a = 4u * w;
    if (a + 4u <= n) return *reinterpret_cast<const uint32_t*>(comp + a);
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (a + k < n) v |= (uint32_t)comp[a + k] << (8 * k);
    return v;
}

__global__ __launch_bounds__(256) void k_gz_find(const uint8_t* __restrict__ comp, uint64_t n, uint64_t chunk_bytes, uint64_t* __restrict__ cand) {
    __shared__ unsigned long long best;
    const uint64_t k = (uint64_t)blockIdx.x + 1u;
    const uint64_t lo = k * chunk_bytes * 8u, hi = (k + 1u) * chunk_bytes < n ? (k + 1u) * chunk_bytes * 8u : n * 8u;
    if (threadIdx.x == 0) best = gz::NONE;
    __syncthreads();
    auto word = [&](uint64_t w) { return load_word(comp, n, w); };
    for (uint64_t base = lo; base < hi; base += 8ull * gz::FIND_STEP) {
        const uint64_t end = base + 8ull * gz::FIND_STEP < hi ? base + 8ull * gz::FIND_STEP : hi;
        for (uint64_t pos = base + threadIdx.x; pos < end; pos += 256u)
            if (gz::header_ok(word, n * 8u, pos)) {
                atomicMin(&best, (unsigned long long)pos);
                break;  // (this lane's later positions are higher)
            }
        __syncthreads();
        const unsigned long long seen = best;
        __syncthreads();  // (nobody is in the next window, and lowers `best`, before everybody has read it: all leave together)
        if (seen != gz::NONE) break;
    }
    if (threadIdx.x == 0) cand[k] = best;
}

__global__ __launch_bounds__(64) void k_gz_size(const uint8_t* __restrict__ comp, const gz::Geometry* __restrict__ G, ChunkResult* __restrict__ res) {
    __shared__ gz::GzTables T;
    const uint64_t k = blockIdx.x;
    if (k != 0 && G->cand[k] == gz::NONE) {  // (the same in every lane)
        if (threadIdx.x == 0) res[k] = ChunkResult{gz::NONE, 0, gz::NONE, 0, 0, 0};
        return;
    }
    if (threadIdx.x == 0) T.park = gz::Parked{*G, k, 0, k ? gz::NONE : 0, nullptr, nullptr, 0};
    __syncthreads();
    GzWaveLane io{comp, G->n, make_uint2(0u, 0u), ~0u};
    gz::Walker<GzWaveLane, false> W(io, T, nullptr);
    const ChunkResult R = W.run(0);
    if (threadIdx.x == 0) res[blockIdx.x] = R;
}

__global__ __launch_bounds__(64) void k_gz_decode(const uint8_t* __restrict__ comp, const gz::Geometry* __restrict__ G,
                                                  const ChainDesc* __restrict__ chain, uint16_t* __restrict__ sym, MemberRec* __restrict__ mem,
                                                  ChunkResult* __restrict__ res) {
    __shared__ gz::GzDecodeLds S;
    const ChainDesc d = chain[blockIdx.x];
    if (threadIdx.x == 0) S.T.park = gz::Parked{*G, d.k, d.text, d.k ? gz::NONE : 0, mem + d.member0, sym + d.text_off, d.members};
    __syncthreads();
    GzWaveLane io{comp, G->n, make_uint2(0u, 0u), ~0u};
    gz::Walker<GzWaveLane, true> W(io, S.T, S.ring);
    const ChunkResult R = W.run((uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)d.text_off & 7u)));
    if (threadIdx.x == 0) res[blockIdx.x] = R;
}

// W[j] from W[j - 1] and the symbols of chain chunk j - 1, j = 1 .. in order.  W[0] is zero (the host clears it)
__global__ __launch_bounds__(1024) void k_gz_windows(const ChainDesc* __restrict__ chain, uint64_t nchain, const uint16_t* __restrict__ sym,
                                                     uint8_t* __restrict__ W) {
    for (uint64_t j = 1; j < nchain; ++j) {
        uint8_t* Wj = W + j * gz::WIN;
        const uint8_t* Wi = Wj - gz::WIN;
        const int64_t start_i = (int64_t)chain[j - 1].text_off, start_j = (int64_t)chain[j].text_off;
        for (uint32_t m = threadIdx.x; m < gz::WIN; m += 1024u) {
            const int64_t pos = start_j - (int64_t)gz::WIN + m;
            uint8_t v;
            if (pos >= start_i) {
                const uint16_t s = sym[pos];
                v = s < 0x8000u ? (uint8_t)s : Wi[s & 0x7FFFu];
            } else {
                v = Wi[pos - start_i + (int64_t)gz::WIN];
            }
            Wj[m] = v;
        }
        __threadfence();
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_gz_translate(const ChainDesc* __restrict__ chain, uint64_t nchain, const uint16_t* __restrict__ sym,
                                                      const uint8_t* __restrict__ W, uint8_t* __restrict__ text, uint64_t total,
                                                      unsigned long long* __restrict__ status) {
    const uint64_t q0 = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 16u;
    if (q0 >= total) return;
    uint64_t lo = 0, hi = nchain;  // the last chain chunk whose text begins at or before q0
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) / 2;
        if (chain[mid].text_off <= q0) lo = mid; else hi = mid;
    }
    uint64_t c = lo;
    uint32_t mlo = chain[c].marker_lo;
    uint64_t next = c + 1 < nchain ? chain[c + 1].text_off : ~0ull;
    const uint32_t cnt = total - q0 < 16u ? (uint32_t)(total - q0) : 16u;
    uint16_t s[16];
    if (cnt == 16u) {
        const uint4 a = *reinterpret_cast<const uint4*>(sym + q0), b = *reinterpret_cast<const uint4*>(sym + q0 + 8);
        const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = (uint16_t)(w[i >> 1] >> (16 * (i & 1)));
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = (uint32_t)i < cnt ? sym[q0 + i] : (uint16_t)0;
    }
    uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint64_t q = q0 + i;
        while (q >= next) {
            ++c;
            mlo = chain[c].marker_lo;
            next = c + 1 < nchain ? chain[c + 1].text_off : ~0ull;
        }
        uint32_t v = s[i];
        if (v & 0x8000u) {
            const uint32_t m = v & 0x7FFFu;
            if (m < mlo && (uint32_t)i < cnt) atomicMin(status, (unsigned long long)c);
            v = W[c * gz::WIN + m];
        }
        o[i >> 2] |= (v & 255u) << (8 * (i & 3));
    }
    if (cnt == 16u) *reinterpret_cast<uint4*>(text + q0) = make_uint4(o[0], o[1], o[2], o[3]);
    else
        for (uint32_t i = 0; i < cnt; ++i) text[q0 + i] = (uint8_t)(o[i >> 2] >> (8 * (i & 3)));
}

__global__ __launch_bounds__(64) void k_gz_crc(const uint8_t* __restrict__ text, const gz::Piece* __restrict__ pieces, const uint32_t* __restrict__ mat,
                                               uint32_t* __restrict__ out) {
    __shared__ uint32_t tab[256];
    __shared__ uint32_t M[32];
    for (uint32_t i = threadIdx.x; i < 256u; i += 64u) tab[i] = bgzf::crc_table_entry(i);
    if (threadIdx.x < 32u) M[threadIdx.x] = mat[threadIdx.x];
    __syncthreads();
    const gz::Piece p = pieces[blockIdx.x];
    const uint32_t len = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.len);
    const uint32_t back = threadIdx.x * gz::CRC_CHUNK;
    uint32_t c = 0xFFFFFFFFu;
    if (back < len) {
        const uint32_t ce = len - back, cs = ce > gz::CRC_CHUNK ? ce - gz::CRC_CHUNK : 0u;
        const uint8_t* t = text + p.off;
        for (uint32_t q = cs; q < ce; ++q) c = tab[(c ^ t[q]) & 255u] ^ (c >> 8);
    }
    const uint32_t mine = ~c;
    const uint32_t nchunks = (len + gz::CRC_CHUNK - 1u) / gz::CRC_CHUNK;
    const uint32_t got = bgzf::crc_fold(M, nchunks, [&](uint32_t k) { return (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)k); });
    if (threadIdx.x == 0) out[blockIdx.x] = got;
}

// ---- host side

thread_local gz::Plan g_plan;

int fail_code(int f) { return f == gz::FAIL_UNSUPPORTED ? BSK_ERR_UNSUPPORTED : BSK_ERR_FORMAT; }

}  // namespace

void gzip_last_plan(uint64_t out[8]) { g_plan.to(out); }

// ---- the kernels for the segment reader (ops_gzip.hpp): nothing is launched over an empty grid
int gzip_launch_find(const void* d_comp, uint64_t n, uint64_t chunk_bytes, uint64_t nchunks, uint64_t* d_cand, void* stream) {
    if (nchunks > 1) hipLaunchKernelGGL(k_gz_find, dim3((unsigned)(nchunks - 1)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)d_comp, n, chunk_bytes, d_cand);
    return (int)hipGetLastError();
}
int gzip_launch_size(const void* d_comp, const gz::Geometry* d_geo, uint64_t nchunks, ChunkResult* d_res, void* stream) {
    if (nchunks) hipLaunchKernelGGL(k_gz_size, dim3((unsigned)nchunks), dim3(64), 0, (hipStream_t)stream, (const uint8_t*)d_comp, d_geo, d_res);
    return (int)hipGetLastError();
}
int gzip_launch_decode(const void* d_comp, const gz::Geometry* d_geo, const ChainDesc* d_chain, uint64_t nchain, uint16_t* d_sym, MemberRec* d_mem,
                       ChunkResult* d_res, void* stream) {
    if (nchain) hipLaunchKernelGGL(k_gz_decode, dim3((unsigned)nchain), dim3(64), 0, (hipStream_t)stream, (const uint8_t*)d_comp, d_geo, d_chain, d_sym, d_mem, d_res);
    return (int)hipGetLastError();
}
int gzip_launch_windows(const ChainDesc* d_chain, uint64_t nchain, const uint16_t* d_sym, uint8_t* d_W, void* stream) {
    if (nchain > 1) hipLaunchKernelGGL(k_gz_windows, dim3(1), dim3(1024), 0, (hipStream_t)stream, d_chain, nchain, d_sym, d_W);
    return (int)hipGetLastError();
}
int gzip_launch_translate(const ChainDesc* d_chain, uint64_t nchain, const uint16_t* d_sym, const uint8_t* d_W, uint8_t* d_text, uint64_t total,
                          unsigned long long* d_status, void* stream) {
    const uint64_t threads = (total + 15) / 16;
    if (total && nchain) hipLaunchKernelGGL(k_gz_translate, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_chain, nchain, d_sym, d_W, d_text, total, d_status);
    return (int)hipGetLastError();
}
int gzip_launch_crc(const uint8_t* d_text, const gz::Piece* d_pieces, uint64_t npieces, const uint32_t* d_mat, uint32_t* d_out, void* stream) {
    if (npieces) hipLaunchKernelGGL(k_gz_crc, dim3((unsigned)npieces), dim3(64), 0, (hipStream_t)stream, d_text, d_pieces, d_mat, d_out);
    return (int)hipGetLastError();
}

void gzip_find_host(const void* comp, size_t n, size_t chunk_bytes, uint64_t* cand, size_t nchunks) {
    for (size_t k = 0; k < nchunks; ++k) cand[k] = k ? gz::find_host((const uint8_t*)comp, n, chunk_bytes, k) : gz::NONE;
}

int gzip_header_ok_host(const void* comp, size_t n, uint64_t bit) {
    const gz::HostLane io{(const uint8_t*)comp, n};
    return gz::header_ok([&](uint64_t w) { return io.word(w); }, (uint64_t)n * 8u, bit) ? 1 : 0;
}

int gzip_inflate_host(const void* comp, size_t n, void* out, size_t cap, size_t* n_out, size_t chunk_bytes, std::string& err) {
    if (n_out) *n_out = 0;
    if (chunk_bytes && chunk_bytes < 1024) chunk_bytes = 1024;
    // a size query has inflated the text: it waits for the call that brings the buffer (same bytes, same chunk size), which
    // copies it.  Held once, by the thread that asked; any other call drops it
    struct Kept { uint64_t hash = 0; size_t n = 0, chunk = 0; std::vector<uint8_t> text; gz::Plan plan; bool full = false; };
    thread_local Kept kept;
    uint64_t hash = 0xcbf29ce484222325ull;  // (of the compressed bytes: the same address may hold other bytes by now)
    for (size_t i = 0; i < n; ++i) hash = (hash ^ ((const uint8_t*)comp)[i]) * 0x100000001b3ull;
    std::vector<uint8_t> text;
    if (kept.full && cap != 0 && kept.hash == hash && kept.n == n && kept.chunk == chunk_bytes) {
        text.swap(kept.text);
        g_plan = kept.plan;
        kept = Kept();
    } else {
        kept = Kept();
        const int f = gz::inflate_host((const uint8_t*)comp, n, chunk_bytes, text, g_plan, err);
        if (f) return fail_code(f);
    }
    if (cap == 0) {
        if (n_out) *n_out = text.size();
        kept.hash = hash; kept.n = n; kept.chunk = chunk_bytes; kept.plan = g_plan; kept.full = true;
        kept.text.swap(text);
        return BSK_OK;
    }
    if (n_out) *n_out = text.size();
    if (cap < text.size() || !out) { err = "libbsk: gzip: the output buffer holds " + std::to_string(cap) + " bytes, the text has " + std::to_string(text.size()); return BSK_ERR_CAPACITY; }
    if (!text.empty()) memcpy(out, text.data(), text.size());
    return BSK_OK;
}

int gzip_inflate_device(const void* d_comp_, size_t n, int device, size_t chunk_bytes, void** d_text, size_t* n_text, std::string& err) {
    *d_text = nullptr;
    *n_text = 0;
    g_plan = gz::Plan();
    if (const int rc = select_device(device, kGzip, err)) return rc;
    if (n == 0) {
        CODEC_HIP(kGzip, hipMalloc(d_text, 1));
        return BSK_OK;
    }
    const uint8_t* d_comp = (const uint8_t*)d_comp_;
    DevBuf aligned;  // (the kernels load 8 and 4 bytes at a time from multiples of 8 and 4 of the buffer)
    if (const int rc = align_input(d_comp, n, aligned, kGzip, err)) return rc;
    if (chunk_bytes == 0) {
        const char* e = getenv("BSK_GZIP_CHUNK_BYTES");
        if (e && *e) chunk_bytes = (size_t)strtoull(e, nullptr, 10);
    }
    if (chunk_bytes == 0) {
        hipDeviceProp_t prop;
        CODEC_HIP(kGzip, hipGetDeviceProperties(&prop, device));
        const uint64_t waves = 2ull * (uint64_t)std::max(1, prop.multiProcessorCount);  // (69 120 bytes of LDS a wave: two per CU)
        chunk_bytes = std::max<uint64_t>(n / (4 * waves), 256u << 10);
    }
    chunk_bytes = std::max<size_t>(chunk_bytes, 1024);
    gz::Geometry geo = gz::geometry(n, chunk_bytes, nullptr);  // (a power of two, or everything in one chunk)
    chunk_bytes = geo.chunk_bytes;
    const uint64_t nchunks = geo.nchunks;
    if (nchunks > 0x7FFFFFFFull) { err = "libbsk: gzip: " + std::to_string(nchunks) + " chunks of " + std::to_string(chunk_bytes) + " bytes are more than one launch takes; use larger chunks"; return BSK_ERR_UNSUPPORTED; }
    // ---- find and size
    DevBuf d_cand, d_res, d_geo;
    CODEC_HIP(kGzip, d_cand.alloc(8 * nchunks));
    CODEC_HIP(kGzip, d_geo.alloc(sizeof(gz::Geometry)));
    geo.cand = (const uint64_t*)d_cand.p;
    CODEC_HIP(kGzip, hipMemcpy(d_geo.p, &geo, sizeof geo, hipMemcpyHostToDevice));
    CODEC_HIP(kGzip, d_res.alloc(sizeof(ChunkResult) * nchunks));
    CODEC_HIP(kGzip, hipMemset(d_cand.p, 0xFF, 8 * nchunks));
    std::vector<uint64_t> cand(nchunks);
    std::vector<ChunkResult> res(nchunks);
    {
        CodecStage T("gzip_find");
        if (nchunks > 1) {
            hipLaunchKernelGGL(k_gz_find, dim3((unsigned)(nchunks - 1)), dim3(256), 0, nullptr, d_comp, (uint64_t)n, (uint64_t)chunk_bytes, d_cand.as<uint64_t>());
            CODEC_HIP(kGzip, hipGetLastError());
        }
        CODEC_HIP(kGzip, hipMemcpy(cand.data(), d_cand.p, 8 * nchunks, hipMemcpyDeviceToHost));
    }
    {
        CodecStage T("gzip_size");
        hipLaunchKernelGGL(k_gz_size, dim3((unsigned)nchunks), dim3(64), 0, nullptr, d_comp, d_geo.as<gz::Geometry>(), d_res.as<ChunkResult>());
        CODEC_HIP(kGzip, hipGetLastError());
        CODEC_HIP(kGzip, hipMemcpy(res.data(), d_res.p, sizeof(ChunkResult) * nchunks, hipMemcpyDeviceToHost));
    }
    d_res.release();
    // ---- the chain
    std::vector<gz::ChainChunk> chain;
    const int f = gz::walk_chain(cand, res, chunk_bytes, chain, g_plan, err);
    if (f) return fail_code(f);
    const uint64_t total = g_plan.text, nchain = chain.size(), nmem = g_plan.members;
    {
        size_t free_b = 0, all_b = 0;
        CODEC_HIP(kGzip, hipMemGetInfo(&free_b, &all_b));
        const uint64_t need = 3 * total + nchain * gz::WIN + (64u << 20);
        if (need > free_b) {
            err = "libbsk: gzip: the text (" + std::to_string(total) + " bytes), its symbols (" + std::to_string(2 * total) + " bytes) and the input (" +
                  std::to_string(n) + " bytes) do not fit on the device together (" + std::to_string(free_b) + " bytes are free with the input loaded)";
            return BSK_ERR_CAPACITY;
        }
    }
    std::vector<ChainDesc> desc(nchain);
    for (uint64_t i = 0; i < nchain; ++i) desc[i] = ChainDesc{chain[i].k, chain[i].text_off, chain[i].text, chain[i].member0, chain[i].marker_lo, chain[i].members};
    DevBuf d_chain, d_sym, d_mem, d_dres, d_W, d_text_buf, d_ctl;
    CODEC_HIP(kGzip, d_chain.alloc(sizeof(ChainDesc) * nchain));
    CODEC_HIP(kGzip, d_sym.alloc(2 * total + 32));
    CODEC_HIP(kGzip, d_mem.alloc(sizeof(MemberRec) * nmem));
    CODEC_HIP(kGzip, d_dres.alloc(sizeof(ChunkResult) * nchain));
    CODEC_HIP(kGzip, d_W.alloc(nchain * gz::WIN));
    CODEC_HIP(kGzip, d_text_buf.alloc(total));
    CODEC_HIP(kGzip, d_ctl.alloc(8 + 128));
    CODEC_HIP(kGzip, hipMemcpy(d_chain.p, desc.data(), sizeof(ChainDesc) * nchain, hipMemcpyHostToDevice));
    std::vector<ChunkResult> dres(nchain);
    std::vector<MemberRec> mem(nmem);
    {
        CodecStage T("gzip_decode");
        hipLaunchKernelGGL(k_gz_decode, dim3((unsigned)nchain), dim3(64), 0, nullptr, d_comp, d_geo.as<gz::Geometry>(), d_chain.as<ChainDesc>(),
                           d_sym.as<uint16_t>(), d_mem.as<MemberRec>(), d_dres.as<ChunkResult>());
        CODEC_HIP(kGzip, hipGetLastError());
        CODEC_HIP(kGzip, hipMemcpy(dres.data(), d_dres.p, sizeof(ChunkResult) * nchain, hipMemcpyDeviceToHost));
        if (nmem) CODEC_HIP(kGzip, hipMemcpy(mem.data(), d_mem.p, sizeof(MemberRec) * nmem, hipMemcpyDeviceToHost));
    }
    for (uint64_t i = 0; i < nchain; ++i) {
        if (dres[i].err) return fail_code(gz::chunk_failure(dres[i], chain[i].member0, err));
        if (dres[i].members != chain[i].members || dres[i].text != chain[i].text) { err = "libbsk: gzip: the decode of chunk " + std::to_string(chain[i].k) + " does not repeat its size pass"; return BSK_ERR_FORMAT; }
        for (uint32_t m = 0; m < chain[i].members; ++m) mem[chain[i].member0 + m].text_end += chain[i].text_off;  // (from the chunk's start -> of the text)
    }
    // ---- windows, translate, CRC
    unsigned long long* d_status = d_ctl.as<unsigned long long>();
    uint32_t* d_mat = (uint32_t*)(d_status + 1);
    const unsigned long long clean = ~0ull;
    uint32_t mat[32];
    bgzf::crc_advance_matrix(mat, gz::CRC_CHUNK);
    CODEC_HIP(kGzip, hipMemcpy(d_status, &clean, 8, hipMemcpyHostToDevice));
    CODEC_HIP(kGzip, hipMemcpy(d_mat, mat, 128, hipMemcpyHostToDevice));
    CODEC_HIP(kGzip, hipMemset(d_W.p, 0, gz::WIN));
    {
        CodecStage T("gzip_windows");
        if (nchain > 1) {
            hipLaunchKernelGGL(k_gz_windows, dim3(1), dim3(1024), 0, nullptr, d_chain.as<ChainDesc>(), nchain, d_sym.as<uint16_t>(), d_W.as<uint8_t>());
            CODEC_HIP(kGzip, hipGetLastError());
        }
    }
    {
        CodecStage T("gzip_translate");
        if (total) {
            const uint64_t threads = (total + 15) / 16;
            hipLaunchKernelGGL(k_gz_translate, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, nullptr, d_chain.as<ChainDesc>(), nchain,
                               d_sym.as<uint16_t>(), d_W.as<uint8_t>(), d_text_buf.as<uint8_t>(), total, d_status);
            CODEC_HIP(kGzip, hipGetLastError());
        }
    }
    std::vector<gz::Piece> pieces;
    gz::crc_pieces(mem, pieces);
    std::vector<uint32_t> pcrc(pieces.size());
    {
        CodecStage T("gzip_crc");
        DevBuf d_pieces, d_pcrc;
        CODEC_HIP(kGzip, d_pieces.alloc(sizeof(gz::Piece) * pieces.size()));
        CODEC_HIP(kGzip, d_pcrc.alloc(4 * pieces.size()));
        if (!pieces.empty()) {
            CODEC_HIP(kGzip, hipMemcpy(d_pieces.p, pieces.data(), sizeof(gz::Piece) * pieces.size(), hipMemcpyHostToDevice));
            hipLaunchKernelGGL(k_gz_crc, dim3((unsigned)pieces.size()), dim3(64), 0, nullptr, d_text_buf.as<uint8_t>(), d_pieces.as<gz::Piece>(), d_mat,
                               d_pcrc.as<uint32_t>());
            CODEC_HIP(kGzip, hipGetLastError());
            CODEC_HIP(kGzip, hipMemcpy(pcrc.data(), d_pcrc.p, 4 * pieces.size(), hipMemcpyDeviceToHost));
        }
        unsigned long long status = clean;
        CODEC_HIP(kGzip, hipMemcpy(&status, d_status, 8, hipMemcpyDeviceToHost));
        if (status != clean) {
            const gz::ChainChunk& c = chain[(size_t)status];
            err = gz::where(c.member0, cand[c.k] / 8u) + gz::error_text(bgzf::ERR_DISTANCE) + " (in chunk " + std::to_string(c.k) + ")";
            return BSK_ERR_FORMAT;
        }
    }
    const int fm = gz::check_members(mem, pieces, pcrc, err);
    if (fm) return fail_code(fm);
    *d_text = d_text_buf.p;
    d_text_buf.p = nullptr;
    *n_text = (size_t)total;
    return BSK_OK;
}

}  // namespace bsk
