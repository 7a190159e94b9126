// The device's side of the gzip piece reader (gzip_stream.hpp holds the rule).
//   compressed   two pinned slots and two device slots.  A reader thread preads segment k + 1 into its pinned slot and copies it
//                on a stream of its own while segment k is decoded; a slot begins at a multiple of 4096 of the file, so the
//                kernels' aligned loads hold
//   a segment    find, size, decode, windows, translate and crc of ops_gzip.hip through its launchers, on the reader's stream.  A
//                segment that is re-entered sizes and decodes its chunks with k_gzs_size / k_gzs_decode: the same walk, chunk 0
//                from the resume bit (gz::Walker<.., RESUME>).  W[0] is the carried window, copied from the host
//   text         the segment's text lands in a staging buffer -- the translate kernel stores 16 bytes at multiples of 16 -- and
//                the part of it that is wanted is copied behind the text at hand, device to device.  The last 32 KiB go to the
//                host with the status word: they are the next window
//   the cut      k_bgzf_stream_cut through its launcher (ops_bgzf_stream.hip): one lane runs stream_cut and one word comes
//                back.  FASTQ windows that it declines, or in which it finds no start, are judged by find_fastq_cut on a host copy
// Synchronisations per segment: four -- the candidates, the sizes, the decode's results, the status word with the CRCs and the
// tail -- and one per piece for the cut.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sys/stat.h>

#include <thread>

#include "codec_host.hpp"
#include "gzip_stream.hpp"
#include "gzip_wave_dev.hpp"
#include "ops_gzip.hpp"

namespace bsk {
namespace {

using gz::ChunkResult;
using gz::GzWaveLane;
using gz::MemberRec;

// k_gz_size and k_gz_decode of ops_gzip.hip for a segment that is re-entered: chunk 0 has a start like every other chunk
__global__ __launch_bounds__(64) void k_gzs_size(const uint8_t* __restrict__ comp, const gz::Geometry* __restrict__ G, ChunkResult* __restrict__ res) {
    __shared__ gz::GzTables T;
    const uint64_t k = blockIdx.x;
    if (G->cand[k] == gz::NONE) {  // (the same in every lane)
        if (threadIdx.x == 0) res[k] = ChunkResult{gz::NONE, 0, gz::NONE, 0, 0, 0};
        return;
    }
    if (threadIdx.x == 0) T.park = gz::Parked{*G, k, 0, gz::NONE, nullptr, nullptr, 0};
    __syncthreads();
    GzWaveLane io{comp, G->n, make_uint2(0u, 0u), ~0u};
    gz::Walker<GzWaveLane, false, true> W(io, T, nullptr);
    const ChunkResult R = W.run(0);
    if (threadIdx.x == 0) res[blockIdx.x] = R;
}

__global__ __launch_bounds__(64) void k_gzs_decode(const uint8_t* __restrict__ comp, const gz::Geometry* __restrict__ G,
                                                   const ChainDesc* __restrict__ chain, uint16_t* __restrict__ sym, MemberRec* __restrict__ mem,
                                                   ChunkResult* __restrict__ res) {
    __shared__ gz::GzDecodeLds S;
    const ChainDesc d = chain[blockIdx.x];
    if (threadIdx.x == 0) S.T.park = gz::Parked{*G, d.k, d.text, gz::NONE, mem + d.member0, sym + d.text_off, d.members};
    __syncthreads();
    GzWaveLane io{comp, G->n, make_uint2(0u, 0u), ~0u};
    gz::Walker<GzWaveLane, true, true> W(io, S.T, S.ring);
    const ChunkResult R = W.run((uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)d.text_off & 7u)));
    if (threadIdx.x == 0) res[blockIdx.x] = R;
}

constexpr uint64_t CUT_BACK = (8ull << 20) + 64;  // (the look-behind of find_fastq_cut and a margin, as in ops_bgzf_stream.hip)

struct GzipDeviceBackend : GzipStreamBackend {
    int device;
    hipStream_t sx = nullptr, sc = nullptr;  // the reader's stream, and the stream of the segment copies
    hipEvent_t ev_reuse = nullptr;
    uint8_t *h_comp[2] = {nullptr, nullptr}, *d_comp[2] = {nullptr, nullptr}, *d_text[2] = {nullptr, nullptr};
    size_t cap_comp = 0, cap_text[2] = {0, 0};
    // a buffer of the segment at hand: it grows to what a segment needs and is kept
    struct Grow { void* p = nullptr; size_t cap = 0; };
    Grow d_cand, d_res, d_geo, d_chain, d_sym, d_mem, d_dres, d_W, d_stage, d_pieces, d_pcrc;
    uint8_t* d_small = nullptr;             // 128 bytes of the CRC operator, the status word, the cut
    unsigned long long* h_small = nullptr;  // pinned: [0] the status read back, [1] the cut read back, [2] ~0
    std::thread reader[2];
    size_t got[2] = {0, 0};
    std::string read_err[2];
    int cus = 1;
    // the segment at hand
    int slot = 0;
    uint64_t n = 0, nchunks = 0;
    bool resumed = false;

    explicit GzipDeviceBackend(int dev) : device(dev) {}
    ~GzipDeviceBackend() override {
        for (auto& t : reader)
            if (t.joinable()) t.join();
        (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();  // (operators that were handed the last pieces may still read them)
        for (int k = 0; k < 2; ++k) {
            if (h_comp[k]) (void)hipHostFree(h_comp[k]);
            if (d_comp[k]) (void)hipFree(d_comp[k]);
            if (d_text[k]) (void)hipFree(d_text[k]);
        }
        for (Grow* g : {&d_cand, &d_res, &d_geo, &d_chain, &d_sym, &d_mem, &d_dres, &d_W, &d_stage, &d_pieces, &d_pcrc})
            if (g->p) (void)hipFree(g->p);
        if (d_small) (void)hipFree(d_small);
        if (h_small) (void)hipHostFree(h_small);
        if (ev_reuse) (void)hipEventDestroy(ev_reuse);
        if (sx) (void)hipStreamDestroy(sx);
        if (sc) (void)hipStreamDestroy(sc);
    }
    uint32_t* d_mat() const { return (uint32_t*)d_small; }
    unsigned long long* d_status() const { return (unsigned long long*)(d_small + 128); }
    uint64_t* d_cut() const { return (uint64_t*)(d_small + 136); }

    // at least `bytes`; what the buffer held is not kept
    int need(Grow& g, size_t bytes) {
        if (bytes <= g.cap && g.p) return BSK_OK;
        CODEC_HIP(kGzip, hipStreamSynchronize(sx));
        if (g.p) CODEC_HIP(kGzip, hipFree(g.p));
        holds(-(int64_t)g.cap);
        g.p = nullptr;
        g.cap = 0;
        const size_t cap = std::max<size_t>(bytes, 256);
        CODEC_HIP(kGzip, hipMalloc(&g.p, cap));
        g.cap = cap;
        holds((int64_t)cap);
        return BSK_OK;
    }
    int alloc_comp(size_t cap) {
        for (int k = 0; k < 2; ++k) {
            if (reader[k].joinable()) reader[k].join();
            if (h_comp[k]) CODEC_HIP(kGzip, hipHostFree(h_comp[k]));
            h_comp[k] = nullptr;
            if (d_comp[k]) CODEC_HIP(kGzip, hipFree(d_comp[k]));
            d_comp[k] = nullptr;
        }
        holds(-(int64_t)(2 * cap_comp));
        cap_comp = 0;
        for (int k = 0; k < 2; ++k) {
            CODEC_HIP(kGzip, hipHostMalloc((void**)&h_comp[k], cap, hipHostMallocDefault));
            CODEC_HIP(kGzip, hipMalloc((void**)&d_comp[k], cap));
        }
        cap_comp = cap;
        holds((int64_t)(2 * cap));
        return BSK_OK;
    }

    uint64_t chunk_of(uint64_t chunk_bytes, uint64_t n_) const {  // (0: the rule of gzip_inflate_device)
        return std::max<uint64_t>(chunk_bytes ? chunk_bytes : std::max<uint64_t>(n_ / (4 * 2ull * (uint64_t)cus), 256u << 10), 1024);
    }
    int open(size_t comp_cap, size_t text_cap_, size_t seg_text, size_t chunk_bytes) override {
        if (const int rc = select_device(device, kGzip, err)) return rc;  // (device -1, the host backend, never comes here)
        hipDeviceProp_t prop;
        CODEC_HIP(kGzip, hipGetDeviceProperties(&prop, device));
        cus = std::max(1, prop.multiProcessorCount);
        CODEC_HIP(kGzip, hipStreamCreateWithFlags(&sx, hipStreamNonBlocking));
        CODEC_HIP(kGzip, hipStreamCreateWithFlags(&sc, hipStreamNonBlocking));
        CODEC_HIP(kGzip, hipEventCreateWithFlags(&ev_reuse, hipEventDisableTiming));
        if (const int rc = alloc_comp(std::max<size_t>(comp_cap, 4096))) return rc;
        for (int k = 0; k < 2; ++k) {
            CODEC_HIP(kGzip, hipMalloc((void**)&d_text[k], text_cap_));
            cap_text[k] = text_cap_;
            holds((int64_t)text_cap_);
        }
        CODEC_HIP(kGzip, hipMalloc((void**)&d_small, 256));
        CODEC_HIP(kGzip, hipHostMalloc((void**)&h_small, 64, hipHostMallocDefault));
        h_small[2] = ~0ull;
        uint32_t mat[32];
        bgzf::crc_advance_matrix(mat, gz::CRC_CHUNK);
        CODEC_HIP(kGzip, hipMemcpy(d_small, mat, 128, hipMemcpyHostToDevice));
        const uint64_t most_chunks = gz::geometry(comp_cap, chunk_of(chunk_bytes, comp_cap), nullptr).nchunks;
        for (const auto& want : {std::make_pair(&d_geo, sizeof(gz::Geometry)), std::make_pair(&d_cand, (size_t)(8 * most_chunks)),
                                 std::make_pair(&d_res, (size_t)(sizeof(ChunkResult) * most_chunks)), std::make_pair(&d_chain, (size_t)(sizeof(ChainDesc) * most_chunks)),
                                 std::make_pair(&d_dres, (size_t)(sizeof(ChunkResult) * most_chunks)), std::make_pair(&d_W, (size_t)(most_chunks * gz::WIN)),
                                 std::make_pair(&d_sym, 2 * seg_text + 32), std::make_pair(&d_stage, seg_text + 16)})
            if (const int rc = need(*want.first, want.second)) return rc;
        return BSK_OK;
    }
    int comp_grow(size_t cap) override {
        if (cap <= cap_comp) return BSK_OK;
        CODEC_HIP(kGzip, hipStreamSynchronize(sx));
        return alloc_comp(cap);
    }
    int start_read(int s, int fd, uint64_t file_off, size_t len) override {
        if (reader[s].joinable()) reader[s].join();
        got[s] = 0;
        read_err[s].clear();
        if (len > cap_comp) { err = "libbsk: gzip: a segment does not fit the reader's buffers"; return BSK_ERR_INVALID_ARG; }
        reader[s] = std::thread([this, s, fd, file_off, len]() {
            size_t at = 0;
            while (at < len) {
                const ssize_t k = pread(fd, h_comp[s] + at, len - at, (off_t)(file_off + at));
                if (k < 0) { read_err[s] = "libbsk: gzip: reading the file failed"; return; }
                if (k == 0) break;
                at += (size_t)k;
            }
            got[s] = at;
            if (at == 0) return;
            if (hipSetDevice(device) != hipSuccess || hipMemcpyAsync(d_comp[s], h_comp[s], at, hipMemcpyHostToDevice, sc) != hipSuccess ||
                hipStreamSynchronize(sc) != hipSuccess)
                read_err[s] = "libbsk: gzip: copying a segment to the device failed";
        });
        return BSK_OK;
    }
    int wait_read(int s, size_t* g) override {
        if (reader[s].joinable()) reader[s].join();
        *g = got[s];
        if (!read_err[s].empty()) { err = read_err[s]; return read_err[s].find("reading") != std::string::npos ? BSK_ERR_INVALID_ARG : BSK_ERR_HIP; }
        return BSK_OK;
    }

    int size(int slot_, uint64_t n_, uint64_t chunk_bytes, uint64_t rel_bit, std::vector<uint64_t>& cand, std::vector<ChunkResult>& res, uint64_t* chunk_used) override {
        slot = slot_;
        n = n_;
        resumed = rel_bit != gz::NONE;
        if (n > cap_comp) { err = "libbsk: gzip: a segment does not fit the reader's buffers"; return BSK_ERR_INVALID_ARG; }
        gz::Geometry geo = gz::geometry(n, chunk_of(chunk_bytes, n), nullptr);
        *chunk_used = geo.chunk_bytes;
        nchunks = geo.nchunks;
        if (nchunks > 0x7FFFFFFFull) { err = "libbsk: gzip: " + std::to_string(nchunks) + " chunks of " + std::to_string(geo.chunk_bytes) + " bytes are more than one launch takes; use larger chunks"; return BSK_ERR_UNSUPPORTED; }
        if (int rc = need(d_cand, 8 * nchunks)) return rc;
        if (int rc = need(d_res, sizeof(ChunkResult) * nchunks)) return rc;
        cand.assign(nchunks, gz::NONE);
        res.assign(nchunks, ChunkResult{gz::NONE, 0, gz::NONE, 0, 0, 0});
        geo.cand = (const uint64_t*)d_cand.p;
        CODEC_HIP(kGzip, hipMemsetAsync(d_cand.p, 0xFF, 8 * nchunks, sx));
        CODEC_HIP(kGzip, hipMemcpyAsync(d_geo.p, &geo, sizeof geo, hipMemcpyHostToDevice, sx));
        {
            CodecStage T("gzip_find", sx);
            CODEC_HIP(kGzip, (hipError_t)gzip_launch_find(d_comp[slot], n, geo.chunk_bytes, nchunks, (uint64_t*)d_cand.p, sx));
            CODEC_HIP(kGzip, hipMemcpyAsync(cand.data(), d_cand.p, 8 * nchunks, hipMemcpyDeviceToHost, sx));
            CODEC_HIP(kGzip, hipStreamSynchronize(sx));
        }
        if (resumed) {  // chunk 0 starts at the resume bit: nothing at or in front of it is a start of a later chunk
            uint64_t fix = 1;
            cand[0] = rel_bit;
            for (uint64_t k = 1; k < nchunks && k * geo.chunk_bytes * 8u <= rel_bit; ++k) {
                if (cand[k] <= rel_bit) cand[k] = gz::NONE;
                fix = k + 1;
            }
            CODEC_HIP(kGzip, hipMemcpyAsync(d_cand.p, cand.data(), 8 * fix, hipMemcpyHostToDevice, sx));
        }
        {
            CodecStage T("gzip_size", sx);
            if (resumed) {
                hipLaunchKernelGGL(k_gzs_size, dim3((unsigned)nchunks), dim3(64), 0, sx, d_comp[slot], (const gz::Geometry*)d_geo.p, (ChunkResult*)d_res.p);
                CODEC_HIP(kGzip, hipGetLastError());
            } else {
                CODEC_HIP(kGzip, (hipError_t)gzip_launch_size(d_comp[slot], (const gz::Geometry*)d_geo.p, nchunks, (ChunkResult*)d_res.p, sx));
            }
            CODEC_HIP(kGzip, hipMemcpyAsync(res.data(), d_res.p, sizeof(ChunkResult) * nchunks, hipMemcpyDeviceToHost, sx));
            CODEC_HIP(kGzip, hipStreamSynchronize(sx));
        }
        return BSK_OK;
    }

    int decode(const std::vector<gz::ChainChunk>& chain, uint64_t member0, uint64_t total, const uint8_t* window, std::vector<MemberRec>& mem,
               std::vector<ChunkResult>& dres) override {
        const uint64_t nchain = chain.size(), nmem = mem.size() - 1;
        std::vector<ChainDesc> desc(nchain);
        uint64_t text = 0;
        for (uint64_t i = 0; i < nchain; ++i) {
            const gz::ChainChunk& c = chain[i];
            // (the list is the host's own; still: nothing is launched that writes outside the buffers)
            if (c.k >= nchunks || c.text_off != text || c.member0 < member0 || c.member0 - member0 + c.members > nmem) { err = "libbsk: gzip: a chain chunk does not fit the reader's buffers"; return BSK_ERR_INVALID_ARG; }
            text += c.text;
            desc[i] = ChainDesc{c.k, c.text_off, c.text, c.member0 - member0, c.marker_lo, c.members};
        }
        if (text != total) { err = "libbsk: gzip: the chain does not add up to the segment's text"; return BSK_ERR_INVALID_ARG; }
        if (int rc = need(d_chain, sizeof(ChainDesc) * nchain)) return rc;
        if (int rc = need(d_sym, 2 * total + 32)) return rc;
        if (int rc = need(d_mem, sizeof(MemberRec) * nmem)) return rc;
        if (int rc = need(d_dres, sizeof(ChunkResult) * nchain)) return rc;
        if (int rc = need(d_W, nchain * (size_t)gz::WIN)) return rc;
        dres.assign(nchain, ChunkResult{gz::NONE, 0, gz::NONE, 0, 0, 0});
        CODEC_HIP(kGzip, hipMemcpyAsync(d_chain.p, desc.data(), sizeof(ChainDesc) * nchain, hipMemcpyHostToDevice, sx));
        CODEC_HIP(kGzip, hipMemcpyAsync(d_W.p, window, gz::WIN, hipMemcpyHostToDevice, sx));
        CodecStage T("gzip_decode", sx);
        if (resumed) {
            if (nchain) hipLaunchKernelGGL(k_gzs_decode, dim3((unsigned)nchain), dim3(64), 0, sx, d_comp[slot], (const gz::Geometry*)d_geo.p, (const ChainDesc*)d_chain.p,
                                           (uint16_t*)d_sym.p, (MemberRec*)d_mem.p, (ChunkResult*)d_dres.p);
            CODEC_HIP(kGzip, hipGetLastError());
        } else {
            CODEC_HIP(kGzip, (hipError_t)gzip_launch_decode(d_comp[slot], (const gz::Geometry*)d_geo.p, (const ChainDesc*)d_chain.p, nchain, (uint16_t*)d_sym.p,
                                                            (MemberRec*)d_mem.p, (ChunkResult*)d_dres.p, sx));
        }
        CODEC_HIP(kGzip, hipMemcpyAsync(dres.data(), d_dres.p, sizeof(ChunkResult) * nchain, hipMemcpyDeviceToHost, sx));
        if (nmem) CODEC_HIP(kGzip, hipMemcpyAsync(mem.data(), d_mem.p, sizeof(MemberRec) * nmem, hipMemcpyDeviceToHost, sx));
        CODEC_HIP(kGzip, hipStreamSynchronize(sx));
        return BSK_OK;
    }

    int finish(const std::vector<gz::ChainChunk>& chain, uint64_t total, const std::vector<gz::Piece>* pieces, std::vector<uint32_t>& pcrc, uint64_t* bad,
               uint32_t tail, uint8_t* tail_dst) override {
        const uint64_t nchain = chain.size();
        if (int rc = need(d_stage, total + 16)) return rc;
        CODEC_HIP(kGzip, hipMemcpyAsync(d_status(), &h_small[2], 8, hipMemcpyHostToDevice, sx));
        {
            CodecStage T("gzip_windows", sx);
            CODEC_HIP(kGzip, (hipError_t)gzip_launch_windows((const ChainDesc*)d_chain.p, nchain, (const uint16_t*)d_sym.p, (uint8_t*)d_W.p, sx));
        }
        {
            CodecStage T("gzip_translate", sx);
            CODEC_HIP(kGzip, (hipError_t)gzip_launch_translate((const ChainDesc*)d_chain.p, nchain, (const uint16_t*)d_sym.p, (const uint8_t*)d_W.p, (uint8_t*)d_stage.p,
                                                               total, d_status(), sx));
        }
        if (pieces) {
            for (const gz::Piece& p : *pieces)
                if (p.off + p.len > total) { err = "libbsk: gzip: a CRC piece does not fit the segment's text"; return BSK_ERR_INVALID_ARG; }
            pcrc.assign(pieces->size(), 0);
            if (!pieces->empty()) {
                if (int rc = need(d_pieces, sizeof(gz::Piece) * pieces->size())) return rc;
                if (int rc = need(d_pcrc, 4 * pieces->size())) return rc;
                CodecStage T("gzip_crc", sx);
                CODEC_HIP(kGzip, hipMemcpyAsync(d_pieces.p, pieces->data(), sizeof(gz::Piece) * pieces->size(), hipMemcpyHostToDevice, sx));
                CODEC_HIP(kGzip, (hipError_t)gzip_launch_crc((const uint8_t*)d_stage.p, (const gz::Piece*)d_pieces.p, pieces->size(), d_mat(), (uint32_t*)d_pcrc.p, sx));
                CODEC_HIP(kGzip, hipMemcpyAsync(pcrc.data(), d_pcrc.p, 4 * pieces->size(), hipMemcpyDeviceToHost, sx));
            }
        }
        CODEC_HIP(kGzip, hipMemcpyAsync(&h_small[0], d_status(), 8, hipMemcpyDeviceToHost, sx));
        if (tail) CODEC_HIP(kGzip, hipMemcpyAsync(tail_dst, (const uint8_t*)d_stage.p + (total - tail), tail, hipMemcpyDeviceToHost, sx));
        CODEC_HIP(kGzip, hipStreamSynchronize(sx));
        *bad = h_small[0];
        return BSK_OK;
    }

    int take(uint64_t from, int tbuf, size_t off, size_t k) override {
        if (from + k + 16 > d_stage.cap || off + k > cap_text[tbuf]) { err = "libbsk: gzip: a segment's text does not fit the reader's buffers"; return BSK_ERR_INVALID_ARG; }
        CODEC_HIP(kGzip, hipMemcpyAsync(d_text[tbuf] + off, (const uint8_t*)d_stage.p + from, k, hipMemcpyDeviceToDevice, sx));
        return BSK_OK;
    }
    size_t text_cap(int tbuf) const override { return cap_text[tbuf]; }
    int text_grow(int tbuf, size_t cap, size_t keep) override {
        uint8_t* p = nullptr;
        CODEC_HIP(kGzip, hipMalloc((void**)&p, cap));
        if (keep) {
            const hipError_t e = hipMemcpyAsync(p, d_text[tbuf], std::min(keep, cap_text[tbuf]), hipMemcpyDeviceToDevice, sx);
            if (e != hipSuccess) { (void)hipFree(p); CODEC_HIP(kGzip, e); }
        }
        CODEC_HIP(kGzip, hipStreamSynchronize(sx));
        CODEC_HIP(kGzip, hipFree(d_text[tbuf]));
        holds((int64_t)cap - (int64_t)cap_text[tbuf]);
        d_text[tbuf] = p;
        cap_text[tbuf] = cap;
        return BSK_OK;
    }
    const uint8_t* text(int tbuf) const override { return d_text[tbuf]; }
    int reuse(int) override {
        // (the operators that were handed the buffer's last piece run on the default stream, or on streams that it waits for)
        CODEC_HIP(kGzip, hipSetDevice(device));
        CODEC_HIP(kGzip, hipEventRecord(ev_reuse, nullptr));
        CODEC_HIP(kGzip, hipStreamWaitEvent(sx, ev_reuse, 0));
        return BSK_OK;
    }
    int move(int from, size_t from_off, int to, size_t to_off, size_t k) override {
        if (from_off + k > cap_text[from] || to_off + k > cap_text[to]) { err = "libbsk: gzip: the carried head does not fit the reader's buffers"; return BSK_ERR_INVALID_ARG; }
        CODEC_HIP(kGzip, hipMemcpyAsync(d_text[to] + to_off, d_text[from] + from_off, k, hipMemcpyDeviceToDevice, sx));
        return BSK_OK;
    }
    int find_cut(int tbuf, uint64_t k, uint64_t from, int format, uint64_t* cut) override {
        if (k > cap_text[tbuf]) { err = "libbsk: gzip: the window does not fit the reader's buffers"; return BSK_ERR_INVALID_ARG; }
        {
            CodecStage T("gzip_stream_cut", sx);
            CODEC_HIP(kGzip, (hipError_t)bgzf_launch_stream_cut(d_text[tbuf], k, from, format, d_cut(), sx));
            CODEC_HIP(kGzip, hipMemcpyAsync(&h_small[1], d_cut(), 8, hipMemcpyDeviceToHost, sx));
            CODEC_HIP(kGzip, hipStreamSynchronize(sx));
        }
        *cut = h_small[1];
        if (format != BSK_FORMAT_FASTQ) {
            if (*cut > k) *cut = k;
            return BSK_OK;
        }
        if (*cut < k) return BSK_OK;
        // declined, or no start: the host rule on a copy of the window
        const uint64_t lo = from > CUT_BACK ? from - CUT_BACK : 0;
        std::vector<uint8_t> h((size_t)(k - lo));
        CODEC_HIP(kGzip, hipMemcpyAsync(h.data(), d_text[tbuf] + lo, h.size(), hipMemcpyDeviceToHost, sx));
        CODEC_HIP(kGzip, hipStreamSynchronize(sx));
        const uint64_t r = find_fastq_cut(h.data(), h.size(), from - lo);
        *cut = r >= h.size() ? k : r + lo;
        return BSK_OK;
    }
    int sync() override {
        CODEC_HIP(kGzip, hipStreamSynchronize(sx));
        return BSK_OK;
    }
};

}  // namespace

GzipPieceReader* gzip_reader_open(int fd, int device, int format, size_t piece, size_t look, size_t segment, size_t chunk, int* rc, std::string& err) {
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) {
        *rc = BSK_ERR_INVALID_ARG;
        err = "libbsk: gzip: the reader needs a regular file (a pipe goes through bsk_gzip_inflate_host)";
        return nullptr;
    }
    std::unique_ptr<GzipStreamBackend> B;
    if (device < 0) B.reset(new GzipHostBackend());
    else B.reset(new GzipDeviceBackend(device));
    std::unique_ptr<GzipPieceReader> R(new GzipPieceReader(std::move(B), fd, (uint64_t)sb.st_size, format, piece, look, segment, chunk));
    *rc = R->open();
    if (*rc != BSK_OK) {
        err = R->error();
        return nullptr;
    }
    return R.release();
}

}  // namespace bsk
