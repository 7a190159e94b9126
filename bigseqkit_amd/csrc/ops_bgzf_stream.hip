// The device's side of the BGZF piece reader (bgzf_stream.hpp holds the rule).
//   compressed   two pinned slots and two device slots, allocated at open.  A reader thread preads chunk k + 1 into its pinned
//                slot and copies it on a stream of its own while the blocks of chunk k are inflated; the bytes of a block that
//                straddles the end of a chunk are put in front of the next chunk, on the host and on the device
//   the chain    is walked on the host in the pinned slot -- the header and the trailer of every block are at hand there, so the
//                block list costs no kernel and no read-back -- and goes to k_bgzf_inflate (ops_bgzf.hip) as a list of blocks
//                whose text offsets begin at the length of the carried head: every block is written into place
//   text         two buffers, allocated at open; the carried head moves to the front of the other one by a device copy.  A
//                buffer is written again only behind an event that follows everything the default stream was given before
//   the cut      k_bgzf_stream_cut: one lane runs stream_cut (bgzf_stream.hpp) and one word comes back.  FASTQ windows that it
//                declines, or in which it finds no start, are judged by find_fastq_cut on a host copy
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sys/stat.h>

#include "bgzf_stream.hpp"
#include "codec_host.hpp"

namespace bsk {
namespace {

__global__ __launch_bounds__(64) void k_bgzf_stream_cut(const uint8_t* __restrict__ buf, uint64_t n, uint64_t from, int format,
                                                        uint64_t* __restrict__ res) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    *res = stream_cut(buf, n, from, format);
}

// the look-behind of find_fastq_cut (fastq_multiline_prev_agrees: 8 MiB) and a margin, so that a copy that begins there is read
// as the whole window is
constexpr uint64_t CUT_BACK = (8ull << 20) + 64;

struct BgzfDeviceBackend : BgzfStreamBackend {
    int device;
    hipStream_t sx = nullptr, sc = nullptr;  // the reader's stream, and the stream of the chunk copies
    hipEvent_t ev_reuse = nullptr;
    uint8_t *h_comp[2] = {nullptr, nullptr}, *d_comp[2] = {nullptr, nullptr}, *d_text[2] = {nullptr, nullptr};
    size_t cap_text[2] = {0, 0};
    BgzfBlockDesc* d_desc = nullptr;
    size_t cap_desc = 0;
    uint8_t* d_small = nullptr;          // 128 bytes of the CRC operator, the status word, the cut
    unsigned long long* h_small = nullptr;  // pinned: [0] the status read back, [1] the cut read back, [2] ~0
    std::thread reader[2];
    size_t got[2] = {0, 0};
    std::string read_err[2];

    explicit BgzfDeviceBackend(int dev) : device(dev) {}
    ~BgzfDeviceBackend() override {
        for (auto& t : reader)
            if (t.joinable()) t.join();
        (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();  // (operators that were handed the last pieces may still read them)
        for (int k = 0; k < 2; ++k) {
            if (h_comp[k]) (void)hipHostFree(h_comp[k]);
            if (d_comp[k]) (void)hipFree(d_comp[k]);
            if (d_text[k]) (void)hipFree(d_text[k]);
        }
        if (d_desc) (void)hipFree(d_desc);
        if (d_small) (void)hipFree(d_small);
        if (h_small) (void)hipHostFree(h_small);
        if (ev_reuse) (void)hipEventDestroy(ev_reuse);
        if (sx) (void)hipStreamDestroy(sx);
        if (sc) (void)hipStreamDestroy(sc);
    }
    uint32_t* d_mat() const { return (uint32_t*)d_small; }
    unsigned long long* d_status() const { return (unsigned long long*)(d_small + 128); }
    uint64_t* d_cut() const { return (uint64_t*)(d_small + 136); }

    int open(size_t chunk_bytes, size_t text_cap_) override {
        if (const int rc = select_device(device, kBgzf, err)) return rc;  // (device -1, the host backend, never comes here)
        CODEC_HIP(kBgzf, hipStreamCreateWithFlags(&sx, hipStreamNonBlocking));
        CODEC_HIP(kBgzf, hipStreamCreateWithFlags(&sc, hipStreamNonBlocking));
        CODEC_HIP(kBgzf, hipEventCreateWithFlags(&ev_reuse, hipEventDisableTiming));
        for (int k = 0; k < 2; ++k) {
            CODEC_HIP(kBgzf, hipHostMalloc((void**)&h_comp[k], FRONT + chunk_bytes, hipHostMallocDefault));
            CODEC_HIP(kBgzf, hipMalloc((void**)&d_comp[k], FRONT + chunk_bytes));
            CODEC_HIP(kBgzf, hipMalloc((void**)&d_text[k], text_cap_));
            cap_text[k] = text_cap_;
        }
        CODEC_HIP(kBgzf, hipMalloc((void**)&d_small, 256));
        CODEC_HIP(kBgzf, hipHostMalloc((void**)&h_small, 64, hipHostMallocDefault));
        h_small[2] = ~0ull;
        uint32_t mat[32];
        bgzf_crc_matrix(mat);
        CODEC_HIP(kBgzf, hipMemcpy(d_small, mat, 128, hipMemcpyHostToDevice));
        return BSK_OK;
    }
    uint8_t* comp_host(int slot) override { return h_comp[slot]; }
    int start_read(int slot, int fd, uint64_t file_off, size_t len) override {
        if (reader[slot].joinable()) reader[slot].join();
        got[slot] = 0;
        read_err[slot].clear();
        reader[slot] = std::thread([this, slot, fd, file_off, len]() {
            size_t at = 0;
            while (at < len) {
                const ssize_t k = pread(fd, h_comp[slot] + FRONT + at, len - at, (off_t)(file_off + at));
                if (k < 0) { read_err[slot] = "libbsk: bgzf: reading the file failed"; return; }
                if (k == 0) break;
                at += (size_t)k;
            }
            got[slot] = at;
            if (at == 0) return;
            if (hipSetDevice(device) != hipSuccess || hipMemcpyAsync(d_comp[slot] + FRONT, h_comp[slot] + FRONT, at, hipMemcpyHostToDevice, sc) != hipSuccess ||
                hipStreamSynchronize(sc) != hipSuccess)
                read_err[slot] = "libbsk: bgzf: copying a chunk to the device failed";
        });
        return BSK_OK;
    }
    int wait_read(int slot, size_t* g) override {
        if (reader[slot].joinable()) reader[slot].join();
        *g = got[slot];
        if (!read_err[slot].empty()) { err = read_err[slot]; return read_err[slot].find("reading") != std::string::npos ? BSK_ERR_INVALID_ARG : BSK_ERR_HIP; }
        return BSK_OK;
    }
    int push_front(int slot, size_t left) override {
        CODEC_HIP(kBgzf, hipMemcpyAsync(d_comp[slot] + FRONT - left, h_comp[slot] + FRONT - left, left, hipMemcpyHostToDevice, sx));
        return BSK_OK;
    }
    int inflate(int slot, size_t slot_bytes, const BgzfBlockDesc* d, size_t nb, int tbuf, uint64_t* bad) override {
        *bad = ~0ull;
        if (nb == 0) return BSK_OK;
        if (nb > cap_desc) {
            CODEC_HIP(kBgzf, hipStreamSynchronize(sx));
            if (d_desc) CODEC_HIP(kBgzf, hipFree(d_desc));
            d_desc = nullptr;
            cap_desc = std::max<size_t>(nb, 2 * cap_desc);
            CODEC_HIP(kBgzf, hipMalloc((void**)&d_desc, cap_desc * sizeof(BgzfBlockDesc)));
        }
        for (size_t i = 0; i < nb; ++i)  // (the list is the host's own; still: nothing is launched that writes outside the buffer)
            if (d[i].coff + d[i].csize > slot_bytes || d[i].ooff + d[i].usize > cap_text[tbuf]) { err = "libbsk: bgzf: a block does not fit the reader's buffers"; return BSK_ERR_INVALID_ARG; }
        CodecStage T("bgzf_inflate", sx);
        CODEC_HIP(kBgzf, hipMemcpyAsync(d_desc, d, nb * sizeof(BgzfBlockDesc), hipMemcpyHostToDevice, sx));
        CODEC_HIP(kBgzf, hipMemcpyAsync(d_status(), &h_small[2], 8, hipMemcpyHostToDevice, sx));
        CODEC_HIP(kBgzf, (hipError_t)bgzf_launch_inflate(d_comp[slot], slot_bytes, d_desc, nb, d_text[tbuf], d_mat(), d_status(), sx));
        CODEC_HIP(kBgzf, hipMemcpyAsync(&h_small[0], d_status(), 8, hipMemcpyDeviceToHost, sx));
        CODEC_HIP(kBgzf, hipStreamSynchronize(sx));
        T.stop();
        *bad = h_small[0];
        return BSK_OK;
    }
    size_t text_cap(int tbuf) const override { return cap_text[tbuf]; }
    int text_grow(int tbuf, size_t cap, size_t keep) override {
        uint8_t* p = nullptr;
        CODEC_HIP(kBgzf, hipMalloc((void**)&p, cap));
        if (keep) {
            const hipError_t e = hipMemcpyAsync(p, d_text[tbuf], std::min(keep, cap_text[tbuf]), hipMemcpyDeviceToDevice, sx);
            if (e != hipSuccess) { (void)hipFree(p); CODEC_HIP(kBgzf, e); }
        }
        CODEC_HIP(kBgzf, hipStreamSynchronize(sx));
        CODEC_HIP(kBgzf, hipFree(d_text[tbuf]));
        d_text[tbuf] = p;
        cap_text[tbuf] = cap;
        return BSK_OK;
    }
    const uint8_t* text(int tbuf) const override { return d_text[tbuf]; }
    int reuse(int) override {
        // (the operators that were handed the buffer's last piece run on the default stream, or on streams that it waits for)
        CODEC_HIP(kBgzf, hipSetDevice(device));
        CODEC_HIP(kBgzf, hipEventRecord(ev_reuse, nullptr));
        CODEC_HIP(kBgzf, hipStreamWaitEvent(sx, ev_reuse, 0));
        return BSK_OK;
    }
    int move(int from, size_t from_off, int to, size_t to_off, size_t n) override {
        if (from_off + n > cap_text[from] || to_off + n > cap_text[to]) { err = "libbsk: bgzf: the carried head does not fit the reader's buffers"; return BSK_ERR_INVALID_ARG; }
        CODEC_HIP(kBgzf, hipMemcpyAsync(d_text[to] + to_off, d_text[from] + from_off, n, hipMemcpyDeviceToDevice, sx));
        return BSK_OK;
    }
    int cut_on_device(const uint8_t* d_buf, uint64_t n, uint64_t from, int format, uint64_t* cut) {
        CodecStage T("bgzf_stream_cut", sx);
        hipLaunchKernelGGL(k_bgzf_stream_cut, dim3(1), dim3(64), 0, sx, d_buf, n, from, format, d_cut());
        CODEC_HIP(kBgzf, hipGetLastError());
        CODEC_HIP(kBgzf, hipMemcpyAsync(&h_small[1], d_cut(), 8, hipMemcpyDeviceToHost, sx));
        CODEC_HIP(kBgzf, hipStreamSynchronize(sx));
        T.stop();
        *cut = h_small[1];
        return BSK_OK;
    }
    int find_cut(int tbuf, uint64_t n, uint64_t from, int format, uint64_t* cut) override {
        if (FRONT + n > cap_text[tbuf]) { err = "libbsk: bgzf: the window does not fit the reader's buffers"; return BSK_ERR_INVALID_ARG; }
        const int rc = cut_on_device(d_text[tbuf] + FRONT, n, from, format, cut);
        if (rc != BSK_OK) return rc;
        if (format != BSK_FORMAT_FASTQ) {
            if (*cut > n) *cut = n;
            return BSK_OK;
        }
        if (*cut < n) return BSK_OK;
        // declined, or no start: the host rule on a copy of the window
        const uint64_t lo = from > CUT_BACK ? from - CUT_BACK : 0;
        std::vector<uint8_t> h((size_t)(n - lo));
        CODEC_HIP(kBgzf, hipMemcpyAsync(h.data(), d_text[tbuf] + FRONT + lo, h.size(), hipMemcpyDeviceToHost, sx));
        CODEC_HIP(kBgzf, hipStreamSynchronize(sx));
        const uint64_t r = find_fastq_cut(h.data(), h.size(), from - lo);
        *cut = r >= h.size() ? n : r + lo;
        return BSK_OK;
    }
    int sync() override {
        CODEC_HIP(kBgzf, hipStreamSynchronize(sx));
        return BSK_OK;
    }
};

}  // namespace

BgzfPieceReader* bgzf_reader_open(int fd, int device, int format, size_t piece, size_t look, size_t chunk, int* rc, std::string& err) {
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) {
        *rc = BSK_ERR_INVALID_ARG;
        err = "libbsk: bgzf: the reader needs a regular file (a pipe goes through bsk_bgzf_inflate_host)";
        return nullptr;
    }
    std::unique_ptr<BgzfStreamBackend> B;
    if (device < 0) B.reset(new BgzfHostBackend(8));
    else B.reset(new BgzfDeviceBackend(device));
    std::unique_ptr<BgzfPieceReader> R(new BgzfPieceReader(std::move(B), fd, (uint64_t)sb.st_size, format, piece, look, chunk));
    *rc = R->open();
    if (*rc != BSK_OK) {
        err = R->error();
        return nullptr;
    }
    return R.release();
}

int bgzf_launch_stream_cut(const uint8_t* d_text, uint64_t n, uint64_t from, int format, uint64_t* d_cut, void* stream) {
    hipLaunchKernelGGL(k_bgzf_stream_cut, dim3(1), dim3(64), 0, (hipStream_t)stream, d_text, n, from, format, d_cut);
    return (int)hipGetLastError();
}

int bgzf_stream_cut_run(const uint8_t* text, uint64_t n, uint64_t from, int format, int device, uint64_t* cut, std::string& err) {
    if (device < 0) {
        *cut = stream_cut(text, n, from, format);
        return BSK_OK;
    }
    BgzfDeviceBackend B(device);
    const int rc = B.open(1, BgzfStreamBackend::FRONT + (size_t)n + 16);
    if (rc != BSK_OK) { err = B.err; return rc; }
    CODEC_HIP(kBgzf, hipMemcpy(B.d_text[0] + BgzfStreamBackend::FRONT, text, (size_t)n, hipMemcpyHostToDevice));
    const int rc2 = B.cut_on_device(B.d_text[0] + BgzfStreamBackend::FRONT, n, from, format, cut);
    if (rc2 != BSK_OK) err = B.err;
    return rc2;
}

}  // namespace bsk
