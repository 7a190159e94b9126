// The host side that the codec sources share (ops_bgzf.hip, ops_bgzf_write.hip, ops_gzip.hip, ops_bgzf_stream.hip): a device
// buffer, the stages of bsk_profile_dump and their timer, the HIP-status macro, the choice of the device, the aligned copy of
// an input and the pool of host workers.  Nothing here is device code; codec_host.cpp holds what needs one definition.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <string>
#include <thread>
#include <vector>

#include "../../include/bsk.h"

namespace bsk {

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; }
    hipError_t alloc(size_t n) { return hipMalloc(&p, n ? n : 1); }
    template <class T> T* as() const { return (T*)p; }
};

// the stages of the codec calls for bsk_profile_dump (process-wide: these calls have no context)
void codec_profile_enable(bool on);
bool codec_profile_on();
void codec_profile_add(const char* stage, double ms);
void codec_profile_reset();
std::string codec_profile_text();  // "name=ms/launches;" per stage that ran

// One stage, timed on `stream` from here to stop() or to the end of the scope.  With profiling off it creates no event and
// takes the registry's lock once.
struct CodecStage {
    const char* name;
    hipStream_t st;
    hipEvent_t a = nullptr, b = nullptr;
    explicit CodecStage(const char* nm, hipStream_t s = nullptr) : name(nm), st(s) {
        if (!codec_profile_on()) return;
        if (hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess && hipEventRecord(a, st) == hipSuccess) return;
        drop();
    }
    void drop() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
        a = b = nullptr;
    }
    void stop() {
        if (!a) return;
        float ms = 0;
        if (hipEventRecord(b, st) != hipSuccess || hipEventSynchronize(b) != hipSuccess || hipEventElapsedTime(&ms, a, b) != hipSuccess) ms = 0;
        drop();
        codec_profile_add(name, ms);
    }
    ~CodecStage() { stop(); }
};

constexpr char kBgzf[] = "libbsk: bgzf: ", kGzip[] = "libbsk: gzip: ";
// in a function that has `std::string err` in reach and returns a BSK_* code; prefix: kBgzf or kGzip
#define CODEC_HIP(prefix, x)                                                                                      \
    do {                                                                                                          \
        const hipError_t e_ = (x);                                                                                \
        if (e_ != hipSuccess) { err = std::string(prefix) + hipGetErrorString(e_) + " (" #x ")"; return BSK_ERR_HIP; } \
    } while (0)

// is a device visible, is this one, hipSetDevice
int select_device(int device, const char* prefix, std::string& err);
// The kernels load up to 16 bytes at a time from multiples of 16 of the buffer: an input that is not aligned so is copied into
// `aligned`, and d_comp points there
int align_input(const uint8_t*& d_comp, size_t n, DevBuf& aligned, const char* prefix, std::string& err);

// `threads` (<= 0: 8, at most 64, at most one per item) workers, one of them the caller.  work(next) sets up what a worker
// owns, then takes the items i = next() while i < items
template <class Work>
void run_workers(int threads, uint64_t items, Work work) {
    std::atomic<uint64_t> counter{0};
    auto next = [&counter]() { return counter.fetch_add(1); };
    const int T = (int)std::min<uint64_t>((uint64_t)std::max(1, std::min(threads > 0 ? threads : 8, 64)), std::max<uint64_t>(items, 1));
    std::vector<std::thread> pool;
    for (int t = 1; t < T; ++t) pool.emplace_back([&]() { work(next); });
    work(next);
    for (auto& t : pool) t.join();
}

}  // namespace bsk
