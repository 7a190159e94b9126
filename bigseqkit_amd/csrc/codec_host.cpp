// What codec_host.hpp needs defined once: the process-wide stage registry, the choice of the device, the aligned copy.
#include "codec_host.hpp"

#include <cstdio>
#include <map>
#include <mutex>

namespace bsk {
namespace {

std::mutex g_prof_mu;
bool g_prof_on = false;
struct Stage { double ms = 0; uint64_t launches = 0; };
std::map<std::string, Stage> g_prof;

}  // namespace

void codec_profile_enable(bool on) { std::lock_guard<std::mutex> g(g_prof_mu); g_prof_on = on; }
bool codec_profile_on() { std::lock_guard<std::mutex> g(g_prof_mu); return g_prof_on; }
void codec_profile_add(const char* stage, double ms) {
    std::lock_guard<std::mutex> g(g_prof_mu);
    g_prof[stage].ms += ms;
    g_prof[stage].launches += 1;
}
void codec_profile_reset() { std::lock_guard<std::mutex> g(g_prof_mu); g_prof.clear(); }
std::string codec_profile_text() {
    std::lock_guard<std::mutex> g(g_prof_mu);
    std::string out;
    for (auto& kv : g_prof) {
        char num[96];
        snprintf(num, sizeof num, "=%.6f/%llu;", kv.second.ms, (unsigned long long)kv.second.launches);
        out += kv.first + num;
    }
    return out;
}

int select_device(int device, const char* prefix, std::string& err) {
    int have = 0;
    if (hipGetDeviceCount(&have) != hipSuccess || have <= 0) { err = "libbsk: no HIP device visible"; return BSK_ERR_NO_DEVICE; }
    if (device < 0 || device >= have) { err = "libbsk: device " + std::to_string(device) + " is not visible"; return BSK_ERR_NO_DEVICE; }
    CODEC_HIP(prefix, hipSetDevice(device));
    return BSK_OK;
}

int align_input(const uint8_t*& d_comp, size_t n, DevBuf& aligned, const char* prefix, std::string& err) {
    if (!((uintptr_t)d_comp & 15u)) return BSK_OK;
    CODEC_HIP(prefix, aligned.alloc(n));
    CODEC_HIP(prefix, hipMemcpy(aligned.p, d_comp, n, hipMemcpyDeviceToDevice));
    d_comp = aligned.as<uint8_t>();
    return BSK_OK;
}

}  // namespace bsk
