// ops_replace.hip -- Replace.Call (/root/reference/bigseqkit-lib/replace.go:108-179), see ops_replace.hpp.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ops_replace.hpp"
#include "pattern_match_dev.hpp"  // fnv1a64, text_of

namespace bsk {

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;

struct GroupNames {  // Regexp.SubexpNames lookup for ${name}
    const uint8_t* names;
    const uint32_t* off;
    uint32_t ngroups;
    __device__ int operator()(const uint8_t* s, uint32_t n) const {
        for (uint32_t g = 1; g <= ngroups; ++g) {
            const uint32_t a = off[g], b = off[g + 1];
            if (b - a != n) continue;
            bool same = true;
            for (uint32_t k = 0; k < n && same; ++k) same = names[a + k] == s[k];
            if (same) return (int)g;
        }
        return -1;
    }
};
struct NoNames {
    __device__ int operator()(const uint8_t*, uint32_t) const { return -1; }
};

__device__ __forceinline__ bool is_sym(const uint8_t* p, uint32_t i, uint32_t n, uint8_t lo, uint8_t hi) {
    // {nr} / {NR} (lo, hi = 'n', 'r') or {kv} / {KV}: reNR / reKV of replace.go:181-182
    if (i + 4 > n || p[i] != '{' || p[i + 3] != '}') return false;
    return (p[i + 1] == lo && p[i + 2] == hi) || (p[i + 1] == lo - 32 && p[i + 2] == hi - 32);
}

// the record's template: {nr} -> fmt.Sprintf("%0*d", NrWidth, nr), then every {kv} -> Expand(value) against reKV's
// match (group 1 = "kv" / "KV").  Digits never form or break a {kv}, so one pass over -r gives both substitutions.
// Returns the length, or NONE when it does not fit.
__device__ uint32_t build_template(const ReplParams& R, uint64_t nr, const uint8_t* val, uint32_t vl, uint8_t* rb) {
    uint32_t n = 0;
    bool over = false;
    auto put = [&](uint8_t ch) { if (n < REPL_TMPL_MAX) rb[n++] = ch; else over = true; };
    char dig[24];
    int nd = 0;
    for (uint64_t v = nr;; v /= 10u) { dig[nd++] = (char)('0' + v % 10u); if (v < 10u) break; }
    const uint8_t* p = R.tmpl;
    for (uint32_t i = 0; i < R.tmpl_len;) {
        if (is_sym(p, i, R.tmpl_len, 'n', 'r')) {
            const int w = R.nr_width < 0 ? -R.nr_width : R.nr_width;
            if (R.nr_width > 0) for (int k = nd; k < w; ++k) put('0');
            for (int k = nd - 1; k >= 0; --k) put((uint8_t)dig[k]);
            if (R.nr_width < 0) for (int k = nd; k < w; ++k) put(' ');  // %0*d with a negative width: left-justified
            i += 4;
            continue;
        }
        if (R.kv && val && is_sym(p, i, R.tmpl_len, 'k', 'v')) {
            const uint32_t caps[4] = {i, i + 4u, i + 1u, i + 3u};
            vm_expand(val, vl, [p](uint32_t k) { return p[k]; }, caps, 4u, 1u, NoNames(), put);
            i += 4;
            continue;
        }
        put(p[i++]);
    }
    return over ? NONE : n;
}

__device__ __forceinline__ void flag(const ReplParams& R, int kind, uint64_t i) { atomicMin(&R.err[kind], (unsigned long long)i); }

template <int NCAP, bool WRITE>
__global__ __launch_bounds__(64) void k_repl_heads(const uint8_t* __restrict__ buf, RecordTable t, ReplParams R,
                                                   uint32_t* __restrict__ rep_len, const uint64_t* __restrict__ rep_off,
                                                   uint8_t* __restrict__ stage) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.n) return;
    if (WRITE && rep_len[i] == 0) return;
    const uint32_t lh = t.l_head[i];
    const uint8_t* h = buf + t.start[i] + 1;
    const uint32_t hl = lh > 0 ? lh - 1 : 0;
    if (!WRITE) {
        for (uint32_t k = 0; k < hl; ++k)
            if (h[k] >= 0x80) { flag(R, REPL_ERR_NONASCII, i); rep_len[i] = 0; return; }
    }
    auto text = [h](uint32_t k) { return h[k]; };
    const VmProgram& P = *R.prog;
    const uint8_t* val = nullptr;
    uint32_t vl = 0;
    if (R.kv) {
        uint32_t caps[NCAP];
        const uint32_t found = vm_find_two<NCAP>(P, text, hl, caps);
        if (found > 1) { flag(R, REPL_ERR_MULTI, i); rep_len[i] = 0; return; }
        if (found == 0) { rep_len[i] = 0; return; }
        if (R.capt_over) { flag(R, REPL_ERR_CAPT, i); rep_len[i] = 0; return; }
        const uint32_t a = caps[2 * R.capt_idx], b = caps[2 * R.capt_idx + 1];
        const uint8_t* key = h + (a == NONE ? 0u : a);
        const uint32_t kl = (a == NONE || b == NONE) ? 0u : b - a;
        const uint64_t hk = fnv1a64(key, kl, R.icase != 0);
        int64_t e = -1;
        for (uint64_t s = hk & R.kv_mask;; s = (s + 1) & R.kv_mask) {
            const uint64_t sk = R.kv_keys[s];
            if (sk == 0) break;
            if (sk != hk) continue;
            const uint32_t pe = R.kv_idx[s];
            const uint64_t ka = R.kv_off[2 * pe], kb = R.kv_off[2 * pe + 1];
            if (kb - ka != kl) continue;
            bool same = true;
            for (uint32_t q = 0; q < kl && same; ++q) {
                uint8_t ch = key[q];
                if (R.icase && ch >= 'A' && ch <= 'Z') ch += 32;
                same = ch == R.kv_blob[ka + q];
            }
            if (same) { e = pe; break; }
        }
        if (e >= 0) { val = R.kv_blob + R.kv_off[2 * e + 1]; vl = (uint32_t)(R.kv_off[2 * e + 2] - R.kv_off[2 * e + 1]); }
        else if (R.keep_untouch) { rep_len[i] = 0; return; }
        else if (R.keep_key) { val = key; vl = kl; }
        else { val = R.miss; vl = R.miss_len; }
        if (!val) val = R.tmpl;  // (an empty value: any non-null pointer)
    }
    uint8_t rb[REPL_TMPL_MAX];
    const uint32_t rl = build_template(R, R.nr_base + i + 1u, val, vl, rb);
    if (rl == NONE) { flag(R, REPL_ERR_TMPL, i); rep_len[i] = 0; return; }
    const GroupNames names{R.names, R.name_off, R.ngroups};
    if (!WRITE) {
        uint64_t cnt = 0;  // (a template can make a head grow without bound: counted in 64 bits, checked below)
        auto count = [&cnt](uint8_t) { ++cnt; };
        const uint32_t hits = vm_replace_all<NCAP>(P, text, hl, rb, rl, names, count);
        if (!hits) { rep_len[i] = 0; return; }
        // the whole output record -- marker, head, '\n', wrapped sequence, '\n' (+ "+\n" quality '\n') -- in u32
        const uint64_t L = t.l_seq[i];
        const uint64_t W = (!R.fastq && R.line_width > 0) ? (uint64_t)R.line_width : 0u;
        const uint64_t wl = (W && L) ? L + (L - 1) / W : L;
        const uint64_t total = 1u + cnt + 1u + wl + 1u + (R.fastq ? 2u + L + 1u : 0u);
        if (total > REPL_RECORD_MAX) { flag(R, REPL_ERR_SIZE, i); rep_len[i] = 0; return; }
        rep_len[i] = (uint32_t)cnt + 1u;
    } else {
        uint8_t* o = stage + rep_off[i];
        uint32_t x = 0;
        auto put = [o, &x](uint8_t ch) { o[x++] = ch; };
        vm_replace_all<NCAP>(P, text, hl, rb, rl, names, put);
    }
}

__device__ __forceinline__ bool in_cls(const uint32_t* s, uint8_t c) { return (s[c >> 5] >> (c & 31)) & 1u; }

// -s: record.Seq.Seq = ReplaceAll(seq, -r); record.Format(LineWidth): '>' name '\n' wrapped sequence '\n'
template <int NCAP, bool WRITE>
__global__ __launch_bounds__(64) void k_repl_seq(const uint8_t* __restrict__ buf, RecordTable t, TextTable tt, ReplParams R,
                                                 uint32_t* __restrict__ out_len, const uint64_t* __restrict__ out_off,
                                                 uint8_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.n) return;
    const uint32_t lh = t.l_head[i];
    const uint8_t* h = buf + t.start[i] + 1;
    const uint32_t hl = lh > 0 ? lh - 1 : 0;
    const Text T = text_of(buf, t, tt, i);
    auto text = [&T](uint32_t k) { return T.at(k); };
    if (!WRITE) {
        for (uint32_t k = 0; k < T.L; ++k)
            if (T.at(k) >= 0x80) { flag(R, REPL_ERR_NONASCII, i); out_len[i] = 0; return; }
    }
    const uint64_t W = R.line_width > 0 ? (uint64_t)R.line_width : 0u;
    uint64_t L = 0;          // sequence bytes out so far (64 bits: a template can make a record grow without bound)
    uint8_t* o = WRITE ? out + out_off[i] : nullptr;
    uint32_t x = 0;
    if (WRITE) {
        o[x++] = '>';
        for (uint32_t k = 0; k < hl; ++k) o[x++] = h[k];
        o[x++] = '\n';
    }
    auto put = [&](uint8_t ch) {
        if (WRITE) {
            if (W && L && L % W == 0) o[x++] = '\n';
            o[x++] = ch;
        }
        ++L;
    };
    if (R.byte_class) {
        // one position, no assertion, not nullable: every byte is its own match or no match, so ReplaceAll is a map
        const uint32_t caps[4] = {0u, 1u, R.class_group1 ? 0u : NONE, R.class_group1 ? 1u : NONE};
        const GroupNames names{R.names, R.name_off, R.ngroups};
        for (uint32_t k = 0; k < T.L; ++k) {
            const uint8_t c = T.at(k);
            if (!in_cls(R.cls, c)) { put(c); continue; }
            vm_expand(R.tmpl, R.tmpl_len, [c](uint32_t) { return c; }, caps, 4u, R.ngroups, names, put);
        }
    } else {
        const GroupNames names{R.names, R.name_off, R.ngroups};
        vm_replace_all<NCAP>(*R.prog, text, T.L, R.tmpl, R.tmpl_len, names, put);
    }
    if (WRITE) o[x++] = '\n';
    else {
        const uint64_t wl = (W && L) ? L + (L - 1) / W : L;
        const uint64_t total = 1u + (uint64_t)hl + 1u + wl + 1u;
        if (total > REPL_RECORD_MAX) { flag(R, REPL_ERR_SIZE, i); out_len[i] = 0; return; }
        out_len[i] = (uint32_t)total;
    }
}

template <int NCAP>
hipError_t heads(bool write, const uint8_t* buf, const RecordTable& t, const ReplParams& R, uint32_t* rep_len,
                 const uint64_t* rep_off, uint8_t* stage, hipStream_t st) {
    const uint32_t blocks = (uint32_t)((t.n + 63) / 64);
    if (write) hipLaunchKernelGGL((k_repl_heads<NCAP, true>), dim3(blocks), dim3(64), 0, st, buf, t, R, rep_len, rep_off, stage);
    else hipLaunchKernelGGL((k_repl_heads<NCAP, false>), dim3(blocks), dim3(64), 0, st, buf, t, R, rep_len, rep_off, stage);
    return hipGetLastError();
}

template <int NCAP>
hipError_t seqs(bool write, const uint8_t* buf, const RecordTable& t, const TextTable& tt, const ReplParams& R,
                uint32_t* out_len, const uint64_t* out_off, uint8_t* out, hipStream_t st) {
    const uint32_t blocks = (uint32_t)((t.n + 63) / 64);
    if (write) hipLaunchKernelGGL((k_repl_seq<NCAP, true>), dim3(blocks), dim3(64), 0, st, buf, t, tt, R, out_len, out_off, out);
    else hipLaunchKernelGGL((k_repl_seq<NCAP, false>), dim3(blocks), dim3(64), 0, st, buf, t, tt, R, out_len, out_off, out);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_repl_heads(int ncap, bool write, const uint8_t* buf, const RecordTable& t, const ReplParams& R,
                             uint32_t* rep_len, const uint64_t* rep_off, uint8_t* stage, hipStream_t st) {
    if (t.n == 0) return hipSuccess;
    if (ncap <= 4) return heads<4>(write, buf, t, R, rep_len, rep_off, stage, st);
    if (ncap <= 8) return heads<8>(write, buf, t, R, rep_len, rep_off, stage, st);
    return heads<20>(write, buf, t, R, rep_len, rep_off, stage, st);
}

hipError_t launch_repl_seq(int ncap, bool write, const uint8_t* buf, const RecordTable& t, const uint32_t* text_w,
                           const uint64_t* lin_off, const uint8_t* lin, const ReplParams& R, uint32_t* out_len,
                           const uint64_t* out_off, uint8_t* out, hipStream_t st) {
    if (t.n == 0) return hipSuccess;
    TextTable tt;
    tt.text_w = text_w; tt.lin_off = lin_off; tt.lin = lin; tt.lin_n = 0;
    if (ncap <= 4) return seqs<4>(write, buf, t, tt, R, out_len, out_off, out, st);
    if (ncap <= 8) return seqs<8>(write, buf, t, tt, R, out_len, out_off, out, st);
    return seqs<20>(write, buf, t, tt, R, out_len, out_off, out, st);
}

}  // namespace bsk
