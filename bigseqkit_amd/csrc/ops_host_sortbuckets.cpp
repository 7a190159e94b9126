// Host side of `sort` in buckets of the key (include/bsk.h; PARITY.md SORT, "Buckets"): the sample of keys, the splitters, the
// histogram pass, the collect pass of one bucket and its finish.  The kernels are in ops_sort_buckets.hip; the accumulate step
// is the one `shuffle` uses (bucket_accumulate, ops_host_shuffle.cpp), and a bucket is sorted by sort_run_device itself.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/bsk.h"
#include "ctx.hpp"
#include "ops_host.hpp"
#include "ops_host_internal.hpp"
#include "ops_records.hpp"
#include "ops_sort.hpp"
#include "ops_sort_buckets.hpp"
#include "sample_dev.hpp"

namespace bsk {

// the padded comparison of PARITY SORT: bytes, the shorter string zero-padded
static int cmp_padded(const uint8_t* a, size_t la, const uint8_t* b, size_t lb) {
    const size_t m = std::min(la, lb);
    const int r = m ? memcmp(a, b, m) : 0;
    if (r) return r;
    for (size_t j = m; j < la; ++j) if (a[j]) return 1;
    for (size_t j = m; j < lb; ++j) if (b[j]) return -1;
    return 0;
}

// (ops_host.hpp) at most max_bins - 1 splitters at the quantiles of the sample, strictly ascending; duplicates collapse.
// A key without its trailing zero bytes is the same key under the padded comparison, and on such keys that comparison is the
// plain one of byte strings.
std::vector<std::string> sort_pick_splitters(std::vector<std::string> keys, uint32_t max_bins) {
    std::vector<std::string> out;
    const uint32_t bins = std::min<uint32_t>(std::max<uint32_t>(max_bins, 1), BUCKET_BINS);
    if (keys.empty() || bins < 2) return out;
    for (std::string& k : keys) while (!k.empty() && k.back() == '\0') k.pop_back();
    std::sort(keys.begin(), keys.end());
    const uint64_t n = keys.size();
    for (uint32_t j = 1; j < bins; ++j) {
        const std::string& s = keys[(size_t)((uint64_t)j * n / bins)];
        if (out.empty() || out.back() < s) out.push_back(s);
    }
    return out;
}

// ---- what every pass does first: the table of the shard and the complaints of the index pass (index_shard_status), the text
// view and the -N keys
struct SortShard {
    TextTableH tt;
    SortParams P;
    SortNatKeys nat;
};
static int sort_index_shard(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, SortShard* S) {
    int rc = index_shard_status(c, d_buf, n, format, st);
    if (rc != BSK_OK || c->table.n == 0) return rc;
    rc = prepare_text(c, d_buf, format, st, &S->tt);
    if (rc != BSK_OK) return rc;
    sort_key_params(c, d_buf, n, format, &S->P);
    return sort_natural_keys(c, d_buf, &S->P, st, &S->nat);
}

// the -l / -b numbers (k_sort_intkeys, with its 16 lanes per record for the gap count) into `int_keys`; the string keys need none
static int sort_key_source(bsk_ctx* c, const uint8_t* d_buf, size_t n, const SortShard& S, uint64_t* int_keys, hipStream_t st,
                           SortKeySource* K) {
    *K = SortKeySource{d_buf, n, S.tt, S.P, nullptr};
    if (S.P.mode < 3) return BSK_OK;
    HIP_TRYX(c, launch_sort_intkeys(d_buf, c->table, S.tt, S.P, int_keys, st));
    K->int_keys = int_keys;
    return BSK_OK;
}

static SortSplitters splitters_of(const bsk_ctx* c) {
    const bsk_ctx::SortBuckets& B = c->sob;
    return SortSplitters{B.d_spl, B.d_spl_off, B.d_spl ? (uint32_t)(B.spl_off.size() - 1) : 0u};
}

// ---- the sample
static void sort_sample_thin(bsk_ctx::SortBuckets& B, uint64_t threshold) {
    B.threshold = threshold;
    size_t w = 0;
    for (size_t r = 0; r < B.sample_keys.size(); ++r) {
        if ((B.sample_draws[r] >> 11) >= threshold) continue;
        if (w != r) { B.sample_keys[w] = std::move(B.sample_keys[r]); B.sample_draws[w] = B.sample_draws[r]; }
        ++w;
    }
    B.sample_keys.resize(w);
    B.sample_draws.resize(w);
}

int sort_sample_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, double rate, hipStream_t st,
                       uint64_t* n_records) {
    bsk_ctx::SortBuckets& B = c->sob;
    c->last_kernel_flags = 0;
    if (!(rate >= 0.0 && rate <= 1.0)) {
        c->set_error("libbsk: bsk_sort_sample_run: the rate must lie in [0, 1]");
        return BSK_ERR_INVALID_ARG;
    }
    SortShard S;
    int rc = sort_index_shard(c, d_buf, n, format, st, &S);
    if (rc != BSK_OK) return rc;
    const uint64_t N = c->table.n;
    if (n_records) *n_records = N;
    // the threshold of the draw's upper 53 bits, as `sample` has it; a lower rate than before thins what is stored
    const uint64_t T = (uint64_t)std::min<long double>(std::ceil((long double)rate * 9007199254740992.0L), 9007199254740992.0L);
    if (!B.sampling) { B.sampling = true; B.threshold = T; }
    else if (T < B.threshold) sort_sample_thin(B, T);
    if (N == 0 || B.threshold == 0) return BSK_OK;
    rc = ensure_record_scratch(c);
    if (rc != BSK_OK) return rc;
    Arena A;
    const uint64_t o_ikeys = A.take(S.P.mode >= 3 ? N * 8 : 0), o_klen = A.take(N * 4), o_take = A.take(N * 4), o_koff = A.take((N + 1) * 8),
                   o_toff = A.take((N + 1) * 8);
    rc = arena_reserve(c, &A);
    if (rc != BSK_OK) return rc;
    SortKeySource K;
    rc = sort_key_source(c, d_buf, n, S, A.at<uint64_t>(o_ikeys), st, &K);
    if (rc != BSK_OK) return rc;
    uint32_t* klen = A.at<uint32_t>(o_klen);
    uint32_t* take = A.at<uint32_t>(o_take);
    uint64_t* koff = A.at<uint64_t>(o_koff);
    uint64_t* toff = A.at<uint64_t>(o_toff);
    Timed tm(c, "k_sort_sample_keys", st);
    HIP_TRYX(c, launch_sort_sample_size(K, c->table, first_record, sample_interval(B.threshold).hi, klen, take, st));
    HIP_TRYX(c, launch_scan_u32(klen, koff, N, c->d_scan_tmp, st));
    HIP_TRYX(c, launch_scan_u32(take, toff, N, c->d_scan_tmp, st));
    uint64_t bytes = 0, count = 0;
    HIP_TRYX(c, hipMemcpyAsync(&bytes, koff + N, sizeof bytes, hipMemcpyDeviceToHost, st));
    HIP_TRYX(c, hipMemcpyAsync(&count, toff + N, sizeof count, hipMemcpyDeviceToHost, st));
    HIP_TRYX(c, hipStreamSynchronize(st));
    if (count == 0) return BSK_OK;
    // the compact list in the output block: draws[count], lengths[count], then the key bytes
    const uint64_t o_lens = count * 8, o_bytes = (count * 12 + 15) & ~15ull;
    rc = ensure_out(c, o_bytes + bytes);
    if (rc != BSK_OK) return rc;
    uint64_t* d_draws = reinterpret_cast<uint64_t*>(c->d_out);
    uint32_t* d_lens = reinterpret_cast<uint32_t*>(c->d_out + o_lens);
    HIP_TRYX(c, launch_sort_sample_emit(K, c->table, first_record, klen, koff, take, toff, c->d_out + o_bytes, d_draws, d_lens, st));
    std::vector<uint8_t> h(o_bytes + bytes);
    HIP_TRYX(c, hipMemcpyAsync(h.data(), c->d_out, h.size(), hipMemcpyDeviceToHost, st));
    HIP_TRYX(c, hipStreamSynchronize(st));
    const uint64_t* draws = reinterpret_cast<const uint64_t*>(h.data());
    const uint32_t* lens = reinterpret_cast<const uint32_t*>(h.data() + o_lens);
    uint64_t at = o_bytes;
    for (uint64_t j = 0; j < count; ++j) {
        B.sample_draws.push_back(draws[j]);
        B.sample_keys.emplace_back(reinterpret_cast<const char*>(h.data() + at), lens[j]);
        at += lens[j];
    }
    // above the cap the sample thins itself: half the threshold, and the stored samples above it leave.  What remains is the
    // sample that the lower threshold would have taken from the start, so it does not depend on the cut into shards either
    const uint64_t cap = (uint64_t)c->tune.num("sort_sample_cap", 1 << 18);
    while (B.sample_keys.size() > cap && B.threshold > 0) sort_sample_thin(B, B.threshold >> 1);
    return BSK_OK;
}

void sort_sample_reset(bsk_ctx* c) {
    bsk_ctx::SortBuckets& B = c->sob;
    B.sample_keys.clear();
    B.sample_draws.clear();
    B.threshold = 0;
    B.sampling = false;
}

// ---- the splitters
int sort_splitters_install(bsk_ctx* c, const std::vector<std::string>& sp) {
    bsk_ctx::SortBuckets& B = c->sob;
    if (B.open) {
        c->set_error("libbsk: sort: the splitters cannot change while a bucket is open");
        return BSK_ERR_INVALID_ARG;
    }
    if (sp.size() > SORT_MAX_SPLITTERS) {
        c->set_error("libbsk: sort: at most 4095 splitters (4096 fine bins)");
        return BSK_ERR_INVALID_ARG;
    }
    uint64_t total = 0;
    for (size_t j = 0; j < sp.size(); ++j) {
        total += sp[j].size();
        if (j && cmp_padded((const uint8_t*)sp[j - 1].data(), sp[j - 1].size(), (const uint8_t*)sp[j].data(), sp[j].size()) >= 0) {
            c->set_error("libbsk: sort: the splitters are not strictly ascending (splitter " + std::to_string(j) +
                         " is not above the one before it; bytes compare with the shorter string zero-padded)");
            return BSK_ERR_INVALID_ARG;
        }
    }
    if (total > (1u << 20)) {
        c->set_error("libbsk: sort: the splitters hold " + std::to_string(total) + " bytes, more than 1 MiB");
        return BSK_ERR_INVALID_ARG;
    }
    HIP_TRYX(c, hipDeviceSynchronize());
    if (B.d_spl) HIP_TRYX(c, hipFree(B.d_spl));
    if (B.d_spl_off) HIP_TRYX(c, hipFree(B.d_spl_off));
    B.d_spl = nullptr;
    B.d_spl_off = nullptr;
    B.spl_bytes.clear();
    B.spl_off.assign(1, 0u);
    for (const std::string& s : sp) { B.spl_bytes += s; B.spl_off.push_back((uint32_t)B.spl_bytes.size()); }
    if (sp.empty()) return BSK_OK;
    HIP_TRYX(c, hipMalloc((void**)&B.d_spl, std::max<size_t>(B.spl_bytes.size(), 16)));
    HIP_TRYX(c, hipMalloc((void**)&B.d_spl_off, B.spl_off.size() * sizeof(uint32_t)));
    if (!B.spl_bytes.empty()) HIP_TRYX(c, hipMemcpy(B.d_spl, B.spl_bytes.data(), B.spl_bytes.size(), hipMemcpyHostToDevice));
    HIP_TRYX(c, hipMemcpy(B.d_spl_off, B.spl_off.data(), B.spl_off.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return BSK_OK;
}

int sort_splitters_build(bsk_ctx* c, uint32_t max_bins, uint32_t* n_bins) {
    const std::vector<std::string> sp = sort_pick_splitters(c->sob.sample_keys, max_bins);
    const int rc = sort_splitters_install(c, sp);
    if (rc == BSK_OK && n_bins) *n_bins = (uint32_t)sp.size() + 1;
    return rc;
}

// ---- the histogram pass
int sort_hist_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, uint64_t* n_records) {
    c->last_kernel_flags = 0;
    int rc = bucket_hist_alloc(c, &c->sob, st);
    if (rc != BSK_OK) return rc;
    SortShard S;
    rc = sort_index_shard(c, d_buf, n, format, st, &S);  // (the counters accumulate: the complaints of the index pass come first)
    if (rc != BSK_OK) return rc;
    const uint64_t N = c->table.n;
    if (n_records) *n_records = N;
    if (N == 0) return BSK_OK;
    Arena A;
    const uint64_t o_ikeys = A.take(S.P.mode >= 3 ? N * 8 : 0), o_bins = A.take(N * 2);
    rc = arena_reserve(c, &A);
    if (rc != BSK_OK) return rc;
    SortKeySource K;
    rc = sort_key_source(c, d_buf, n, S, A.at<uint64_t>(o_ikeys), st, &K);
    if (rc != BSK_OK) return rc;
    {
        Timed tm(c, "k_sort_bins", st);
        HIP_TRYX(c, launch_sort_bins(K, c->table, splitters_of(c), A.at<uint16_t>(o_bins), st));
    }
    Timed tm(c, "k_sort_hist", st);
    HIP_TRYX(c, launch_sort_hist(d_buf, n, c->table, S.P.fastq, A.at<uint16_t>(o_bins), c->sob.d_hist, c->sob.d_hist + BUCKET_BINS, c->num_cus, st));
    return BSK_OK;
}

// ---- one bucket
int sort_bucket_begin(bsk_ctx* c, uint32_t lo_bin, uint32_t hi_bin) {
    const int rc = bucket_begin(c, &c->sob, "sort", lo_bin, hi_bin,
                                [&](uint64_t bytes, uint64_t) { return bucket_acc_reserve(c, &c->sob, bytes, 0, false, nullptr); });
    if (rc == BSK_OK) c->sob.format = -1;
    return rc;
}

static int sort_bucket_add_open(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st) {
    bsk_ctx::SortBuckets& B = c->sob;
    c->last_kernel_flags = 0;
    // ties keep file order because the accumulation receives its records in input order
    int rc = bucket_in_order(c, B, "sort", first_record);
    if (rc != BSK_OK) return rc;
    if (B.format >= 0 && B.format != format) {
        c->set_error("libbsk: bsk_sort_bucket_add: the shards of a bucket have one format");
        return BSK_ERR_INVALID_ARG;
    }
    SortShard S;
    rc = sort_index_shard(c, d_buf, n, format, st, &S);
    if (rc != BSK_OK) return rc;
    const uint64_t N = c->table.n;
    if (N == 0) return BSK_OK;
    BucketAccumulate step{c, &B, d_buf, st, "sort", true};
    const uint64_t o_ikeys = step.A.take(S.P.mode >= 3 ? N * 8 : 0), o_bins = step.A.take(N * 2);
    step.pick = [&](size_t n_eff, int fastq_eff, uint32_t* out_len, uint32_t* keep) -> int {
        SortKeySource K;
        const int rk = sort_key_source(c, d_buf, n_eff, S, step.A.at<uint64_t>(o_ikeys), st, &K);
        if (rk != BSK_OK) return rk;
        uint16_t* bins = step.A.at<uint16_t>(o_bins);
        {
            Timed tm(c, "k_sort_bins", st);
            HIP_TRYX(c, launch_sort_bins(K, c->table, splitters_of(c), bins, st));
        }
        Timed tm(c, "k_sort_pick", st);
        HIP_TRYX(c, launch_sort_pick(d_buf, n_eff, c->table, fastq_eff, bins, B.lo, B.hi, out_len, keep, c->d_status, st));
        return BSK_OK;
    };
    rc = step.queue(n, S.P.fastq);
    if (rc != BSK_OK) return rc;
    uint64_t status = 0;
    HIP_TRYX(c, hipMemcpyAsync(&status, c->d_status, sizeof status, hipMemcpyDeviceToHost, st));
    HIP_TRYX(c, hipStreamSynchronize(st));
    rc = kernel_error_to_status(c, status);
    if (rc != BSK_OK) return rc;
    rc = step.collect();
    if (rc != BSK_OK) return rc;
    B.next_first = first_record + N;
    B.format = format;
    return BSK_OK;
}

int sort_bucket_add(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st) {
    const int rc = bucket_require_open(c, c->sob, "sort", "add");
    if (rc != BSK_OK) return rc;
    // (no close on an error here: a wrapped FASTQ shard comes back once more as its 4-line rewrite -- run_multiline -- and needs
    // the bucket; the entry point closes it when the call has failed for good, bucket_close.  rmdup_bucket_add does the same)
    return sort_bucket_add_open(c, d_buf, n, format, first_record, st);
}

int sort_bucket_finish(bsk_ctx* c, hipStream_t st, bsk_out* out) {
    bsk_ctx::SortBuckets& B = c->sob;
    int rc = bucket_require_open(c, B, "sort", "finish");
    if (rc != BSK_OK) return rc;
    if (B.n == 0) {
        rc = empty_result(c, out);
    } else {
        // the accumulation is one text in input order: the keys, the tie pass, Format(LineWidth) and the copy are sort's own
        Timed tm(c, "sort_bucket_sort", st);
        rc = sort_run_device(c, B.d_acc, B.acc_used, B.format, st, out);
    }
    bucket_close(&B);
    return rc;
}

}  // namespace bsk
