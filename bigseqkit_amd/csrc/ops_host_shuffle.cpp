// Host side of `shuffle` (PARITY.md SHUF): the order-and-emit that the one-pass shuffle (records_run_device, ops_host_next.cpp)
// and the finish of a bucket share, and the passes of the shuffle in buckets of the draw.  The kernels are in ops_sample.hip.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <optional>
#include <type_traits>
#include <vector>

#include "../../include/bsk.h"
#include "ctx.hpp"
#include "ops_host.hpp"
#include "ops_host_internal.hpp"
#include "ops_records.hpp"
#include "ops_sample.hpp"
#include "ops_segcopy.hpp"
#include "ops_sort.hpp"

namespace bsk {

// (ops_host_internal.hpp)
int shuffle_order_emit(bsk_ctx* c, const ShuffleRecords& R, hipStream_t st, bsk_out* out) {
    const uint64_t N = R.N;
    out->d_data = nullptr;
    out->len = 0;
    out->records = 0;
    if (N == 0) return BSK_OK;
    size_t tmp_bytes = 0;
    int rc = sort_query(c, sort_pairs_bits_iota_temp_bytes(N, 0, 64, &tmp_bytes));
    if (rc != BSK_OK) return rc;
    Arena A;
    const uint64_t o_sorted = A.take(N * 8), o_perm = A.take(N * 4), o_len = A.take(N * 4), o_off = A.take((N + 1) * 8),
                   o_tmp = A.take(tmp_bytes ? tmp_bytes : 16), o_keys = A.take(R.draws ? 0 : N * 8);
    rc = arena_reserve(c, &A);
    if (rc != BSK_OK) return rc;
    uint32_t* perm = A.at<uint32_t>(o_perm);
    uint32_t* len_perm = A.at<uint32_t>(o_len);
    uint64_t* seg_off = A.at<uint64_t>(o_off);
    // the scan of N lengths: N need not be the record count of c->table that ensure_record_scratch sized the scratch for
    rc = grow(c, &c->d_scan_tmp, &c->scan_tmp_cap, 3 * ((N + 2047) / 2048) + 6, 16);
    if (rc != BSK_OK) return rc;
    rc = seg_begin(c, N, R.total, st);
    if (rc != BSK_OK) return rc;
    rc = ensure_out(c, R.total);
    if (rc != BSK_OK) return rc;
    const uint64_t* draws = R.draws;
    if (!draws) {
        Timed tm(c, R.stage_keys, st);
        HIP_TRYX(c, launch_shuffle_keys(N, c->opts.i("Seed"), A.at<uint64_t>(o_keys), st));
        draws = A.at<uint64_t>(o_keys);
    }
    {
        Timed tm(c, R.stage_sort, st);  // (the values are 0 .. N - 1: no iota array is written or read)
        HIP_TRYX(c, launch_sort_pairs_bits_iota(A.at<uint8_t>(o_tmp), tmp_bytes, draws, A.at<uint64_t>(o_sorted), perm, N, 0, 64, st));
    }
    std::optional<Timed> emit;
    if (R.stage_emit) emit.emplace(c, R.stage_emit, st);
    {
        std::optional<Timed> tm;
        if (R.stage_segments) tm.emplace(c, R.stage_segments, st);
        HIP_TRYX(c, launch_shuffle_segments(N, R.text, R.extent, R.off, R.len, perm, c->d_seg_src, len_perm,
                                            R.check_newline ? seg_other(c) : nullptr, st));
    }
    HIP_TRYX(c, launch_scan_u32(len_perm, seg_off, N, c->d_scan_tmp, st));
    if (!segcopy_on(c)) {
        HIP_TRYX(c, launch_shuffle_fix(N, R.text, R.off, perm, len_perm, seg_off, c->d_seg_src, c->d_out, true, st));
    } else {
        uint64_t other = 0;
        rc = seg_run(c, SegList{c->d_seg_src, seg_off, N, R.total}, c->d_out, R.text, R.extent, st, &other);
        if (rc != BSK_OK) return rc;
        if (other) HIP_TRYX(c, launch_shuffle_fix(N, R.text, R.off, perm, len_perm, seg_off, c->d_seg_src, c->d_out, false, st));
    }
    out->d_data = c->d_out;
    out->len = R.total;
    out->records = N;
    return BSK_OK;
}

// ---------------------------------------------------------------------------
// shuffle in buckets of the draw (include/bsk.h; PARITY.md SHUF): the histogram pass, the collect pass of one bucket and its
// finish.  The order of the output is the order of the draws, and a draw is a pure function of (seed, global record index),
// so the records whose draws lie in one interval can be collected from the input piece by piece and sorted on their own.
// ---------------------------------------------------------------------------
int shuffle_hist_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st, uint64_t* n_records) {
    c->last_kernel_flags = 0;
    int fastq = 0;
    int rc = bucket_hist_alloc(c, &c->shb, st);
    if (rc != BSK_OK) return rc;
    // the counters accumulate, so the index pass's complaints (a shard that is wrapped behind its head) are read BEFORE the
    // histogram kernel runs -- of an empty table too: this is the one synchronisation of the pass, nothing is read back after
    // the kernel
    rc = index_record_text(c, d_buf, &n, format, &fastq, st, true, nullptr);
    if (rc != BSK_OK) return rc;
    if (n_records) *n_records = c->table.n;
    if (c->table.n == 0) return BSK_OK;
    Timed tm(c, "k_shuffle_hist", st);
    HIP_TRYX(c, launch_shuffle_hist(d_buf, n, c->table, fastq, first_record, c->opts.i("Seed"), c->shb.d_hist, c->shb.d_hist + BUCKET_BINS,
                                    c->num_cus, st));
    return BSK_OK;
}

int bucket_too_many(bsk_ctx* c, const char* op) {
    c->set_error(std::string("libbsk: ") + op + ": 2^32 or more records in one bucket are not supported (a smaller budget makes more buckets)");
    return BSK_ERR_UNSUPPORTED;
}

// ---- the accumulate step of an open bucket (ops_host_internal.hpp)
int bucket_acc_reserve(bsk_ctx* c, bsk_ctx::BucketAcc* Bp, uint64_t bytes, uint64_t recs, bool with_records, hipStream_t st, uint64_t** extra) {
    bsk_ctx::BucketAcc& B = *Bp;
    auto regrow = [&](auto** p, uint64_t used, uint64_t cap) -> int {
        using T = std::remove_reference_t<decltype(**p)>;
        T* nb = nullptr;
        HIP_TRYX(c, hipMalloc((void**)&nb, std::max<uint64_t>(cap, 1) * sizeof(T)));
        if (*p && used) HIP_TRYX(c, hipMemcpyAsync(nb, *p, used * sizeof(T), hipMemcpyDeviceToDevice, st));
        HIP_TRYX(c, hipStreamSynchronize(st));
        if (*p) HIP_TRYX(c, hipFree(*p));
        *p = nb;
        return BSK_OK;
    };
    int rc = BSK_OK;
    if (bytes > B.acc_cap || !B.d_acc) {
        const uint64_t cap = bytes + bytes / 4 + 4096;
        rc = regrow(&B.d_acc, B.acc_used, cap);
        if (rc != BSK_OK) return rc;
        B.acc_cap = cap;
    }
    if (with_records && (recs > B.rec_cap || !B.d_draw || (extra && !*extra))) {
        const uint64_t cap = recs + recs / 4 + 256;
        rc = extra ? regrow(extra, B.n, cap) : BSK_OK;
        if (rc == BSK_OK) rc = regrow(&B.d_draw, B.n, cap);
        if (rc == BSK_OK) rc = regrow(&B.d_off, B.n, cap);
        if (rc == BSK_OK) rc = regrow(&B.d_len, B.n, cap);
        if (rc != BSK_OK) return rc;
        B.rec_cap = cap;
    }
    return BSK_OK;
}

int BucketAccumulate::queue(size_t n, int fastq) {
    const uint64_t N = c->table.n;
    n_eff = n;
    const int rs = ensure_record_scratch(c);
    if (rs != BSK_OK) return rs;
    const uint64_t o_keep = A.take(N * 4);
    o_koff = A.take((N + 1) * 8);
    const int ra = arena_reserve(c, &A);
    if (ra != BSK_OK) return ra;
    uint32_t* keep = A.at<uint32_t>(o_keep);
    uint64_t* keep_off = A.at<uint64_t>(o_koff);
    const int rp = pick(n, fastq, c->d_out_len, keep);
    if (rp != BSK_OK) return rp;
    HIP_TRYX(c, launch_scan_u32(c->d_out_len, c->d_out_off, N, c->d_scan_tmp, st));
    HIP_TRYX(c, launch_scan_u32(keep, keep_off, N, c->d_scan_tmp, st));
    HIP_TRYX(c, hipMemcpyAsync(&total, c->d_out_off + N, sizeof total, hipMemcpyDeviceToHost, st));
    HIP_TRYX(c, hipMemcpyAsync(&kept, keep_off + N, sizeof kept, hipMemcpyDeviceToHost, st));
    return BSK_OK;
}

int BucketAccumulate::collect() {
    const uint64_t N = c->table.n;
    if (kept == 0) return BSK_OK;
    if (B->n + kept >= (1ull << 32)) return bucket_too_many(c, op);
    const uint64_t at = packed ? B->acc_used : (B->acc_used + 255) & ~255ull;  // (the segmented copy stores aligned 16-byte words)
    int rc = bucket_acc_reserve(c, B, at + total + (packed ? 64 : 0), B->n + kept, (bool)append, st);  // (packed: read as a shard, with the slack of one)
    if (rc != BSK_OK) return rc;
    if (packed) {
        rc = ensure_out(c, total);
        if (rc != BSK_OK) return rc;
    }
    uint8_t* dst = packed ? c->d_out : B->d_acc + at;
    rc = seg_begin(c, N, total, st);
    if (rc != BSK_OK) return rc;
    if (!segcopy_on(c)) {
        // every kept record byte by byte: the fix-up kernel writes the records whose source is 0
        HIP_TRYX(c, hipMemsetAsync(c->d_seg_src, 0, N * sizeof(uint64_t), st));
        HIP_TRYX(c, launch_seg_fix_text(d_buf, c->table, c->d_out_len, c->d_out_off, c->d_seg_src, dst, st));
    } else {
        {
            Timed tm(c, "k_seg_prep", st);
            HIP_TRYX(c, launch_seg_build_text(d_buf, n_eff, c->table, c->d_out_len, c->d_seg_src, seg_other(c), st));
        }
        uint64_t other = 0;
        rc = seg_run(c, SegList{c->d_seg_src, c->d_out_off, N, total}, dst, d_buf, n_eff, st, &other);
        if (rc != BSK_OK) return rc;
        // a last record of the input without its newline gets one here: in the output it can land anywhere
        if (other) HIP_TRYX(c, launch_seg_fix_text(d_buf, c->table, c->d_out_len, c->d_out_off, c->d_seg_src, dst, st));
    }
    if (packed) HIP_TRYX(c, hipMemcpyAsync(B->d_acc + at, dst, total, hipMemcpyDeviceToDevice, st));
    if (append) HIP_TRYX(c, append(N, A.at<uint64_t>(o_koff), B->n, at));
    B->acc_used = at + total;
    B->total += total;
    B->n += kept;
    return BSK_OK;
}

// ---- the life cycle of a bucket (ops_host_internal.hpp)
constexpr size_t HIST_BYTES = 2 * BUCKET_BINS * sizeof(uint64_t);

int bucket_hist_alloc(bsk_ctx* c, bsk_ctx::BucketState* B, hipStream_t st) {
    if (B->d_hist) return BSK_OK;
    HIP_TRYX(c, hipMalloc((void**)&B->d_hist, HIST_BYTES));
    HIP_TRYX(c, hipMemsetAsync(B->d_hist, 0, HIST_BYTES, st));
    return BSK_OK;
}

int bucket_hist_get(bsk_ctx* c, bsk_ctx::BucketState* B, uint64_t* bytes, uint64_t* records) {
    int rc = bucket_hist_alloc(c, B, nullptr);
    if (rc != BSK_OK) return rc;
    HIP_TRYX(c, hipDeviceSynchronize());
    if (bytes) HIP_TRYX(c, hipMemcpy(bytes, B->d_hist, HIST_BYTES / 2, hipMemcpyDeviceToHost));
    if (records) HIP_TRYX(c, hipMemcpy(records, B->d_hist + BUCKET_BINS, HIST_BYTES / 2, hipMemcpyDeviceToHost));
    return BSK_OK;
}

int bucket_hist_reset(bsk_ctx* c, bsk_ctx::BucketState* B) {
    HIP_TRYX(c, hipDeviceSynchronize());
    if (B->d_hist) HIP_TRYX(c, hipMemset(B->d_hist, 0, HIST_BYTES));
    return BSK_OK;
}

int bucket_require_closed(bsk_ctx* c, const bsk_ctx::BucketState& B, const char* op, const char* fn) {
    if (!B.open) return BSK_OK;
    c->set_error(std::string("libbsk: bsk_") + op + "_" + fn + ": a bucket is open (bsk_" + op + "_bucket_finish ends it)");
    return BSK_ERR_INVALID_ARG;
}

int bucket_require_open(bsk_ctx* c, const bsk_ctx::BucketState& B, const char* op, const char* fn) {
    if (B.open) return BSK_OK;
    c->set_error(std::string("libbsk: bsk_") + op + "_bucket_" + fn + ": no bucket is open (bsk_" + op + "_bucket_begin first)");
    return BSK_ERR_INVALID_ARG;
}

int bucket_in_order(bsk_ctx* c, const bsk_ctx::BucketState& B, const char* op, uint64_t first_record) {
    if (first_record >= B.next_first) return BSK_OK;
    c->set_error(std::string("libbsk: bsk_") + op + "_bucket_add: first_record " + std::to_string(first_record) + " goes backwards (the shards of a "
                 "bucket are added in input order; the next one starts at record " + std::to_string(B.next_first) + " or later)");
    return BSK_ERR_INVALID_ARG;
}

int bucket_begin(bsk_ctx* c, bsk_ctx::BucketState* Bp, const char* op, uint32_t lo_bin, uint32_t hi_bin,
                 const std::function<int(uint64_t bytes, uint64_t recs)>& reserve) {
    bsk_ctx::BucketState& B = *Bp;
    int rc = bucket_require_closed(c, B, op, "bucket_begin");
    if (rc != BSK_OK) return rc;
    B.lo = lo_bin;
    B.hi = hi_bin;
    B.next_first = 0;
    bucket_acc_clear(&B);
    if (B.d_hist) {
        // the histogram of this context says what the bucket will hold: the accumulation is allocated once (a shard more than
        // expected grows it)
        std::vector<uint64_t> h(2 * BUCKET_BINS);
        HIP_TRYX(c, hipDeviceSynchronize());
        HIP_TRYX(c, hipMemcpy(h.data(), B.d_hist, HIST_BYTES, hipMemcpyDeviceToHost));
        uint64_t bytes = 0, recs = 0;
        for (uint32_t b = lo_bin; b < hi_bin; ++b) { bytes += h[b]; recs += h[BUCKET_BINS + b]; }
        if (recs >= (1ull << 32)) return bucket_too_many(c, op);
        if (recs) {
            rc = reserve(bytes, recs);
            if (rc != BSK_OK) return rc;
        }
    }
    B.open = true;
    return BSK_OK;
}

int index_shard_status(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st) {
    const int rc = build_index(c, d_buf, n, format, st);
    if (rc != BSK_OK) return rc;
    uint64_t status = 0;
    HIP_TRYX(c, hipMemcpyAsync(&status, c->d_status, sizeof status, hipMemcpyDeviceToHost, st));
    HIP_TRYX(c, hipStreamSynchronize(st));
    return kernel_error_to_status(c, status);
}

// ---- shuffle: one bucket.  Every shard's share of the accumulation begins on a 256-byte boundary, hence the slack
int shuffle_bucket_begin(bsk_ctx* c, uint32_t lo_bin, uint32_t hi_bin) {
    return bucket_begin(c, &c->shb, "shuffle", lo_bin, hi_bin,
                        [&](uint64_t bytes, uint64_t recs) { return bucket_acc_reserve(c, &c->shb, bytes + 16 * 256, recs, true, nullptr); });
}

static int shuffle_bucket_add_open(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st) {
    bsk_ctx::ShuffleBuckets& B = c->shb;
    c->last_kernel_flags = 0;
    int fastq = 0;
    const int64_t seed = c->opts.i("Seed");
    // the draws of the bucket, both inclusive: those whose upper bits are the bins [lo, hi)
    const uint64_t lo = (uint64_t)B.lo << SHUFFLE_BIN_SHIFT, hi = B.hi >= BUCKET_BINS ? ~0ull : ((uint64_t)B.hi << SHUFFLE_BIN_SHIFT) - 1;
    BucketAccumulate S{c, &B, d_buf, st, "shuffle", false};
    S.pick = [&](size_t n_eff, int fastq_eff, uint32_t* out_len, uint32_t* keep) -> int {
        Timed tm(c, "k_shuffle_pick", st);
        HIP_TRYX(c, launch_sample_size(d_buf, n_eff, c->table, SampleParams{fastq_eff, first_record, seed, lo, hi}, out_len, keep, c->d_status, st));
        return BSK_OK;
    };
    S.append = [&](uint64_t N, const uint64_t* keep_off, uint64_t n0, uint64_t bytes0) {
        return launch_shuffle_append(N, first_record, seed, c->d_out_len, c->d_out_off, keep_off, n0, bytes0, B.d_draw, B.d_off, B.d_len, st);
    };
    const int rc = index_record_text(c, d_buf, &n, format, &fastq, st, false, [&](size_t n_eff, int fastq_eff) -> int {
        S.A = Arena();  // (the strict reader's late complaints run the step once more)
        return S.queue(n_eff, fastq_eff);
    });
    if (rc != BSK_OK) return rc;
    if (c->table.n == 0) {
        bsk_out none;
        return empty_result(c, &none);
    }
    return S.collect();
}

int shuffle_bucket_add(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st) {
    int rc = bucket_require_open(c, c->shb, "shuffle", "add");
    if (rc != BSK_OK) return rc;
    rc = shuffle_bucket_add_open(c, d_buf, n, format, first_record, st);
    if (rc != BSK_OK) bucket_close(&c->shb);
    return rc;
}

int shuffle_bucket_finish(bsk_ctx* c, hipStream_t st, bsk_out* out) {
    int rc = bucket_require_open(c, c->shb, "shuffle", "finish");
    if (rc != BSK_OK) return rc;
    const bsk_ctx::ShuffleBuckets& B = c->shb;
    // the bytes of the bucket are the sum of what its shards added, whatever the order: nothing is read back for them
    rc = shuffle_order_emit(c, ShuffleRecords{B.d_acc, B.acc_used, B.d_off, B.d_len, B.n, B.total, B.d_draw, false, nullptr,
                                                        "shuffle_bucket_sort", nullptr, "shuffle_bucket_copy"}, st, out);
    bucket_close(&c->shb);
    return rc;
}

}  // namespace bsk
