// Host side of `concat` in buckets of the key (include/bsk.h; PARITY.md CONB).  Two phases over file 1 followed by file 2:
//   match   in buckets of the key, on c->rdb with the steps of `rmdup` in buckets of the key (ops_host_rmdupbuckets.cpp:
//           rdb_hist_device, rdb_bucket_begin, rdb_bucket_add, rdb_group_keys, rdb_flagged_texts), as the match phase of `pair`.  A
//           bucket ends in its share of the verdict: head[g] of the records of both files.  A bucket receives file 1 before
//           file 2 and its accumulated indices ascend with g, so the first record of a key group is the group's lowest g
//   join    in windows of file 1, on c->cab.win with the steps of the shuffle kind (bucket_hist_alloc, bucket_begin,
//           BucketAccumulate, packed): the weights W and C of the heads over file 2, the window histogram of the costs over file 1,
//           and per window the records of file 1 of its bins followed by the records of file 2 that they pull in -- on which
//           concat_run_device runs: the window's share of the output.  The tail (Full) filters a shard of file 2 by "no head"
// The kernels are in ops_concat_buckets.hip.  A match bucket finishes in rdb_bucket_finish around catb_bucket_decide
// (rdb_flagged_read / rdb_flagged_settle); the verdict is opened here, not by rdb_verdict_open: see concat_verdict_begin.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/bsk.h"
#include "ctx.hpp"
#include "ops_concat_buckets.hpp"
#include "ops_host.hpp"
#include "ops_host_internal.hpp"
#include "ops_records.hpp"
#include "ops_seq.hpp"

namespace bsk {

static int catb_fail(bsk_ctx* c, const char* fn, const std::string& what) {
    c->set_error(std::string("libbsk: bsk_concat_") + fn + ": " + what);
    return BSK_ERR_INVALID_ARG;
}
static int catb_require_joined(bsk_ctx* c, const char* fn) {
    if (c->rdb.verdict && c->cab.joined) return BSK_OK;
    if (!c->rdb.verdict) return catb_fail(c, fn, "no verdict (bsk_concat_verdict_begin and the buckets first)");
    return catb_fail(c, fn, "the join phase has not begun (bsk_concat_join_begin first)");
}
static int catb_window_state(bsk_ctx* c, const char* fn, bool want_open) {
    if (c->cab.win.open == want_open) return BSK_OK;
    return catb_fail(c, fn, want_open ? "no window is open (bsk_concat_window_begin first)" : "a window is open (bsk_concat_window_finish ends it)");
}
static int catb_no_slices(bsk_ctx* c, const char* fn) {
    if (!slices_wanted(c)) return BSK_OK;
    c->set_error(std::string("libbsk: bsk_concat_") + fn + ": out=slices is not available on the concat path in buckets of the key");
    return BSK_ERR_UNSUPPORTED;
}
// the records first_record .. first_record + N of a shard: inside the union, and inside ONE file; which = 0: either file,
// 1 / 2: that file
static int catb_shard_range(bsk_ctx* c, const char* fn, uint64_t first_record, uint64_t N, int which = 0) {
    const uint64_t n1 = c->rdb.file_sums[0], total = c->rdb.total_records;
    const std::string span = "the shard's records " + std::to_string(first_record) + " .. " + std::to_string(first_record + N);
    if (first_record > total || N > total - first_record)
        return catb_fail(c, fn, span + " reach past the sum of file_records = " + std::to_string(total) + " of bsk_concat_verdict_begin");
    if (first_record < n1 && N > n1 - first_record)
        return catb_fail(c, fn, span + " straddle the two files (file 1 ends at record " + std::to_string(n1) + "; a shard belongs to one file)");
    if (N && which == 1 && first_record >= n1)
        return catb_fail(c, fn, span + " lie in file 2 (this pass runs over file 1, records 0 .. " + std::to_string(n1) + ")");
    if (N && which == 2 && first_record < n1)
        return catb_fail(c, fn, span + " lie in file 1 (this pass runs over file 2, records " + std::to_string(n1) + " .. " + std::to_string(total) + ")");
    return BSK_OK;
}

// ---- the verdict
int concat_verdict_begin(bsk_ctx* c, const uint64_t* file_records) {
    bsk_ctx::RmDupBuckets& B = c->rdb;
    bsk_ctx::ConcatBuckets& P = c->cab;
    int rc = bucket_require_closed(c, B, "concat", "verdict_begin");
    if (rc == BSK_OK) rc = catb_window_state(c, "verdict_begin", false);
    if (rc != BSK_OK) return rc;
    const uint64_t n1 = file_records[0], n2 = file_records[1];
    if (n2 > ~n1) return catb_fail(c, "verdict_begin", "the sum of file_records does not fit 64 bits");
    // (written out, not rdb_verdict_open: 64-bit words of 0xFF, and none to write for an empty input)
    HIP_TRYX(c, hipDeviceSynchronize());
    rc = grow(c, &P.d_head, &P.head_cap, n1 + n2);
    if (rc != BSK_OK) return rc;
    if (n1 + n2) HIP_TRYX(c, hipMemset(P.d_head, 0xFF, (n1 + n2) * sizeof(uint64_t)));
    P.joined = false;
    P.weighed = 0;
    P.shift = 0;
    B.total_records = n1 + n2;
    B.file_sums = {n1, n1 + n2};
    B.verdict = true;
    std::fill(B.decided.begin(), B.decided.end(), (uint8_t)0);
    return BSK_OK;
}

int concat_verdict_get(bsk_ctx* c, uint64_t first, uint64_t count, uint64_t* head) {
    const bsk_ctx::RmDupBuckets& B = c->rdb;
    if (!B.verdict) return catb_fail(c, "verdict_get", "no verdict (bsk_concat_verdict_begin first)");
    if (first > B.total_records || count > B.total_records - first)
        return catb_fail(c, "verdict_get", "records " + std::to_string(first) + " .. reach past the " + std::to_string(B.total_records) +
                                               " records of the verdict");
    if (count == 0) return BSK_OK;
    HIP_TRYX(c, hipDeviceSynchronize());
    HIP_TRYX(c, hipMemcpy(head, c->cab.d_head + first, count * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return BSK_OK;
}

// ---- the match phase: one bucket
int concat_bucket_begin(bsk_ctx* c, uint32_t lo_bin, uint32_t hi_bin) {
    if (c->rdb.verdict && c->cab.joined)
        return catb_fail(c, "bucket_begin", "the join phase has begun on this verdict (bsk_concat_verdict_begin starts a new one)");
    return rdb_bucket_begin(c, lo_bin, hi_bin);
}

int concat_bucket_add(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st) {
    int rc = bucket_require_open(c, c->rdb, "concat", "add");
    if (rc != BSK_OK) return rc;
    rc = rdb_bucket_add(c, d_buf, n, format, first_record, st);
    if (rc != BSK_OK) return rc;
    return catb_shard_range(c, "bucket_add", first_record, c->table.n);
}

// The flagged records settled on the host: grouped by text -- a text other than the first text of its key group has ALL its
// records flagged, because they share k1 --, the head of a text = its lowest flagged record when that one is of file 1 (the list
// is in input order, file 1 first).  *matched = the flagged records that have a head.
static int catb_settle_flagged(bsk_ctx* c, uint32_t m, hipStream_t st, uint64_t* matched) {
    *matched = 0;
    return rdb_flagged_texts(c, m, st, [&](const std::vector<uint32_t>& list, const std::vector<uint64_t>& gidx, const std::string& blob,
                                           const std::vector<uint64_t>& off) {
        const uint64_t n1 = c->rdb.file_sums[0];
        std::unordered_map<std::string, uint64_t> head_of;
        std::vector<uint64_t> gh(2 * (size_t)m);  // the records, then their heads
        for (uint32_t j = 0; j < m; ++j) {
            const uint64_t g = gidx[list[j]];
            const uint64_t h = head_of.emplace(blob.substr(off[j], off[j + 1] - off[j]), g < n1 ? g : CATB_NONE).first->second;
            gh[j] = g;
            gh[m + j] = h;
            *matched += h != CATB_NONE ? 1 : 0;
        }
        uint64_t* d_gh = nullptr;
        const bool ok = hipMalloc((void**)&d_gh, gh.size() * 8) == hipSuccess &&
                        hipMemcpyAsync(d_gh, gh.data(), gh.size() * 8, hipMemcpyHostToDevice, st) == hipSuccess &&
                        launch_catb_set(d_gh, d_gh + m, m, c->cab.d_head, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
        if (d_gh) hipFree(d_gh);
        return ok ? (int)BSK_OK : (int)BSK_ERR_HIP;
    });
}

static int catb_bucket_decide(bsk_ctx* c, hipStream_t st, uint64_t* n_matched, uint64_t* n_flagged) {
    bsk_ctx::RmDupBuckets& B = c->rdb;
    const uint64_t N = B.n;
    if (N == 0) return BSK_OK;
    Arena A;
    uint64_t o_first = 0;
    int rc = rdb_group_keys(c, st, &A, &o_first);
    if (rc != BSK_OK) return rc;
    const uint32_t* first = A.at<uint32_t>(o_first);
    uint64_t* d_matched = c->d_fin + bsk_ctx::FIN_AUX0;
    HIP_TRYX(c, hipMemsetAsync(d_matched, 0, sizeof(uint64_t), st));
    {
        Timed t(c, "k_catb_verify", st);
        HIP_TRYX(c, launch_catb_verify(B.d_acc, B.d_off, B.d_len, B.d_draw, first, N, B.file_sums[0], c->cab.d_head, c->d_xflag,
                                       (uint32_t)RDB_FLAG_MAX, d_matched, st));
    }
    rc = rdb_flagged_read(c, st, n_matched, n_flagged);  // (the arena is the next call's)
    if (rc != BSK_OK) return rc;
    return rdb_flagged_settle(c, *n_flagged, "catb_settle_flagged", st, n_matched, catb_settle_flagged);
}

int concat_bucket_finish(bsk_ctx* c, hipStream_t st, uint64_t* n_matched, uint64_t* n_flagged) {
    return rdb_bucket_finish(c, st, n_matched, n_flagged, catb_bucket_decide);
}

// ---- the join phase
int concat_join_begin(bsk_ctx* c, hipStream_t st) {
    bsk_ctx::RmDupBuckets& B = c->rdb;
    bsk_ctx::ConcatBuckets& P = c->cab;
    if (!B.verdict) return catb_fail(c, "join_begin", "no verdict (bsk_concat_verdict_begin and the buckets first)");
    int rc = bucket_require_closed(c, B, "concat", "join_begin");
    if (rc == BSK_OK) rc = catb_window_state(c, "join_begin", false);
    if (rc != BSK_OK) return rc;
    for (uint32_t b = 0; b < BUCKET_BINS; ++b)
        if (!B.decided[b])
            return catb_fail(c, "join_begin", "fine bin " + std::to_string(b) + " has not been decided (every bin belongs to a bucket that "
                                                  "was finished since bsk_concat_verdict_begin)");
    const uint64_t n1 = B.file_sums[0], words = (n1 + 31) / 32 + 1;
    HIP_TRYX(c, hipDeviceSynchronize());
    if (n1 > P.wc_cap || !P.d_w || !P.d_c) {
        for (void* p : {(void*)P.d_w, (void*)P.d_c}) if (p) HIP_TRYX(c, hipFree(p));
        P.d_w = nullptr;
        P.d_c = nullptr;
        P.wc_cap = 0;
        HIP_TRYX(c, hipMalloc((void**)&P.d_w, std::max<uint64_t>(n1, 1) * sizeof(uint64_t)));
        HIP_TRYX(c, hipMalloc((void**)&P.d_c, std::max<uint64_t>(n1, 1) * sizeof(uint64_t)));
        P.wc_cap = n1;
    }
    rc = grow(c, &P.d_mark, &P.mark_words, words);
    if (rc != BSK_OK) return rc;
    if (n1) {
        HIP_TRYX(c, hipMemsetAsync(P.d_w, 0, n1 * sizeof(uint64_t), st));
        HIP_TRYX(c, hipMemsetAsync(P.d_c, 0, n1 * sizeof(uint64_t), st));
    }
    HIP_TRYX(c, hipMemsetAsync(P.d_mark, 0, words * sizeof(uint32_t), st));
    HIP_TRYX(c, hipStreamSynchronize(st));
    rc = bucket_hist_alloc(c, &P.win, st);
    if (rc == BSK_OK) rc = bucket_hist_reset(c, &P.win);
    if (rc != BSK_OK) return rc;
    P.shift = 0;
    while (n1 && ((n1 - 1) >> P.shift) >= BUCKET_BINS) ++P.shift;
    P.weighed = 0;
    P.joined = true;
    return BSK_OK;
}

int concat_weigh_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st, uint64_t* n_records) {
    bsk_ctx::ConcatBuckets& P = c->cab;
    c->last_kernel_flags = 0;
    int rc = catb_require_joined(c, "weigh_run");
    if (rc != BSK_OK) return rc;
    rc = index_shard_status(c, d_buf, n, format, st);  // (the weights accumulate: the complaints of the index pass come first)
    if (rc != BSK_OK) return rc;
    const uint64_t N = c->table.n;
    rc = catb_shard_range(c, "weigh_run", first_record, N, 2);
    if (rc != BSK_OK) return rc;
    if (n_records) *n_records = N;
    if (N == 0) return BSK_OK;
    {
        Timed tm(c, "k_catb_weigh", st);
        HIP_TRYX(c, launch_catb_weigh(d_buf, n, c->table, format == BSK_FORMAT_FASTQ, first_record, P.d_head, P.d_w, P.d_c, st));
    }
    HIP_TRYX(c, hipStreamSynchronize(st));  // (the shard may be a staging buffer that the next call overwrites)
    P.weighed += N;
    return BSK_OK;
}

static int catb_require_weighed(bsk_ctx* c, const char* fn) {
    const uint64_t n2 = c->rdb.file_sums[1] - c->rdb.file_sums[0];
    if (c->cab.weighed == n2) return BSK_OK;
    return catb_fail(c, fn, std::to_string(c->cab.weighed) + " records have been weighed, file 2 has " + std::to_string(n2) +
                                " (bsk_concat_weigh_run over every shard of file 2, once, since bsk_concat_join_begin)");
}

int concat_window_hist_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st, uint64_t* n_records) {
    bsk_ctx::ConcatBuckets& P = c->cab;
    c->last_kernel_flags = 0;
    int rc = catb_require_joined(c, "window_hist_run");
    if (rc == BSK_OK) rc = catb_require_weighed(c, "window_hist_run");
    if (rc != BSK_OK) return rc;
    rc = index_shard_status(c, d_buf, n, format, st);  // (the counters accumulate: the complaints of the index pass come first)
    if (rc != BSK_OK) return rc;
    const uint64_t N = c->table.n;
    rc = catb_shard_range(c, "window_hist_run", first_record, N, 1);
    if (rc != BSK_OK) return rc;
    if (n_records) *n_records = N;
    if (N == 0) return BSK_OK;
    {
        Timed tm(c, "k_catb_hist", st);
        HIP_TRYX(c, launch_catb_hist(d_buf, n, c->table, format == BSK_FORMAT_FASTQ, first_record, P.d_head, P.d_w, P.d_c, P.shift, P.win.d_hist,
                                     P.win.d_hist + BUCKET_BINS, c->num_cus, st));
    }
    HIP_TRYX(c, hipStreamSynchronize(st));
    return BSK_OK;
}

int concat_window_hist_get(bsk_ctx* c, uint64_t* bytes, uint64_t* records) {
    const int rc = catb_require_joined(c, "window_hist_get");
    if (rc != BSK_OK) return rc;
    return bucket_hist_get(c, &c->cab.win, bytes, records);
}

int concat_window_begin(bsk_ctx* c, uint32_t lo_bin, uint32_t hi_bin) {
    bsk_ctx::ConcatBuckets& P = c->cab;
    int rc = catb_require_joined(c, "window_begin");
    if (rc == BSK_OK) rc = catb_window_state(c, "window_begin", false);
    if (rc != BSK_OK) return rc;
    // (the cost of the bins is a planning bound: the accumulation grows as the shares arrive, nothing is reserved from it)
    rc = bucket_begin(c, &P.win, "concat_window", lo_bin, hi_bin, [](uint64_t, uint64_t) { return (int)BSK_OK; });
    if (rc != BSK_OK) return rc;
    const hipError_t e = hipMemset(P.d_mark, 0, ((c->rdb.file_sums[0] + 31) / 32 + 1) * sizeof(uint32_t));
    if (e != hipSuccess) {
        bucket_close(&P.win);
        c->set_error(std::string("libbsk: bsk_concat_window_begin: clearing the mark bits: ") + hipGetErrorString(e));
        return BSK_ERR_HIP;
    }
    P.win_format = -1;
    P.in_file2 = false;
    P.kept1 = P.bytes1 = P.seen2 = 0;
    return BSK_OK;
}

int concat_window_add(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st) {
    bsk_ctx::ConcatBuckets& P = c->cab;
    bsk_ctx::BucketState& B = P.win;
    c->last_kernel_flags = 0;
    int rc = catb_require_joined(c, "window_add");
    if (rc == BSK_OK) rc = catb_window_state(c, "window_add", true);
    if (rc != BSK_OK) return rc;
    if (P.in_file2 && first_record < c->rdb.file_sums[0])
        return catb_fail(c, "window_add", "a shard of file 1 (first_record " + std::to_string(first_record) + ") after a shard of file 2: the records of "
                                              "file 1 come first in a window");
    if (first_record < B.next_first)  // (the rule of bucket_in_order)
        return catb_fail(c, "window_add", "first_record " + std::to_string(first_record) + " goes backwards (the shards of a window are added in input "
                                              "order; the next one starts at record " + std::to_string(B.next_first) + " or later)");
    if (P.win_format >= 0 && P.win_format != format) return catb_fail(c, "window_add", "the shards of a window have one format");
    rc = index_shard_status(c, d_buf, n, format, st);
    if (rc != BSK_OK) return rc;
    const uint64_t N = c->table.n, n1 = c->rdb.file_sums[0];
    rc = catb_shard_range(c, "window_add", first_record, N);
    if (rc != BSK_OK) return rc;
    if (N == 0) return BSK_OK;
    const bool file2 = first_record >= n1;
    if (file2 && !P.in_file2) {  // the boundary inside the accumulation
        P.in_file2 = true;
        P.kept1 = B.n;
        P.bytes1 = B.acc_used;
    }
    const int fastq = format == BSK_FORMAT_FASTQ;
    BucketAccumulate step{c, &B, d_buf, st, "concat_window", true};
    step.pick = [&](size_t n_eff, int fastq_eff, uint32_t* out_len, uint32_t* keep) -> int {
        Timed tm(c, file2 ? "k_catb_pick" : "k_catb_mark", st);
        if (file2)
            HIP_TRYX(c, launch_catb_pick(d_buf, n_eff, c->table, fastq_eff, first_record, P.d_head, P.d_mark, out_len, keep, c->d_status, st));
        else
            HIP_TRYX(c, launch_catb_mark(d_buf, n_eff, c->table, fastq_eff, first_record, P.d_head, P.shift, B.lo, B.hi, P.d_mark, out_len, keep,
                                         c->d_status, st));
        return BSK_OK;
    };
    rc = step.queue(n, fastq);
    if (rc != BSK_OK) return rc;
    uint64_t status = 0;
    HIP_TRYX(c, hipMemcpyAsync(&status, c->d_status, sizeof status, hipMemcpyDeviceToHost, st));
    HIP_TRYX(c, hipStreamSynchronize(st));
    rc = kernel_error_to_status(c, status);
    if (rc != BSK_OK) return rc;
    rc = step.collect();
    if (rc != BSK_OK) return rc;
    HIP_TRYX(c, hipStreamSynchronize(st));  // (the shard may be a staging buffer that the next call overwrites)
    B.next_first = first_record + N;
    P.win_format = format;
    if (file2) P.seen2 += N;
    return BSK_OK;
}

// the accumulation is file 1's records of the window, then the records of file 2 that they pull in: one call of the operator
static int catb_window_emit(bsk_ctx* c, hipStream_t st, bsk_out* out) {
    bsk_ctx::ConcatBuckets& P = c->cab;
    bsk_ctx::BucketState& B = P.win;
    const uint64_t n2 = c->rdb.file_sums[1] - c->rdb.file_sums[0];
    const uint64_t kept1 = P.in_file2 ? P.kept1 : B.n, bytes1 = P.in_file2 ? P.bytes1 : B.acc_used;
    std::vector<uint64_t> recs(BUCKET_BINS);
    int rc = bucket_hist_get(c, &B, nullptr, recs.data());
    if (rc != BSK_OK) return rc;
    uint64_t want1 = 0;
    for (uint32_t b = B.lo; b < B.hi; ++b) want1 += recs[b];
    if (kept1 != want1)
        return catb_fail(c, "window_finish", "the window holds " + std::to_string(kept1) + " records of file 1, the window histogram has " +
                                                 std::to_string(want1) + " for its bins (every shard of file 1 that reaches into the window is added, once)");
    if (P.seen2 != n2)
        return catb_fail(c, "window_finish", "the window has seen " + std::to_string(P.seen2) + " of the " + std::to_string(n2) +
                                                 " records of file 2 (every shard of file 2 is added, once)");
    if (B.n == 0 || (B.n == kept1 && !c->opts.b("Full"))) return empty_result(c, out);  // (no mate collected: nothing is joined)
    Timed tm(c, "concat_window", st);
    rc = concat_run_device(c, B.d_acc, B.acc_used, bytes1, P.win_format, st, out);
    if (rc != BSK_OK) return rc;
    HIP_TRYX(c, hipStreamSynchronize(st));  // (the accumulation is cleared with the window)
    return BSK_OK;
}

int concat_window_finish(bsk_ctx* c, hipStream_t st, bsk_out* out) {
    int rc = catb_require_joined(c, "window_finish");
    if (rc == BSK_OK) rc = catb_window_state(c, "window_finish", true);
    if (rc == BSK_OK) rc = catb_no_slices(c, "window_finish");
    if (rc != BSK_OK) return rc;
    out->d_data = nullptr;
    out->len = 0;
    out->records = 0;
    rc = catb_window_emit(c, st, out);
    bucket_close(&c->cab.win);
    return rc;
}

// ---- the tail: the records of a shard of file 2 without a head, in order, each as concat_run_device prints an unmatched record
// with Full -- Format(LineWidth)
int concat_tail_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st, bsk_out* out) {
    c->last_kernel_flags = 0;
    int rc = catb_require_joined(c, "tail_run");
    if (rc == BSK_OK) rc = catb_no_slices(c, "tail_run");
    if (rc != BSK_OK) return rc;
    const bool fastq = format == BSK_FORMAT_FASTQ;
    rc = index_shard_status(c, d_buf, n, format, st);
    if (rc != BSK_OK) return rc;
    const uint64_t N = c->table.n;
    rc = catb_shard_range(c, "tail_run", first_record, N, 2);
    if (rc != BSK_OK) return rc;
    if (N == 0 || !c->opts.b("Full")) return empty_result(c, out);
    TextTableH tt;
    rc = prepare_text(c, d_buf, format, st, &tt);
    if (rc != BSK_OK) return rc;
    rc = ensure_record_scratch(c);
    if (rc != BSK_OK) return rc;
    SeqParams F = format_params(c, fastq);
    F.text_w = tt.text_w; F.lin_off = tt.lin_off; F.lin = tt.lin;
    F.buf_end = d_buf + n;
    HIP_TRYX(c, hipMemsetAsync(c->d_status, 0, 2 * sizeof(uint64_t), st));
    HIP_TRYX(c, launch_seq_size(d_buf, c->table, F, c->d_out_len, c->d_status, st));
    {
        Timed tm(c, "k_catb_tail", st);
        HIP_TRYX(c, launch_catb_tail(c->cab.d_head, first_record, N, c->d_out_len, st));
    }
    uint64_t total = 0, kept = 0;
    rc = finish_sizes(c, st, &total, &kept);
    if (rc != BSK_OK) return rc;
    out->d_data = nullptr;
    out->len = 0;
    out->records = 0;
    if (total == 0) return BSK_OK;
    rc = ensure_out(c, total);
    if (rc != BSK_OK) return rc;
    apply_long(c, &F);
    rc = emit_records(c, d_buf, n, F, total, kept, st);
    if (rc != BSK_OK) return rc;
    out->d_data = c->d_out;
    out->len = total;
    out->records = kept;
    return BSK_OK;
}

}  // namespace bsk
