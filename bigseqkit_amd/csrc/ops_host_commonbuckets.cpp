// Host side of `common` in buckets of the key (include/bsk.h; PARITY.md COMB): the verdict -- one KEEP bit per record of the
// FIRST file --, the finish of a bucket and the emit pass.  The histogram, the begin and the add of a bucket and the key
// grouping down to first[] are those of `rmdup` in buckets of the key (ops_host_rmdupbuckets.cpp: rdb_hist_device,
// rdb_bucket_begin, rdb_bucket_add, rdb_group_keys), on the same state c->rdb over the union of the files; the kernels of what a
// bucket decides are in ops_common_buckets.hip, and the emit ends as common_run_device does (launch_seq_size, finish_sizes,
// emit_records).  The verdict opens with rdb_verdict_open, its bits are read by rdb_verdict_bits, the finish is
// rdb_bucket_finish around comb_bucket_decide (rdb_flagged_read / rdb_flagged_settle), and the emit ends in rdb_emit_tail.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/bsk.h"
#include "ctx.hpp"
#include "ops_common_buckets.hpp"
#include "ops_host.hpp"
#include "ops_host_internal.hpp"
#include "ops_rmdup.hpp"
#include "ops_seq.hpp"

namespace bsk {

// ---- the verdict
int common_verdict_begin(bsk_ctx* c, const uint64_t* file_records, uint32_t n_files) {
    bsk_ctx::RmDupBuckets& B = c->rdb;
    const int rc = bucket_require_closed(c, B, "common", "verdict_begin");
    if (rc != BSK_OK) return rc;
    std::vector<uint64_t> sums(n_files);
    uint64_t total = 0;
    for (uint32_t f = 0; f < n_files; ++f) {
        if (file_records[f] > ~total) {
            c->set_error("libbsk: bsk_common_verdict_begin: the sum of file_records does not fit 64 bits");
            return BSK_ERR_INVALID_ARG;
        }
        total += file_records[f];
        sums[f] = total;
    }
    return rdb_verdict_open(c, &B.d_bits, &B.bits_words, (file_records[0] + 31) / 32 + 1, std::move(sums));
}

int common_verdict_get(bsk_ctx* c, uint64_t first, uint64_t count, uint8_t* kept) {
    const bsk_ctx::RmDupBuckets& B = c->rdb;
    if (!B.verdict) {
        c->set_error("libbsk: bsk_common_verdict_get: no verdict (bsk_common_verdict_begin first)");
        return BSK_ERR_INVALID_ARG;
    }
    const uint64_t n0 = B.file_sums[0];
    if (first > n0 || count > n0 - first) {
        c->set_error("libbsk: bsk_common_verdict_get: records " + std::to_string(first) + " .. reach past the " + std::to_string(n0) +
                     " records of the first file (file_records[0] of bsk_common_verdict_begin)");
        return BSK_ERR_INVALID_ARG;
    }
    if (count == 0) return BSK_OK;
    return rdb_verdict_bits(c, B.d_bits, first, count, kept);
}

// ---- one bucket
// The flagged records settled on the host: grouped by text -- a text other than the first text of its key group has ALL its
// records flagged, because they share k1 --, the files of a text from the global indices of its records; the lowest index of a
// text that every file holds gets its bit (launch_comb_set) when it lies in the first file.  *kept = their number.
static int comb_settle_flagged(bsk_ctx* c, uint32_t m, uint64_t full, hipStream_t st, uint64_t* kept) {
    *kept = 0;
    return rdb_flagged_texts(c, m, st, [&](const std::vector<uint32_t>& list, const std::vector<uint64_t>& gidx, const std::string& blob,
                                           const std::vector<uint64_t>& off) {
        const std::vector<uint64_t>& sums = c->rdb.file_sums;
        struct Seen { uint64_t lowest, mask; };
        std::unordered_map<std::string, Seen> seen;  // text -> its lowest global index (the list is in input order) and its files
        for (uint32_t j = 0; j < m; ++j) {
            const uint64_t g = gidx[list[j]];
            const uint64_t file = (uint64_t)(std::upper_bound(sums.begin(), sums.end(), g) - sums.begin());
            Seen& s = seen.emplace(blob.substr(off[j], off[j + 1] - off[j]), Seen{g, 0}).first->second;
            if (file < sums.size()) s.mask |= 1ull << file;
        }
        std::vector<uint64_t> keep;
        for (const auto& kv : seen)
            if (kv.second.mask == full && kv.second.lowest < sums[0]) keep.push_back(kv.second.lowest);
        *kept = keep.size();
        if (keep.empty()) return (int)BSK_OK;
        uint64_t* d_keep = nullptr;
        const bool ok = hipMalloc((void**)&d_keep, keep.size() * 8) == hipSuccess &&
                        hipMemcpyAsync(d_keep, keep.data(), keep.size() * 8, hipMemcpyHostToDevice, st) == hipSuccess &&
                        launch_comb_set(d_keep, keep.size(), c->rdb.d_bits, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
        if (d_keep) hipFree(d_keep);
        return ok ? (int)BSK_OK : (int)BSK_ERR_HIP;
    });
}

static int comb_bucket_decide(bsk_ctx* c, hipStream_t st, uint64_t* n_kept, uint64_t* n_flagged) {
    bsk_ctx::RmDupBuckets& B = c->rdb;
    const uint64_t N = B.n;
    if (N == 0) return BSK_OK;
    const uint32_t nf = (uint32_t)B.file_sums.size();
    const uint64_t full = nf >= 64 ? ~0ull : (1ull << nf) - 1ull;
    Arena A;
    uint64_t o_first = 0;
    int rc = rdb_group_keys(c, st, &A, &o_first);
    if (rc != BSK_OK) return rc;
    // the masks of the heads and the running sums of the records per file, outside the budget as the arena is: first[] has to
    // survive when the arena moves
    const uint64_t keep = A.used;
    const uint64_t o_masks = A.take(N * 8), o_sums = A.take((uint64_t)COMMON_MAX_FILES * 8);
    rc = arena_reserve_keep(c, &A, keep, st);
    if (rc != BSK_OK) return rc;
    const uint32_t* first = A.at<uint32_t>(o_first);
    uint64_t* d_masks = A.at<uint64_t>(o_masks);
    uint64_t* d_sums = A.at<uint64_t>(o_sums);
    uint64_t* d_kept = c->d_fin + bsk_ctx::FIN_AUX0;
    HIP_TRYX(c, hipMemsetAsync(d_kept, 0, sizeof(uint64_t), st));
    HIP_TRYX(c, hipMemsetAsync(d_masks, 0, N * 8, st));
    HIP_TRYX(c, hipMemcpyAsync(d_sums, B.file_sums.data(), (size_t)nf * 8, hipMemcpyHostToDevice, st));
    {
        Timed t(c, "k_comb_verify", st);
        HIP_TRYX(c, launch_comb_verify(B.d_acc, B.d_off, B.d_len, B.d_draw, first, N, d_sums, nf, d_masks, c->d_xflag, (uint32_t)RDB_FLAG_MAX, st));
    }
    {
        Timed t(c, "k_comb_decide", st);
        HIP_TRYX(c, launch_comb_decide(first, B.d_draw, d_masks, N, full, B.file_sums[0], B.d_bits, d_kept, st));
    }
    rc = rdb_flagged_read(c, st, n_kept, n_flagged);  // (the synchronisation also ends the copy out of file_sums)
    if (rc != BSK_OK) return rc;
    rc = rdb_flagged_settle(c, *n_flagged, "comb_settle_flagged", st, n_kept,
                            [&](bsk_ctx*, uint32_t m, hipStream_t, uint64_t* more) { return comb_settle_flagged(c, m, full, st, more); });
    if (rc != BSK_OK) return rc;
    HIP_TRYX(c, hipStreamSynchronize(st));  // (the arena is the next call's)
    return BSK_OK;
}

int common_bucket_finish(bsk_ctx* c, hipStream_t st, uint64_t* n_kept, uint64_t* n_flagged) {
    return rdb_bucket_finish(c, st, n_kept, n_flagged, comb_bucket_decide);
}

// ---- the emit pass: the kept records of a shard of the first file, in order, each as common_run_device prints a record
int common_emit_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st, bsk_out* out) {
    const bsk_ctx::RmDupBuckets& B = c->rdb;
    c->last_kernel_flags = 0;
    int rc = rdb_emit_ready(c);
    if (rc != BSK_OK) return rc;
    if (slices_wanted(c)) {
        c->set_error("libbsk: bsk_common_emit_run: out=slices is not available on the common path in buckets of the key");
        return BSK_ERR_UNSUPPORTED;
    }
    const bool fastq = format == BSK_FORMAT_FASTQ;
    rc = index_shard_status(c, d_buf, n, format, st);
    if (rc != BSK_OK) return rc;
    const uint64_t N = c->table.n, n0 = B.file_sums[0];
    if (first_record > n0 || N > n0 - first_record) {
        c->set_error("libbsk: bsk_common_emit_run: the shard's records " + std::to_string(first_record) + " .. " + std::to_string(first_record + N) +
                     " reach past the file_records[0] = " + std::to_string(n0) + " of bsk_common_verdict_begin (the emit runs over the first file)");
        return BSK_ERR_INVALID_ARG;
    }
    if (N == 0) return empty_result(c, out);
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
        Timed tm(c, "k_comb_apply", st);
        HIP_TRYX(c, launch_comb_apply(B.d_bits, first_record, N, c->d_out_len, st));
    }
    uint64_t total = 0, kept = 0;
    rc = finish_sizes(c, st, &total, &kept);
    if (rc != BSK_OK) return rc;
    out->d_data = nullptr;
    out->len = 0;
    out->records = 0;
    if (total == 0) return BSK_OK;
    return rdb_emit_tail(c, d_buf, n, &F, total, kept, st, out);
}

}  // namespace bsk
