// Host side of `rename` in buckets of the key (include/bsk.h; PARITY.md RENB): the verdict -- one ordinal per record of the
// whole input --, the finish of a bucket and the emit pass.  The histogram, the begin and the add of a bucket and the key
// grouping down to first[] are those of `rmdup` in buckets of the key (ops_host_rmdupbuckets.cpp: rdb_hist_device,
// rdb_bucket_begin, rdb_bucket_add, rdb_group_keys), on the same state c->rdb; the kernels of what a bucket decides are in
// ops_rename_buckets.hip, the ordinals of the members come from ops_group.hpp, and the emit ends with the tail of
// rename_run_device (rename_emit).  The verdict opens with rdb_verdict_open (on d_ord), the finish is rdb_bucket_finish around
// renb_bucket_decide, whose middle is rdb_flagged_read / rdb_flagged_settle with the kernels of the members between them.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/bsk.h"
#include "ctx.hpp"
#include "ops_group.hpp"
#include "ops_host.hpp"
#include "ops_host_internal.hpp"
#include "ops_rename_buckets.hpp"
#include "ops_rmdup.hpp"

namespace bsk {

// ---- the verdict
int rename_verdict_begin(bsk_ctx* c, uint64_t total_records) {
    bsk_ctx::RmDupBuckets& B = c->rdb;
    int rc = bucket_require_closed(c, B, "rename", "verdict_begin");
    if (rc != BSK_OK) return rc;
    rc = rdb_verdict_open(c, &B.d_ord, &B.ord_cap, total_records + 1, {total_records});
    if (rc != BSK_OK) return rc;
    B.renamed = 0;
    return BSK_OK;
}

int rename_verdict_get(bsk_ctx* c, uint64_t first, uint64_t count, uint32_t* ord) {
    const bsk_ctx::RmDupBuckets& B = c->rdb;
    if (!B.verdict) {
        c->set_error("libbsk: bsk_rename_verdict_get: no verdict (bsk_rename_verdict_begin first)");
        return BSK_ERR_INVALID_ARG;
    }
    if (first > B.total_records || count > B.total_records - first) {
        c->set_error("libbsk: bsk_rename_verdict_get: records " + std::to_string(first) + " .. reach past the " + std::to_string(B.total_records) +
                     " records of the verdict");
        return BSK_ERR_INVALID_ARG;
    }
    if (count == 0) return BSK_OK;
    HIP_TRYX(c, hipDeviceSynchronize());
    HIP_TRYX(c, hipMemcpy(ord, B.d_ord + first, count * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return BSK_OK;
}

// ---- one bucket
// The flagged records ranked on the host: inside every text the ordinals are 0, 1, 2, ... in ascending global index (a text
// other than the first text of its key group has ALL its records flagged, because they share k1); the non-zero ones are
// written by launch_renb_set.  *renamed = their number.
static int renb_settle_flagged(bsk_ctx* c, uint32_t m, hipStream_t st, uint64_t* renamed) {
    *renamed = 0;
    return rdb_flagged_texts(c, m, st, [&](const std::vector<uint32_t>& list, const std::vector<uint64_t>& gidx, const std::string& blob,
                                           const std::vector<uint64_t>& off) {
        std::unordered_map<std::string, uint32_t> seen;  // text -> its flagged records so far
        std::vector<uint64_t> g;
        std::vector<uint32_t> v;
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t k = seen[blob.substr(off[j], off[j + 1] - off[j])]++;
            if (k) {
                g.push_back(gidx[list[j]]);
                v.push_back(k);
            }
        }
        *renamed = g.size();
        if (g.empty()) return (int)BSK_OK;
        uint64_t* d_g = nullptr;
        uint32_t* d_v = nullptr;
        const bool ok = hipMalloc((void**)&d_g, g.size() * 8) == hipSuccess && hipMalloc((void**)&d_v, v.size() * 4) == hipSuccess &&
                        hipMemcpyAsync(d_g, g.data(), g.size() * 8, hipMemcpyHostToDevice, st) == hipSuccess &&
                        hipMemcpyAsync(d_v, v.data(), v.size() * 4, hipMemcpyHostToDevice, st) == hipSuccess &&
                        launch_renb_set(d_g, d_v, g.size(), c->rdb.d_ord, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
        for (void* p : {(void*)d_g, (void*)d_v}) if (p) hipFree(p);
        return ok ? (int)BSK_OK : (int)BSK_ERR_HIP;
    });
}

static int renb_bucket_decide(bsk_ctx* c, hipStream_t st, uint64_t* n_renamed, uint64_t* n_flagged) {
    bsk_ctx::RmDupBuckets& B = c->rdb;
    const uint64_t N = B.n;
    if (N == 0) return BSK_OK;
    Arena A;
    uint64_t o_first = 0;
    int rc = rdb_group_keys(c, st, &A, &o_first);
    if (rc != BSK_OK) return rc;
    // the member list, its sorted copy, the ordinals inside the bucket and the sort's storage, sized for N members: first[]
    // has to survive when the arena moves
    size_t tmp_bytes = 0;
    rc = sort_query(c, group_sort_temp_bytes(N, &tmp_bytes));
    if (rc != BSK_OK) return rc;
    const uint64_t keep = A.used;
    const uint64_t o_list = A.take(2 * N * 8), o_ord = A.take(N * 4), o_tmp = A.take(tmp_bytes ? tmp_bytes : 16);
    rc = arena_reserve_keep(c, &A, keep, st);
    if (rc != BSK_OK) return rc;
    const uint32_t* first = A.at<uint32_t>(o_first);
    uint64_t* d_list = A.at<uint64_t>(o_list);
    uint32_t* d_ord = A.at<uint32_t>(o_ord);
    uint64_t* d_members = c->d_fin + bsk_ctx::FIN_AUX0;
    HIP_TRYX(c, hipMemsetAsync(d_members, 0, sizeof(uint64_t), st));
    HIP_TRYX(c, hipMemsetAsync(d_ord, 0, N * 4, st));
    {
        Timed t(c, "k_renb_verify", st);
        HIP_TRYX(c, launch_renb_verify(B.d_acc, B.d_off, B.d_len, first, N, d_list, d_members, c->d_xflag, (uint32_t)RDB_FLAG_MAX, st));
    }
    rc = rdb_flagged_read(c, st, n_renamed, n_flagged);
    if (rc != BSK_OK) return rc;
    const uint64_t members = *n_renamed;
    if (members) {
        // the flagged records are not in the list: a member counts only the earlier records of its own text
        {
            Timed t(c, "renb_ordinals(sort+rank)", st);
            HIP_TRYX(c, launch_group_sort(A.at<uint8_t>(o_tmp), tmp_bytes, d_list, d_list + N, members, st, N));
            HIP_TRYX(c, launch_group_ordinals(d_list + N, members, d_ord, st));
        }
        Timed t(c, "k_renb_scatter", st);
        HIP_TRYX(c, launch_renb_scatter(d_ord, B.d_draw, N, B.d_ord, st));
    }
    rc = rdb_flagged_settle(c, *n_flagged, "renb_settle_flagged", st, n_renamed, renb_settle_flagged);
    if (rc != BSK_OK) return rc;
    HIP_TRYX(c, hipStreamSynchronize(st));  // (the arena is the next call's)
    return BSK_OK;
}

int rename_bucket_finish(bsk_ctx* c, hipStream_t st, uint64_t* n_renamed, uint64_t* n_flagged) {
    uint64_t renamed = 0;
    if (!n_renamed) n_renamed = &renamed;  // (wanted here either way: a refused finish still leaves the caller's word alone)
    const int rc = rdb_bucket_finish(c, st, n_renamed, n_flagged, renb_bucket_decide);
    if (rc == BSK_OK) c->rdb.renamed += *n_renamed;
    return rc;
}

// ---- the emit pass: the records of the shard, in order, each as `rename` prints a record with its ordinal
int rename_emit_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st, bsk_out* out) {
    const bsk_ctx::RmDupBuckets& B = c->rdb;
    c->last_kernel_flags = 0;
    int rc = rdb_emit_ready(c);
    if (rc != BSK_OK) return rc;
    rc = index_shard_status(c, d_buf, n, format, st);
    if (rc != BSK_OK) return rc;
    const uint64_t N = c->table.n;
    rc = rdb_emit_in_range(c, first_record, N);
    if (rc != BSK_OK) return rc;
    if (N == 0) return empty_result(c, out);
    rc = check_u32_records(c, "rename");
    if (rc != BSK_OK) return rc;
    TextTableH tt;
    rc = prepare_text(c, d_buf, format, st, &tt);
    if (rc != BSK_OK) return rc;
    rc = ensure_record_scratch(c);
    if (rc != BSK_OK) return rc;
    // one kernel over all records when a quarter of the input is renamed, as rename_run_device chooses for its shard: the
    // share of the whole input stands for the share of this shard, which nobody has counted
    return rename_emit(c, d_buf, n, format == BSK_FORMAT_FASTQ, tt, B.d_ord + first_record, B.renamed * 4 > B.total_records, st, out);
}

}  // namespace bsk
