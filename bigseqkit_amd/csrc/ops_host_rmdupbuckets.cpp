// Host side of `rmdup` in buckets of the key (include/bsk.h; PARITY.md RMDUPB): the histogram pass, the verdict bitmap, the
// collect pass of one bucket and its finish, and the emit pass.  The kernels are in ops_rmdup_buckets.hip; the keys are those of
// launch_rmdup_hash, the grouping of a bucket is launch_bucket_pass + launch_bucket_dedupe (ops_rmdup.hip), and the emit ends
// with the tail of rmdup_dist_emit.
// `rename` in buckets of the key (ops_host_renamebuckets.cpp; PARITY.md RENB) groups by the same subject under the same key: the
// steps down to first[] -- rdb_hist_device, rdb_bucket_begin, rdb_bucket_add, rdb_group_keys -- and rdb_flagged_texts serve both
// operators on c->rdb (declared in ops_host_internal.hpp); their messages name the operator of the context.  So do the steps
// around what a bucket decides, which this file owns for the whole family: rdb_verdict_open, rdb_bucket_finish,
// rdb_flagged_read / rdb_flagged_settle, rdb_verdict_bits and rdb_emit_tail (documented there as well).  `common` in buckets
// of the key (ops_host_commonbuckets.cpp; PARITY.md COMB) takes the same steps over the union of its files, and so does the
// match phase of `pair` in buckets of the key (ops_host_pairbuckets.cpp; PARITY.md PAIRB) over its two, and that of `concat` in
// buckets of the key (ops_host_concatbuckets.cpp; PARITY.md CONB).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/bsk.h"
#include "ctx.hpp"
#include "ops_host.hpp"
#include "ops_host_internal.hpp"
#include "ops_records.hpp"
#include "ops_rmdup.hpp"
#include "ops_rmdup_buckets.hpp"
#include "ops_seq.hpp"

namespace bsk {

// ---- what the histogram and the collect pass do first: the table of the shard and the complaints of the index pass
// (index_shard_status), the text view (-s on FASTA: every wrapped record flattened, as rmdup_run_device has it), the
// parameters and k1 of every record in c->d_keys -- whole: the bin comes from all 64 bits
struct RdbShard {
    TextTableH tt;
    RmDupParams P;
};
const char* rdb_op_name(const bsk_ctx* c) {
    return c->op == Op::Rename ? "rename" : c->op == Op::Common ? "common" : c->op == Op::Pair ? "pair" : c->op == Op::Concat ? "concat" : "rmdup";
}
static std::string rdb_fn(const bsk_ctx* c, const char* fn) { return std::string("bsk_") + rdb_op_name(c) + "_" + fn; }
RmDupParams rdb_params(bsk_ctx* c, const uint8_t* d_buf, size_t n, bool fastq) {
    const Options& o = c->opts;
    const bool rmdup = c->op == Op::RmDup || c->op == Op::Common;  // (common has rmdup's three options; rename: the ID, or the whole header with ByName, as it stands)
    RmDupParams P;
    memset(&P, 0, sizeof P);
    P.fastq = fastq;
    P.by_seq = rmdup && o.b("BySeq");
    // (pair and concat in buckets of the key, PARITY.md PAIRB / CONB: the ID, nothing else)
    P.by_name = c->op != Op::Pair && c->op != Op::Concat && o.b("ByName");
    P.ignore_case = rmdup && o.b("IgnoreCase");
    P.id_mode = id_mode_of(c);
    P.line_width = fastq ? 0 : (int)o.ci("LineWidth");
    P.buf_end = d_buf + n;
    return P;
}
static int rdb_index_shard(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, RdbShard* S) {
    const bool fastq = format == BSK_FORMAT_FASTQ;
    int rc = index_shard_status(c, d_buf, n, format, st);
    if (rc != BSK_OK || c->table.n == 0) return rc;
    S->P = rdb_params(c, d_buf, n, fastq);
    rc = prepare_text(c, d_buf, format, st, &S->tt, /*flatten=*/!fastq && S->P.by_seq, false, n);
    if (rc != BSK_OK) return rc;
    const uint64_t N = c->table.n;
    rc = ensure_record_scratch(c);
    if (rc != BSK_OK) return rc;
    rc = grow(c, &c->d_keys, &c->keys_cap, N, N / 8 + 16);
    if (rc != BSK_OK) return rc;
    if (!fastq && S->P.by_seq && c->flat_long_count) S->P.hash_long_min = c->flat_long_thresh;  // (listed by prepare_text just above)
    Timed t(c, "k_rmdup_hash", st);
    HIP_TRYX(c, launch_rmdup_hash(d_buf, n, c->table, S->tt, S->P, c->d_keys, nullptr, st));
    HIP_TRYX(c, launch_rmdup_hash_long(d_buf, n, c->table, S->tt, S->P, c->d_keys, nullptr, c->d_long_list, c->flat_long_count, st));
    return BSK_OK;
}

// ---- the histogram pass
int rmdup_hist_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, uint64_t* n_records) {
    c->last_kernel_flags = 0;
    if (!c->opts.s("DupSeqsFile").empty() || !c->opts.s("DupNumFile").empty()) {
        c->set_error("libbsk: -d / -D side files are not available on the rmdup path in buckets of the key");
        return BSK_ERR_UNSUPPORTED;
    }
    return rdb_hist_device(c, d_buf, n, format, st, n_records);
}
int rdb_hist_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, uint64_t* n_records) {
    c->last_kernel_flags = 0;
    int rc = bucket_hist_alloc(c, &c->rdb, st);
    if (rc != BSK_OK) return rc;
    RdbShard S;
    rc = rdb_index_shard(c, d_buf, n, format, st, &S);  // (the counters accumulate: the complaints of the index pass come first)
    if (rc != BSK_OK) return rc;
    if (n_records) *n_records = c->table.n;
    if (c->table.n == 0) return BSK_OK;
    Timed tm(c, "k_rdb_hist", st);
    HIP_TRYX(c, launch_rdb_hist(d_buf, c->table, S.tt, S.P, c->d_keys, c->rdb.d_hist, c->rdb.d_hist + BUCKET_BINS, c->num_cus, st));
    return BSK_OK;
}

// ---- the verdict
int rdb_verdict_open(bsk_ctx* c, uint32_t** d_arr, uint64_t* cap, uint64_t words, std::vector<uint64_t> file_sums) {
    bsk_ctx::RmDupBuckets& B = c->rdb;
    HIP_TRYX(c, hipDeviceSynchronize());
    const int rc = grow(c, d_arr, cap, words);
    if (rc != BSK_OK) return rc;
    HIP_TRYX(c, hipMemset(*d_arr, 0, words * sizeof(uint32_t)));
    B.total_records = file_sums.back();
    B.file_sums = std::move(file_sums);
    B.verdict = true;
    std::fill(B.decided.begin(), B.decided.end(), (uint8_t)0);
    return BSK_OK;
}

int rmdup_verdict_begin(bsk_ctx* c, uint64_t total_records) {
    bsk_ctx::RmDupBuckets& B = c->rdb;
    const int rc = bucket_require_closed(c, B, "rmdup", "verdict_begin");
    if (rc != BSK_OK) return rc;
    return rdb_verdict_open(c, &B.d_bits, &B.bits_words, (total_records + 31) / 32 + 1, {total_records});
}

int rdb_verdict_bits(bsk_ctx* c, const uint32_t* d_bits, uint64_t first, uint64_t count, uint8_t* bytes) {
    const uint64_t w0 = first >> 5, w1 = (first + count - 1) >> 5;
    std::vector<uint32_t> words(w1 - w0 + 1);
    HIP_TRYX(c, hipDeviceSynchronize());
    HIP_TRYX(c, hipMemcpy(words.data(), d_bits + w0, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (uint64_t j = 0; j < count; ++j) {
        const uint64_t g = first + j;
        bytes[j] = (uint8_t)((words[(g >> 5) - w0] >> (g & 31u)) & 1u);
    }
    return BSK_OK;
}

int rmdup_verdict_get(bsk_ctx* c, uint64_t first, uint64_t count, uint8_t* removed) {
    const bsk_ctx::RmDupBuckets& B = c->rdb;
    if (!B.verdict) {
        c->set_error("libbsk: bsk_rmdup_verdict_get: no verdict (bsk_rmdup_verdict_begin first)");
        return BSK_ERR_INVALID_ARG;
    }
    if (first > B.total_records || count > B.total_records - first) {
        c->set_error("libbsk: bsk_rmdup_verdict_get: records " + std::to_string(first) + " .. reach past the " + std::to_string(B.total_records) +
                     " records of the verdict");
        return BSK_ERR_INVALID_ARG;
    }
    if (count == 0) return BSK_OK;
    return rdb_verdict_bits(c, B.d_bits, first, count, removed);
}

// ---- one bucket
// the accumulation for `bytes` subject bytes and `recs` records, the keys among them
static int rdb_reserve(bsk_ctx* c, uint64_t bytes, uint64_t recs, hipStream_t st) {
    return bucket_acc_reserve(c, &c->rdb, bytes, recs, true, st, &c->rdb.d_key);
}

int rdb_bucket_begin(bsk_ctx* c, uint32_t lo_bin, uint32_t hi_bin) {
    // (an open bucket has a verdict, so the order of this refusal and the one of bucket_begin does not show)
    if (!c->rdb.verdict) {
        c->set_error("libbsk: " + rdb_fn(c, "bucket_begin") + ": no verdict to write to (" + rdb_fn(c, "verdict_begin") + " first)");
        return BSK_ERR_INVALID_ARG;
    }
    return bucket_begin(c, &c->rdb, rdb_op_name(c), lo_bin, hi_bin, [&](uint64_t bytes, uint64_t recs) {
        return rdb_reserve(c, bytes - recs * RMDUP_BUCKET_RECORD_BYTES, recs, nullptr);  // (the histogram counts the per-record arrays in)
    });
}

static int rdb_bucket_add_open(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st) {
    bsk_ctx::RmDupBuckets& B = c->rdb;
    c->last_kernel_flags = 0;
    // the survivor of a group is its lowest accumulated index because the accumulation receives its records in input order
    int rc = bucket_in_order(c, B, rdb_op_name(c), first_record);
    if (rc != BSK_OK) return rc;
    RdbShard S;
    rc = rdb_index_shard(c, d_buf, n, format, st, &S);
    if (rc != BSK_OK) return rc;
    const uint64_t N = c->table.n;
    if (first_record > B.total_records || N > B.total_records - first_record) {
        c->set_error("libbsk: " + rdb_fn(c, "bucket_add") + ": the shard's records " + std::to_string(first_record) + " .. " +
                     std::to_string(first_record + N) + " reach past the total_records = " + std::to_string(B.total_records) + " of " +
                     rdb_fn(c, "verdict_begin"));
        return BSK_ERR_INVALID_ARG;
    }
    if (N == 0) return BSK_OK;
    Arena A;
    const uint64_t o_keep = A.take(N * 4), o_koff = A.take((N + 1) * 8);
    rc = arena_reserve(c, &A);
    if (rc != BSK_OK) return rc;
    rc = grow(c, &c->d_long_list, &c->long_list_cap, N, N / 8 + 16);
    if (rc != BSK_OK) return rc;
    uint32_t* keep = A.at<uint32_t>(o_keep);
    uint64_t* keep_off = A.at<uint64_t>(o_koff);
    uint64_t total = 0, kept = 0;
    {
        Timed tm(c, "k_rdb_pick", st);
        HIP_TRYX(c, launch_rdb_pick(d_buf, c->table, S.tt, S.P, c->d_keys, B.lo, B.hi, c->d_out_len, keep, st));
    }
    HIP_TRYX(c, launch_scan_u32(c->d_out_len, c->d_out_off, N, c->d_scan_tmp, st));
    HIP_TRYX(c, launch_scan_u32(keep, keep_off, N, c->d_scan_tmp, st));
    HIP_TRYX(c, hipMemsetAsync(c->d_counter, 0, 4 * sizeof(uint64_t), st));
    HIP_TRYX(c, launch_find_long(c->d_out_len, N, RMDUP_PACK_LONG, c->d_long_list, c->d_counter + 2, st));
    HIP_TRYX(c, hipMemcpyAsync(&total, c->d_out_off + N, sizeof total, hipMemcpyDeviceToHost, st));
    HIP_TRYX(c, hipMemcpyAsync(&kept, keep_off + N, sizeof kept, hipMemcpyDeviceToHost, st));
    rc = ctl_readback(c, st);
    if (rc != BSK_OK) return rc;
    rc = kernel_error_to_status(c, c->status_word());
    if (rc != BSK_OK) return rc;
    const uint64_t long_count = c->h_ctl[8 + 2];  // (d_counter is d_ctl[8 ..])
    if (kept) {
        if (B.n + kept >= (1ull << 32)) return bucket_too_many(c, rdb_op_name(c));
        rc = rdb_reserve(c, B.acc_used + total, B.n + kept, st);
        if (rc != BSK_OK) return rc;
        Timed tm(c, "k_rdb_pack", st);
        HIP_TRYX(c, launch_rdb_pack(d_buf, c->table, S.tt, S.P, c->d_keys, c->d_out_len, c->d_out_off, keep, keep_off, first_record, B.n,
                                    B.acc_used, B.d_acc, B.d_key, B.d_draw, B.d_off, B.d_len, st));
        HIP_TRYX(c, launch_rdb_pack_long(d_buf, c->table, S.tt, S.P, c->d_out_len, c->d_out_off, B.acc_used, B.d_acc, c->d_long_list,
                                         long_count, st));
        HIP_TRYX(c, hipStreamSynchronize(st));  // (the shard may be a staging buffer that the next call overwrites)
        B.acc_used += total;
        B.total += total;
        B.n += kept;
    }
    B.next_first = first_record + N;
    return BSK_OK;
}

int rdb_bucket_add(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st) {
    const int rc = bucket_require_open(c, c->rdb, rdb_op_name(c), "add");
    if (rc != BSK_OK) return rc;
    return rdb_bucket_add_open(c, d_buf, n, format, first_record, st);  // (no close on an error here: see sort_bucket_add)
}

// The flagged records -- accumulated indices whose subject differs from that of the record their key group names -- on their
// way to the host, where they are settled exactly, as PARITY KEYS (b) does: the m entries of c->d_xflag in ascending accumulated
// order (which is input order), the global index of every accumulated record, and the subject of flagged record list[j] =
// blob[off[j], off[j + 1]).  All records of one text share k1, hence the group, hence the flag: settle() groups them by TEXT.
int rdb_flagged_texts(bsk_ctx* c, uint32_t m, hipStream_t st, const RdbSettle& settle) {
    bsk_ctx::RmDupBuckets& B = c->rdb;
    std::vector<uint32_t> list(m);
    HIP_TRYX(c, hipMemcpy(list.data(), c->d_xflag + 1, (size_t)m * 4, hipMemcpyDeviceToHost));
    std::sort(list.begin(), list.end());  // (accumulated order is input order)
    std::vector<uint32_t> len(B.n);
    std::vector<uint64_t> gidx(B.n);
    HIP_TRYX(c, hipMemcpy(len.data(), B.d_len, B.n * 4, hipMemcpyDeviceToHost));
    HIP_TRYX(c, hipMemcpy(gidx.data(), B.d_draw, B.n * 8, hipMemcpyDeviceToHost));
    std::vector<uint64_t> off(m + 1, 0);
    for (uint32_t j = 0; j < m; ++j) off[j + 1] = off[j] + len[list[j]];
    std::string blob(off[m], '\0');
    uint32_t* d_list = nullptr;
    uint64_t* d_off = nullptr;
    uint8_t* d_blob = nullptr;
    int rc = BSK_OK;
    if (hipMalloc((void**)&d_list, (size_t)m * 4) != hipSuccess || hipMalloc((void**)&d_off, (size_t)(m + 1) * 8) != hipSuccess ||
        hipMalloc((void**)&d_blob, std::max<uint64_t>(off[m], 1)) != hipSuccess ||
        hipMemcpyAsync(d_list, list.data(), (size_t)m * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(d_off, off.data(), (size_t)(m + 1) * 8, hipMemcpyHostToDevice, st) != hipSuccess ||
        launch_rdb_gather(B.d_acc, B.d_off, B.d_len, d_list, d_off, m, d_blob, st) != hipSuccess ||
        (off[m] && hipMemcpyAsync(&blob[0], d_blob, off[m], hipMemcpyDeviceToHost, st) != hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess)
        rc = BSK_ERR_HIP;
    for (void* p : {(void*)d_list, (void*)d_off, (void*)d_blob}) if (p) hipFree(p);
    if (rc == BSK_OK) rc = settle(list, gidx, blob, off);
    if (rc == BSK_ERR_HIP)
        c->set_error(std::string("libbsk: ") + rdb_op_name(c) + ": settling the records that differ from their key group failed on the device");
    return rc;
}

// rmdup: the lowest global index of every text survives, the others get their bit.  *losers = their number.
static int rdb_settle_flagged(bsk_ctx* c, uint32_t m, hipStream_t st, uint64_t* losers) {
    *losers = 0;
    return rdb_flagged_texts(c, m, st, [&](const std::vector<uint32_t>& list, const std::vector<uint64_t>& gidx, const std::string& blob,
                                           const std::vector<uint64_t>& off) {
        std::unordered_map<std::string, uint32_t> seen;  // text -> its first flagged record
        std::vector<uint64_t> lose;
        for (uint32_t j = 0; j < m; ++j)
            if (!seen.emplace(blob.substr(off[j], off[j + 1] - off[j]), list[j]).second) lose.push_back(gidx[list[j]]);
        *losers = lose.size();
        if (lose.empty()) return (int)BSK_OK;
        uint64_t* d_lose = nullptr;
        const bool ok = hipMalloc((void**)&d_lose, lose.size() * 8) == hipSuccess &&
                        hipMemcpyAsync(d_lose, lose.data(), lose.size() * 8, hipMemcpyHostToDevice, st) == hipSuccess &&
                        launch_rdb_mark(d_lose, lose.size(), c->rdb.d_bits, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
        if (d_lose) hipFree(d_lose);
        return ok ? (int)BSK_OK : (int)BSK_ERR_HIP;
    });
}

// The key grouping of the open bucket (B.n > 0 records): first[i] = the lowest accumulated index that shares the key of
// record i -- the radix-bucket pass on the accumulated keys, or the one big table in HBM.  first[] lies at *o_first of the
// arena *A, which is carved and reserved here; a caller that takes more of it afterwards keeps A->used bytes
// (arena_reserve_keep) and derives the pointer again.  c->d_xflag holds RDB_FLAG_MAX + 1 words afterwards, the first one zeroed.
int rdb_group_keys(bsk_ctx* c, hipStream_t st, Arena* Ap, uint64_t* o_first_out) {
    bsk_ctx::RmDupBuckets& B = c->rdb;
    const uint64_t N = B.n;
    Arena& A = *Ap;
    uint32_t k1_bits = 64;
    if (const char* e = c->tune.get("rmdup_k1_bits"))  // tests: only the low bits of k1 group (different subjects under one key)
        if (atoi(e) >= 16 && atoi(e) < 64) k1_bits = (uint32_t)atoi(e);
    const uint32_t nb = 1u << RMDUP_BUCKET_BITS;
    const uint64_t o_kc = A.take(N * 8), o_sk = A.take(N * 8), o_vo = A.take(N * 4), o_first = A.take(N * 4), o_bs = A.take((nb + 2) * 4),
                   o_hist = A.take(nb * 4), o_has = A.take(N);
    int rc = arena_reserve(c, &A);
    if (rc != BSK_OK) return rc;
    uint64_t* kc = A.at<uint64_t>(o_kc);
    uint32_t* first = A.at<uint32_t>(o_first);
    HIP_TRYX(c, hipMemcpyAsync(kc, B.d_key, N * 8, hipMemcpyDeviceToDevice, st));
    if (k1_bits < 64) HIP_TRYX(c, launch_mask_keys(kc, N, (1ull << k1_bits) - 1ull, st));
    {
        Timed t(c, "rmdup_group(sort+dedupe)", st);
        HIP_TRYX(c, launch_bucket_pass(kc, N, A.at<uint32_t>(o_hist), A.at<uint32_t>(o_bs), first, A.at<uint64_t>(o_sk), A.at<uint32_t>(o_vo), st));
        HIP_TRYX(c, launch_bucket_dedupe(A.at<uint64_t>(o_sk), A.at<uint32_t>(o_vo), N, A.at<uint32_t>(o_bs), first, c->d_status, st, nullptr,
                                         nullptr, 0, true));
    }
    rc = ctl_readback(c, st);
    if (rc != BSK_OK) return rc;
    uint64_t status = c->status_word();
    if (status & ERR_BUCKET_OVERFLOW) {
        // a radix bucket with too many distinct keys for its LDS table: the one big table in HBM, as rmdup_run_device falls back
        rc = clear_status_bits(c, &status, ERR_BUCKET_OVERFLOW, st);
        if (rc != BSK_OK) return rc;
        if (k1_bits < 64) {
            c->set_error("libbsk: BSK_RMDUP_K1_BITS is a test switch of the key path; the table path needs whole keys");
            return BSK_ERR_INVALID_ARG;
        }
        uint64_t cap = 0;
        uint64_t* tk = nullptr;
        rc = key_table(c, N, &cap, &tk, st);
        if (rc != BSK_OK) return rc;
        HIP_TRYX(c, hipMemsetAsync(A.at<uint8_t>(o_has), 0, N, st));
        HIP_TRYX(c, launch_rmdup_insert(kc, N, 0, tk, cap, st));
        HIP_TRYX(c, launch_rmdup_group(N, kc, tk, cap, A.at<uint8_t>(o_has), st));
        HIP_TRYX(c, launch_rdb_narrow(kc, N, first, st));
    }
    rc = kernel_error_to_status(c, status);
    if (rc != BSK_OK) return rc;
    rc = grow(c, &c->d_xflag, &c->xflag_cap, RDB_FLAG_MAX + 1);
    if (rc != BSK_OK) return rc;
    HIP_TRYX(c, hipMemsetAsync(c->d_xflag, 0, sizeof(uint32_t), st));
    *o_first_out = o_first;
    return BSK_OK;
}

int rdb_too_many_flagged(bsk_ctx* c) {
    c->set_error(std::string("libbsk: ") + rdb_op_name(c) + ": more than 2^20 records of one bucket differ from the survivor of their key group; refusing (keys that collide that often are no keys)");
    return BSK_ERR_UNSUPPORTED;
}

static int rdb_bucket_decide(bsk_ctx* c, hipStream_t st, uint64_t* n_removed, uint64_t* n_flagged) {
    bsk_ctx::RmDupBuckets& B = c->rdb;
    const uint64_t N = B.n;
    if (N == 0) return BSK_OK;
    Arena A;
    uint64_t o_first = 0;
    int rc = rdb_group_keys(c, st, &A, &o_first);
    if (rc != BSK_OK) return rc;
    const uint32_t* first = A.at<uint32_t>(o_first);
    uint64_t* d_removed = c->d_fin + bsk_ctx::FIN_AUX0;
    HIP_TRYX(c, hipMemsetAsync(d_removed, 0, sizeof(uint64_t), st));
    {
        Timed t(c, "k_rdb_verify", st);
        HIP_TRYX(c, launch_rdb_verify(B.d_acc, B.d_off, B.d_len, B.d_draw, first, N, B.d_bits, c->d_xflag, (uint32_t)RDB_FLAG_MAX, d_removed, st));
    }
    rc = rdb_flagged_read(c, st, n_removed, n_flagged);
    if (rc != BSK_OK) return rc;
    return rdb_flagged_settle(c, *n_flagged, "rdb_settle_flagged", st, n_removed, rdb_settle_flagged);  // (no synchronisation behind it)
}

int rdb_flagged_read(bsk_ctx* c, hipStream_t st, uint64_t* counted, uint64_t* n_flagged) {
    uint32_t m = 0;
    HIP_TRYX(c, hipMemcpyAsync(&m, c->d_xflag, sizeof m, hipMemcpyDeviceToHost, st));
    const int rc = ctl_readback(c, st);
    if (rc != BSK_OK) return rc;
    *counted = c->fin(bsk_ctx::FIN_AUX0);
    *n_flagged = m;
    return m > RDB_FLAG_MAX ? rdb_too_many_flagged(c) : (int)BSK_OK;
}

int rdb_bucket_finish(bsk_ctx* c, hipStream_t st, uint64_t* n_counted, uint64_t* n_flagged, RdbDecide decide) {
    bsk_ctx::RmDupBuckets& B = c->rdb;
    int rc = bucket_require_open(c, B, rdb_op_name(c), "finish");
    if (rc != BSK_OK) return rc;
    uint64_t counted = 0, flagged = 0;
    rc = decide(c, st, &counted, &flagged);
    if (n_counted) *n_counted = counted;
    if (n_flagged) *n_flagged = flagged;
    if (rc == BSK_OK)
        for (uint32_t b = B.lo; b < B.hi; ++b) B.decided[b] = 1;
    bucket_close(&B);
    return rc;
}

int rmdup_bucket_finish(bsk_ctx* c, hipStream_t st, uint64_t* n_removed, uint64_t* n_flagged) {
    return rdb_bucket_finish(c, st, n_removed, n_flagged, rdb_bucket_decide);
}

// ---- the emit pass: the survivors of the shard, in order, each as Format(LineWidth)
// the refusals of an emit pass: no verdict, an undecided bin (the first is named) / a shard that reaches past the verdict
int rdb_emit_ready(bsk_ctx* c) {
    const bsk_ctx::RmDupBuckets& B = c->rdb;
    if (!B.verdict) {
        c->set_error("libbsk: " + rdb_fn(c, "emit_run") + ": no verdict (" + rdb_fn(c, "verdict_begin") + " and the buckets first)");
        return BSK_ERR_INVALID_ARG;
    }
    for (uint32_t b = 0; b < BUCKET_BINS; ++b)
        if (!B.decided[b]) {
            c->set_error("libbsk: " + rdb_fn(c, "emit_run") + ": fine bin " + std::to_string(b) + " has not been decided (every bin belongs to a bucket that "
                         "was finished since " + rdb_fn(c, "verdict_begin") + ")");
            return BSK_ERR_INVALID_ARG;
        }
    return BSK_OK;
}
int rdb_emit_in_range(bsk_ctx* c, uint64_t first_record, uint64_t N) {
    const bsk_ctx::RmDupBuckets& B = c->rdb;
    if (first_record > B.total_records || N > B.total_records - first_record) {
        c->set_error("libbsk: " + rdb_fn(c, "emit_run") + ": the shard's records " + std::to_string(first_record) + " .. " + std::to_string(first_record + N) +
                     " reach past the total_records = " + std::to_string(B.total_records) + " of " + rdb_fn(c, "verdict_begin"));
        return BSK_ERR_INVALID_ARG;
    }
    return BSK_OK;
}

int rmdup_emit_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st, bsk_out* out) {
    const bsk_ctx::RmDupBuckets& B = c->rdb;
    c->last_kernel_flags = 0;
    int rc = rdb_emit_ready(c);
    if (rc != BSK_OK) return rc;
    if (slices_wanted(c)) {
        c->set_error("libbsk: bsk_rmdup_emit_run: out=slices is not available on the rmdup path in buckets of the key");
        return BSK_ERR_UNSUPPORTED;
    }
    const bool fastq = format == BSK_FORMAT_FASTQ;
    rc = index_shard_status(c, d_buf, n, format, st);
    if (rc != BSK_OK) return rc;
    const uint64_t N = c->table.n;
    rc = rdb_emit_in_range(c, first_record, N);
    if (rc != BSK_OK) return rc;
    if (N == 0) return empty_result(c, out);
    TextTableH tt;
    rc = prepare_text(c, d_buf, format, st, &tt);
    if (rc != BSK_OK) return rc;
    rc = ensure_record_scratch(c);
    if (rc != BSK_OK) return rc;
    {
        Timed tm(c, "k_rdb_apply", st);
        HIP_TRYX(c, launch_rdb_apply(c->table, rdb_params(c, d_buf, n, fastq), B.d_bits, first_record, c->d_out_len, st));
    }
    uint64_t total = 0, kept = 0;
    rc = finish_sizes(c, st, &total, &kept);
    if (rc != BSK_OK) return rc;
    SeqParams F = format_params(c, fastq);
    F.text_w = tt.text_w; F.lin_off = tt.lin_off; F.lin = tt.lin;
    return rdb_emit_tail(c, d_buf, n, &F, total, kept, st, out);
}

int rdb_emit_tail(bsk_ctx* c, const uint8_t* d_buf, size_t n, SeqParams* F, uint64_t total, uint64_t kept, hipStream_t st, bsk_out* out) {
    int rc = ensure_out(c, total);
    if (rc != BSK_OK) return rc;
    apply_long(c, F);
    rc = emit_records(c, d_buf, n, *F, total, kept, st);
    if (rc != BSK_OK) return rc;
    out->d_data = c->d_out;
    out->len = total;
    out->records = kept;
    return BSK_OK;
}

}  // namespace bsk
