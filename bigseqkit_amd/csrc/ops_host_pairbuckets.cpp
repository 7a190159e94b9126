// Host side of `pair` in buckets of the key (include/bsk.h; PARITY.md PAIRB).  Two bucket phases over file 1 followed by file 2:
//   match   in buckets of the key, on c->rdb with the steps of `rmdup` in buckets of the key (ops_host_rmdupbuckets.cpp:
//           rdb_hist_device, rdb_bucket_begin, rdb_bucket_add, rdb_group_keys, rdb_flagged_texts).  A bucket ends in its share of
//           the verdict: the PAIRED bits of both files and, per paired record of file 2, the global index of its mate.  The
//           classification of a key group is launch_pair_classify, as in pair_run_device: a bucket receives file 1 before file 2,
//           so the boundary inside a group's run is the accumulated index of the bucket's first record of file 2
//   rank    once: every mate word becomes `pos`, the output position; P and "file 2 is in mate order" are reduced
//   order   in buckets of pos, on c->pab.order with the steps of the shuffle kind (bucket_hist_alloc, bucket_begin,
//           BucketAccumulate): a bucket prints its run of paired.2.  Not needed when file 2 is in mate order: the emit pass
//           prints paired.2 then, as a filter of file 2
// The emit pass filters a shard of either file by the bits, as pair_run_device prints its outputs 0, 2 and 3.  The kernels
// are in ops_pair_buckets.hip.  The verdict of the match phase opens with rdb_verdict_open (both bitmaps in one array), a match
// bucket finishes in rdb_bucket_finish around pairb_bucket_decide, which reads the control words twice: rdb_flagged_read for the
// members and the flagged records, and once more behind the scatter for its pairs.
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
#include "ops_pair_buckets.hpp"
#include "ops_records.hpp"
#include "ops_seq.hpp"

namespace bsk {

static int pairb_fail(bsk_ctx* c, const char* fn, const std::string& what) {
    c->set_error(std::string("libbsk: bsk_pair_") + fn + ": " + what);
    return BSK_ERR_INVALID_ARG;
}
static int pairb_require_ranked(bsk_ctx* c, const char* fn) {
    if (c->pab.ranked) return BSK_OK;
    return pairb_fail(c, fn, "the verdict has no positions yet (bsk_pair_order_begin first)");
}
// the records first_record .. first_record + N of a shard: inside the union, and inside ONE file
static int pairb_shard_range(bsk_ctx* c, const char* fn, uint64_t first_record, uint64_t N) {
    const uint64_t n1 = c->rdb.file_sums[0], total = c->rdb.total_records;
    if (first_record > total || N > total - first_record)
        return pairb_fail(c, fn, "the shard's records " + std::to_string(first_record) + " .. " + std::to_string(first_record + N) +
                                     " reach past the sum of file_records = " + std::to_string(total) + " of bsk_pair_verdict_begin");
    if (first_record < n1 && N > n1 - first_record)
        return pairb_fail(c, fn, "the shard's records " + std::to_string(first_record) + " .. " + std::to_string(first_record + N) +
                                     " straddle the two files (file 1 ends at record " + std::to_string(n1) + "; a shard belongs to one file)");
    return BSK_OK;
}

// ---- the verdict
int pair_verdict_begin(bsk_ctx* c, const uint64_t* file_records) {
    bsk_ctx::RmDupBuckets& B = c->rdb;
    bsk_ctx::PairBuckets& P = c->pab;
    int rc = bucket_require_closed(c, B, "pair", "verdict_begin");
    if (rc == BSK_OK) rc = bucket_require_closed(c, P.order, "pair_order", "verdict_begin");
    if (rc != BSK_OK) return rc;
    const uint64_t n1 = file_records[0], n2 = file_records[1];
    if (n2 > ~n1) return pairb_fail(c, "verdict_begin", "the sum of file_records does not fit 64 bits");
    const uint64_t words1 = (n1 + 31) / 32 + 1, words2 = (n2 + 31) / 32 + 1, words = words1 + words2;
    rc = rdb_verdict_open(c, &B.d_bits, &B.bits_words, words, {n1, n1 + n2});
    if (rc != BSK_OK) return rc;
    rc = grow(c, &P.d_mates, &P.mates_cap, n2);
    if (rc != BSK_OK) {
        B.verdict = false;  // (rdb_verdict_open has put one in place: without its mate words it must not be used)
        return rc;
    }
    P.d_bits2 = B.d_bits + words1;
    P.words1 = words1;
    P.words2 = words2;
    P.ranked = false;
    P.in_mate_order = false;
    P.pairs = 0;
    P.shift = 0;
    P.first2 = ~0ull;
    return BSK_OK;
}

int pair_verdict_get(bsk_ctx* c, uint64_t first, uint64_t count, uint64_t* pos) {
    const bsk_ctx::RmDupBuckets& B = c->rdb;
    const bsk_ctx::PairBuckets& P = c->pab;
    if (!B.verdict) return pairb_fail(c, "verdict_get", "no verdict (bsk_pair_verdict_begin first)");
    const int rc = pairb_require_ranked(c, "verdict_get");
    if (rc != BSK_OK) return rc;
    if (first > B.total_records || count > B.total_records - first)
        return pairb_fail(c, "verdict_get", "records " + std::to_string(first) + " .. reach past the " + std::to_string(B.total_records) +
                                                " records of the verdict");
    if (count == 0) return BSK_OK;
    uint64_t* d_pos = nullptr;
    HIP_TRYX(c, hipDeviceSynchronize());
    HIP_TRYX(c, hipMalloc((void**)&d_pos, count * 8));
    const bool ok = launch_pairb_pos(first, count, B.file_sums[0], B.d_bits, P.d_wpre, P.d_base, P.d_bits2, P.d_mates, d_pos, nullptr) == hipSuccess &&
                    hipMemcpy(pos, d_pos, count * 8, hipMemcpyDeviceToHost) == hipSuccess;
    hipFree(d_pos);
    if (!ok) {
        c->set_error("libbsk: bsk_pair_verdict_get: reading the positions failed on the device");
        return BSK_ERR_HIP;
    }
    return BSK_OK;
}

// ---- the match phase: one bucket
int pair_bucket_begin(bsk_ctx* c, uint32_t lo_bin, uint32_t hi_bin) {
    if (c->rdb.verdict && c->pab.ranked)
        return pairb_fail(c, "bucket_begin", "the verdict has its positions already (bsk_pair_verdict_begin starts a new one)");
    const int rc = rdb_bucket_begin(c, lo_bin, hi_bin);
    if (rc == BSK_OK) c->pab.first2 = ~0ull;
    return rc;
}

int pair_bucket_add(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st) {
    bsk_ctx::RmDupBuckets& B = c->rdb;
    int rc = bucket_require_open(c, B, "pair", "add");
    if (rc != BSK_OK) return rc;
    // (a wrapped FASTQ shard enters twice, and has added nothing the first time: the boundary is the same)
    if (first_record >= B.file_sums[0] && c->pab.first2 == ~0ull) c->pab.first2 = B.n;
    rc = rdb_bucket_add(c, d_buf, n, format, first_record, st);
    if (rc != BSK_OK) return rc;
    return pairb_shard_range(c, "bucket_add", first_record, c->table.n);
}

// The flagged records settled on the host: grouped by text -- a text other than the first text of its key group has ALL its
// records flagged, because they share k1 --, the records of a text split by file in ascending global index (the list is in
// input order), the k-th of file 1 paired with the k-th of file 2 (launch_pairb_set).  *pairs = their number.
static int pairb_settle_flagged(bsk_ctx* c, uint32_t m, hipStream_t st, uint64_t* pairs) {
    *pairs = 0;
    return rdb_flagged_texts(c, m, st, [&](const std::vector<uint32_t>& list, const std::vector<uint64_t>& gidx, const std::string& blob,
                                           const std::vector<uint64_t>& off) {
        const uint64_t n1 = c->rdb.file_sums[0];
        struct Sides { std::vector<uint64_t> f1, f2; };
        std::unordered_map<std::string, Sides> seen;
        for (uint32_t j = 0; j < m; ++j) {
            const uint64_t g = gidx[list[j]];
            Sides& s = seen[blob.substr(off[j], off[j + 1] - off[j])];
            (g < n1 ? s.f1 : s.f2).push_back(g);
        }
        std::vector<uint64_t> ab;  // the file-1 records, then their mates
        std::vector<uint64_t> b;
        for (const auto& kv : seen)
            for (size_t k = 0; k < std::min(kv.second.f1.size(), kv.second.f2.size()); ++k) {
                ab.push_back(kv.second.f1[k]);
                b.push_back(kv.second.f2[k]);
            }
        const size_t np = b.size();
        *pairs = np;
        if (np == 0) return (int)BSK_OK;
        ab.insert(ab.end(), b.begin(), b.end());
        uint64_t* d_ab = nullptr;
        const bool ok = hipMalloc((void**)&d_ab, ab.size() * 8) == hipSuccess &&
                        hipMemcpyAsync(d_ab, ab.data(), ab.size() * 8, hipMemcpyHostToDevice, st) == hipSuccess &&
                        launch_pairb_set(d_ab, d_ab + np, np, n1, c->rdb.d_bits, c->pab.d_bits2, c->pab.d_mates, st) == hipSuccess &&
                        hipStreamSynchronize(st) == hipSuccess;
        if (d_ab) hipFree(d_ab);
        return ok ? (int)BSK_OK : (int)BSK_ERR_HIP;
    });
}

static int pairb_bucket_decide(bsk_ctx* c, hipStream_t st, uint64_t* n_pairs, uint64_t* n_flagged) {
    bsk_ctx::RmDupBuckets& B = c->rdb;
    bsk_ctx::PairBuckets& P = c->pab;
    const uint64_t N = B.n;
    if (N == 0) return BSK_OK;
    Arena A;
    uint64_t o_first = 0;
    int rc = rdb_group_keys(c, st, &A, &o_first);
    if (rc != BSK_OK) return rc;
    // the member list, its sorted copy, what launch_pair_classify leaves per record and the sort's storage: first[] has to
    // survive when the arena moves
    size_t tmp_bytes = 0;
    rc = sort_query(c, group_sort_temp_bytes(N, &tmp_bytes));
    if (rc != BSK_OK) return rc;
    const uint64_t keep = A.used;
    const uint64_t o_list = A.take(2 * N * 8), o_state = A.take(N), o_partner = A.take(N * 4), o_tmp = A.take(tmp_bytes ? tmp_bytes : 16);
    rc = arena_reserve_keep(c, &A, keep, st);
    if (rc != BSK_OK) return rc;
    const uint32_t* first = A.at<uint32_t>(o_first);
    uint64_t* d_list = A.at<uint64_t>(o_list);
    uint8_t* d_state = A.at<uint8_t>(o_state);
    uint32_t* d_partner = A.at<uint32_t>(o_partner);
    uint64_t* d_members = c->d_fin + bsk_ctx::FIN_AUX0;
    uint64_t* d_pairs = c->d_fin + bsk_ctx::FIN_AUX1;
    HIP_TRYX(c, hipMemsetAsync(d_members, 0, 2 * sizeof(uint64_t), st));  // (FIN_AUX0, FIN_AUX1)
    HIP_TRYX(c, hipMemsetAsync(d_state, 0, N, st));
    {
        Timed t(c, "k_pairb_verify", st);
        HIP_TRYX(c, launch_pairb_verify(B.d_acc, B.d_off, B.d_len, first, N, d_list, d_members, c->d_xflag, (uint32_t)RDB_FLAG_MAX, st));
    }
    uint64_t members = 0;
    rc = rdb_flagged_read(c, st, &members, n_flagged);
    if (rc != BSK_OK) return rc;
    if (members) {
        // the flagged records are not in the list: a member meets only the records of its own text
        const uint64_t first2 = std::min<uint64_t>(P.first2, N);  // (no record of file 2 in the bucket: every member is of file 1)
        {
            Timed t(c, "pairb_classify(sort+classify)", st);
            HIP_TRYX(c, launch_group_sort(A.at<uint8_t>(o_tmp), tmp_bytes, d_list, d_list + N, members, st, N));
            HIP_TRYX(c, launch_pair_classify(d_list + N, members, (uint32_t)first2, d_state, d_partner, st));
        }
        Timed t(c, "k_pairb_scatter", st);
        HIP_TRYX(c, launch_pairb_scatter(d_state, d_partner, B.d_draw, N, B.file_sums[0], B.d_bits, P.d_bits2, P.d_mates, d_pairs, st));
    }
    rc = ctl_readback(c, st);  // (the control words a second time, for the pairs of the scatter; the arena is the next call's)
    if (rc != BSK_OK) return rc;
    *n_pairs = c->fin(bsk_ctx::FIN_AUX1);
    return rdb_flagged_settle(c, *n_flagged, "pairb_settle_flagged", st, n_pairs, pairb_settle_flagged);
}

int pair_bucket_finish(bsk_ctx* c, hipStream_t st, uint64_t* n_pairs, uint64_t* n_flagged) {
    return rdb_bucket_finish(c, st, n_pairs, n_flagged, pairb_bucket_decide);
}

// ---- the rank step
int pair_order_begin(bsk_ctx* c, hipStream_t st, uint64_t* n_pairs, int* in_mate_order) {
    bsk_ctx::RmDupBuckets& B = c->rdb;
    bsk_ctx::PairBuckets& P = c->pab;
    if (!B.verdict) return pairb_fail(c, "order_begin", "no verdict (bsk_pair_verdict_begin and the buckets first)");
    int rc = bucket_require_closed(c, B, "pair", "order_begin");
    if (rc != BSK_OK) return rc;
    for (uint32_t b = 0; b < BUCKET_BINS; ++b)
        if (!B.decided[b])
            return pairb_fail(c, "order_begin", "fine bin " + std::to_string(b) + " has not been decided (every bin belongs to a bucket that "
                                                    "was finished since bsk_pair_verdict_begin)");
    if (!P.ranked) {  // (a second call reports what the first one found: the mate words hold positions by now)
        rc = bucket_require_closed(c, P.order, "pair_order", "begin");
        if (rc != BSK_OK) return rc;
        const uint64_t n2 = B.file_sums[1] - B.file_sums[0];
        const uint64_t blocks1 = (P.words1 + PAIRB_RANK_WORDS - 1) / PAIRB_RANK_WORDS, blocks2 = (P.words2 + PAIRB_RANK_WORDS - 1) / PAIRB_RANK_WORDS;
        rc = grow(c, &P.d_wpre, &P.wpre_cap, P.words1 + P.words2);
        if (rc != BSK_OK) return rc;
        if (blocks1 + blocks2 > P.cnt_cap || !P.d_cnt || !P.d_base) {
            for (void* p : {(void*)P.d_cnt, (void*)P.d_base}) if (p) HIP_TRYX(c, hipFree(p));
            P.d_cnt = nullptr;
            P.d_base = nullptr;
            P.cnt_cap = 0;
            HIP_TRYX(c, hipMalloc((void**)&P.d_cnt, (blocks1 + blocks2) * sizeof(uint32_t)));
            HIP_TRYX(c, hipMalloc((void**)&P.d_base, (blocks1 + blocks2 + 2) * sizeof(uint64_t)));
            P.cnt_cap = blocks1 + blocks2;
        }
        rc = grow(c, &c->d_scan_tmp, &c->scan_tmp_cap, 3 * ((std::max(blocks1, blocks2) + 2047) / 2048) + 6, 16);
        if (rc != BSK_OK) return rc;
        uint16_t* wpre2 = P.d_wpre + P.words1;
        uint32_t* cnt2 = P.d_cnt + blocks1;
        uint64_t* base2 = P.d_base + blocks1 + 1;
        uint64_t* d_disorder = c->d_fin + bsk_ctx::FIN_AUX0;
        HIP_TRYX(c, hipMemsetAsync(d_disorder, 0, sizeof(uint64_t), st));
        {
            Timed t(c, "k_pairb_count", st);
            HIP_TRYX(c, launch_pairb_count(B.d_bits, P.words1, P.d_wpre, P.d_cnt, st));
            HIP_TRYX(c, launch_pairb_count(P.d_bits2, P.words2, wpre2, cnt2, st));
        }
        HIP_TRYX(c, launch_scan_u32(P.d_cnt, P.d_base, blocks1, c->d_scan_tmp, st));
        HIP_TRYX(c, launch_scan_u32(cnt2, base2, blocks2, c->d_scan_tmp, st));
        {
            Timed t(c, "k_pairb_rank", st);
            HIP_TRYX(c, launch_pairb_rank(B.d_bits, P.d_wpre, P.d_base, P.d_bits2, wpre2, base2, n2, P.d_mates, d_disorder, st));
        }
        uint64_t p1 = 0, p2 = 0;
        HIP_TRYX(c, hipMemcpyAsync(&p1, P.d_base + blocks1, sizeof p1, hipMemcpyDeviceToHost, st));
        HIP_TRYX(c, hipMemcpyAsync(&p2, base2 + blocks2, sizeof p2, hipMemcpyDeviceToHost, st));
        rc = ctl_readback(c, st);
        if (rc != BSK_OK) return rc;
        if (p1 != p2) {
            c->set_error("libbsk: bsk_pair_order_begin: " + std::to_string(p1) + " paired records in file 1, " + std::to_string(p2) +
                         " in file 2 (a shard was left out of a bucket, or added twice)");
            return BSK_ERR_INVALID_ARG;
        }
        P.blocks1 = blocks1;
        P.blocks2 = blocks2;
        P.pairs = p1;
        P.in_mate_order = c->fin(bsk_ctx::FIN_AUX0) == 0;
        P.shift = 0;
        while (p1 && ((p1 - 1) >> P.shift) >= BUCKET_BINS) ++P.shift;
        rc = bucket_hist_reset(c, &P.order);
        if (rc != BSK_OK) return rc;
        P.ranked = true;
    }
    if (n_pairs) *n_pairs = P.pairs;
    if (in_mate_order) *in_mate_order = P.in_mate_order ? 1 : 0;
    return BSK_OK;
}

// ---- the emit pass: a shard of file 1 leaves as its shares of paired.1 (outs[0]) and unpaired.1 (outs[1]), a shard of file 2
// as its shares of unpaired.2 (outs[1]) and -- file 2 in mate order, pair_order=buckets not set -- paired.2 (outs[2]); every
// record as pair_run_device prints it
int pair_emit_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st, bsk_out* outs) {
    const bsk_ctx::RmDupBuckets& B = c->rdb;
    const bsk_ctx::PairBuckets& P = c->pab;
    c->last_kernel_flags = 0;
    for (int k = 0; k < 3; ++k) { outs[k].d_data = nullptr; outs[k].len = 0; outs[k].records = 0; }
    int rc = rdb_emit_ready(c);
    if (rc == BSK_OK) rc = pairb_require_ranked(c, "emit_run");
    if (rc != BSK_OK) return rc;
    if (slices_wanted(c)) {
        c->set_error("libbsk: bsk_pair_emit_run: out=slices is not available on the pair path in buckets of the key");
        return BSK_ERR_UNSUPPORTED;
    }
    const bool fastq = format == BSK_FORMAT_FASTQ;
    rc = index_shard_status(c, d_buf, n, format, st);
    if (rc != BSK_OK) return rc;
    const uint64_t N = c->table.n, n1 = B.file_sums[0];
    rc = pairb_shard_range(c, "emit_run", first_record, N);
    if (rc != BSK_OK) return rc;
    if (N == 0) {
        bsk_out none;
        return empty_result(c, &none);
    }
    const bool file2 = first_record >= n1;
    TextTableH tt;
    rc = prepare_text(c, d_buf, format, st, &tt);
    if (rc != BSK_OK) return rc;
    rc = ensure_record_scratch(c);
    if (rc != BSK_OK) return rc;
    Arena A;
    const uint64_t o_fmt = A.take(N * 4), o_set = A.take(N * 4), o_clear = A.take(N * 4), o_off = A.take((N + 1) * 8), o_tot = A.take(4 * 8);
    rc = arena_reserve(c, &A);
    if (rc != BSK_OK) return rc;
    uint32_t* d_fmt = A.at<uint32_t>(o_fmt);
    uint32_t* d_len[2] = {A.at<uint32_t>(o_set), A.at<uint32_t>(o_clear)};
    uint64_t* d_off = A.at<uint64_t>(o_off);
    uint64_t* d_tot = A.at<uint64_t>(o_tot);
    SeqParams F = format_params(c, fastq);
    F.text_w = tt.text_w; F.lin_off = tt.lin_off; F.lin = tt.lin;
    F.buf_end = d_buf + n;
    HIP_TRYX(c, hipMemsetAsync(c->d_status, 0, 2 * sizeof(uint64_t), st));
    HIP_TRYX(c, hipMemsetAsync(d_tot, 0, 4 * 8, st));
    HIP_TRYX(c, launch_seq_size(d_buf, c->table, F, d_fmt, c->d_status, st));
    {
        Timed tm(c, "k_pairb_apply", st);
        HIP_TRYX(c, launch_pairb_apply(file2 ? P.d_bits2 : B.d_bits, file2 ? first_record - n1 : first_record, d_fmt, N, d_len[0], d_len[1], d_tot, st));
    }
    uint64_t tot[4], status = 0;
    HIP_TRYX(c, hipMemcpyAsync(tot, d_tot, sizeof tot, hipMemcpyDeviceToHost, st));
    HIP_TRYX(c, hipMemcpyAsync(&status, c->d_status, 8, hipMemcpyDeviceToHost, st));
    HIP_TRYX(c, hipStreamSynchronize(st));
    rc = kernel_error_to_status(c, status);
    if (rc != BSK_OK) return rc;
    // side 0: the paired records, side 1: the others
    const bool want[2] = {file2 ? (P.in_mate_order && !c->tune.is("pair_order", "buckets")) : true, c->opts.b("SaveUnpaired")};
    const int slot[2] = {file2 ? 2 : 0, 1};
    uint64_t base[3] = {0, 0, 0};
    for (int k = 0; k < 2; ++k) base[k + 1] = base[k] + (want[k] ? ((tot[k] + 255) & ~255ull) : 0);
    rc = ensure_out(c, base[2]);
    if (rc != BSK_OK) return rc;
    for (int k = 0; k < 2; ++k) {
        if (!want[k] || tot[k] == 0) continue;
        HIP_TRYX(c, launch_scan_u32(d_len[k], d_off, N, c->d_scan_tmp, st));
        rc = emit_records_at(c, d_buf, n, F, d_len[k], d_off, c->d_out + base[k], tot[k], tot[2 + k], st);
        if (rc != BSK_OK) return rc;
        outs[slot[k]].d_data = c->d_out + base[k];
        outs[slot[k]].len = tot[k];
        outs[slot[k]].records = tot[2 + k];
    }
    return BSK_OK;
}

// ---- the order phase
// a shard of file 2 under its global first_record: j0 = the index of its first record inside the file
static int pairb_order_shard(bsk_ctx* c, const char* fn, uint64_t first_record, uint64_t N, uint64_t* j0) {
    const uint64_t n1 = c->rdb.file_sums[0], total = c->rdb.total_records;
    if (first_record < n1 && N)
        return pairb_fail(c, fn, "the shard's first record " + std::to_string(first_record) + " lies in file 1 (the order phase runs over file 2, records " +
                                     std::to_string(n1) + " .. " + std::to_string(total) + ")");
    if (first_record > total || N > total - first_record)
        return pairb_fail(c, fn, "the shard's records " + std::to_string(first_record) + " .. " + std::to_string(first_record + N) +
                                     " reach past the sum of file_records = " + std::to_string(total) + " of bsk_pair_verdict_begin");
    *j0 = first_record >= n1 ? first_record - n1 : 0;
    return BSK_OK;
}

int pair_order_hist_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st, uint64_t* n_records) {
    bsk_ctx::PairBuckets& P = c->pab;
    c->last_kernel_flags = 0;
    int rc = pairb_require_ranked(c, "order_hist_run");
    if (rc != BSK_OK) return rc;
    rc = bucket_hist_alloc(c, &P.order, st);
    if (rc != BSK_OK) return rc;
    rc = index_shard_status(c, d_buf, n, format, st);  // (the counters accumulate: the complaints of the index pass come first)
    if (rc != BSK_OK) return rc;
    const uint64_t N = c->table.n;
    uint64_t j0 = 0;
    rc = pairb_order_shard(c, "order_hist_run", first_record, N, &j0);
    if (rc != BSK_OK) return rc;
    if (n_records) *n_records = N;
    if (N == 0 || P.pairs == 0) return BSK_OK;
    Timed tm(c, "k_pairb_order_hist", st);
    HIP_TRYX(c, launch_pairb_order_hist(d_buf, n, c->table, format == BSK_FORMAT_FASTQ, j0, P.d_bits2, P.d_mates, P.shift, P.order.d_hist,
                                        P.order.d_hist + BUCKET_BINS, c->num_cus, st));
    return BSK_OK;
}

int pair_order_hist_get(bsk_ctx* c, uint64_t* bytes, uint64_t* records) {
    const int rc = pairb_require_ranked(c, "order_hist_get");
    if (rc != BSK_OK) return rc;
    return bucket_hist_get(c, &c->pab.order, bytes, records);
}

int pair_order_bucket_begin(bsk_ctx* c, uint32_t lo_bin, uint32_t hi_bin) {
    bsk_ctx::PairBuckets& P = c->pab;
    int rc = pairb_require_ranked(c, "order_bucket_begin");
    if (rc != BSK_OK) return rc;
    // (the accumulation is read as one shard: the slack of one behind it)
    rc = bucket_begin(c, &P.order, "pair_order", lo_bin, hi_bin,
                      [&](uint64_t bytes, uint64_t recs) { return bucket_acc_reserve(c, &P.order, bytes + 64, recs, true, nullptr); });
    if (rc == BSK_OK) P.order_format = -1;
    return rc;
}

int pair_order_bucket_add(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st) {
    bsk_ctx::PairBuckets& P = c->pab;
    bsk_ctx::BucketState& B = P.order;
    c->last_kernel_flags = 0;
    int rc = pairb_require_ranked(c, "order_bucket_add");
    if (rc == BSK_OK) rc = bucket_require_open(c, B, "pair_order", "add");
    if (rc == BSK_OK) rc = bucket_in_order(c, B, "pair_order", first_record);
    if (rc != BSK_OK) return rc;
    if (P.order_format >= 0 && P.order_format != format) return pairb_fail(c, "order_bucket_add", "the shards of a bucket have one format");
    rc = index_shard_status(c, d_buf, n, format, st);
    if (rc != BSK_OK) return rc;
    const uint64_t N = c->table.n;
    uint64_t j0 = 0;
    rc = pairb_order_shard(c, "order_bucket_add", first_record, N, &j0);
    if (rc != BSK_OK) return rc;
    if (N == 0) return BSK_OK;
    const int fastq = format == BSK_FORMAT_FASTQ;
    const uint64_t pos_lo = (uint64_t)B.lo << P.shift, pos_hi = (uint64_t)B.hi << P.shift;
    BucketAccumulate step{c, &B, d_buf, st, "pair_order", true};
    step.pick = [&](size_t n_eff, int fastq_eff, uint32_t* out_len, uint32_t* keep) -> int {
        Timed tm(c, "k_pairb_order_pick", st);
        HIP_TRYX(c, launch_pairb_order_pick(d_buf, n_eff, c->table, fastq_eff, j0, P.d_bits2, P.d_mates, pos_lo, pos_hi, out_len, keep, c->d_status, st));
        return BSK_OK;
    };
    step.append = [&](uint64_t Nn, const uint64_t* keep_off, uint64_t n0, uint64_t bytes0) {
        return launch_pairb_order_append(Nn, j0, P.d_mates, c->d_out_len, c->d_out_off, keep_off, n0, bytes0, B.d_draw, B.d_off, B.d_len, st);
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
    P.order_format = format;
    return BSK_OK;
}

// The positions of a bucket are the run pos_lo .. pos_lo + n - 1, each once: the formatted sizes go to their slots, the scan of
// the slots gives the place of every record, and launch_seq_emit prints the records there -- the tail pair_run_device has for
// its second output.  No sort.
static int pairb_order_emit(bsk_ctx* c, hipStream_t st, bsk_out* out) {
    bsk_ctx::PairBuckets& P = c->pab;
    bsk_ctx::BucketState& B = P.order;
    const uint64_t N = B.n;
    const uint64_t pos_lo = std::min<uint64_t>((uint64_t)B.lo << P.shift, P.pairs), pos_hi = std::min<uint64_t>((uint64_t)B.hi << P.shift, P.pairs);
    if (N != pos_hi - pos_lo)
        return pairb_fail(c, "order_bucket_finish", "the bucket holds " + std::to_string(N) + " of the " + std::to_string(pos_hi - pos_lo) +
                                                        " records of paired.2 whose positions lie in its bins (every shard of file 2 is added, once)");
    if (N == 0) return empty_result(c, out);
    const bool fastq = P.order_format == BSK_FORMAT_FASTQ;
    int rc = index_shard_status(c, B.d_acc, B.acc_used, P.order_format, st);
    if (rc != BSK_OK) return rc;
    if (c->table.n != N)
        return pairb_fail(c, "order_bucket_finish", "the accumulated text reads as " + std::to_string(c->table.n) + " records, " + std::to_string(N) +
                                                        " were added");
    TextTableH tt;
    rc = prepare_text(c, B.d_acc, P.order_format, st, &tt);
    if (rc != BSK_OK) return rc;
    rc = ensure_record_scratch(c);
    if (rc != BSK_OK) return rc;
    Arena A;
    const uint64_t o_fmt = A.take(N * 4), o_slots = A.take(N * 4), o_soff = A.take((N + 1) * 8), o_off = A.take(N * 8);
    rc = arena_reserve(c, &A);
    if (rc != BSK_OK) return rc;
    uint32_t* d_fmt = A.at<uint32_t>(o_fmt);
    uint32_t* d_slots = A.at<uint32_t>(o_slots);
    uint64_t* d_soff = A.at<uint64_t>(o_soff);
    uint64_t* d_off = A.at<uint64_t>(o_off);
    uint64_t* d_bad = c->d_fin + bsk_ctx::FIN_AUX0;
    SeqParams F = format_params(c, fastq);
    F.text_w = tt.text_w; F.lin_off = tt.lin_off; F.lin = tt.lin;
    F.buf_end = B.d_acc + B.acc_used;
    HIP_TRYX(c, hipMemsetAsync(c->d_status, 0, 2 * sizeof(uint64_t), st));
    HIP_TRYX(c, hipMemsetAsync(d_bad, 0, sizeof(uint64_t), st));
    HIP_TRYX(c, hipMemsetAsync(d_slots, 0, N * 4, st));
    HIP_TRYX(c, launch_seq_size(B.d_acc, c->table, F, d_fmt, c->d_status, st));
    {
        Timed tm(c, "k_pairb_order_place", st);
        HIP_TRYX(c, launch_pairb_order_slots(B.d_draw, d_fmt, N, pos_lo, d_slots, st));
        HIP_TRYX(c, launch_scan_u32(d_slots, d_soff, N, c->d_scan_tmp, st));
        HIP_TRYX(c, launch_pairb_order_offsets(B.d_draw, d_fmt, N, pos_lo, d_slots, d_soff, d_off, d_bad, st));
    }
    uint64_t total = 0;
    HIP_TRYX(c, hipMemcpyAsync(&total, d_soff + N, sizeof total, hipMemcpyDeviceToHost, st));
    rc = ctl_readback(c, st);
    if (rc != BSK_OK) return rc;
    rc = kernel_error_to_status(c, c->status_word());
    if (rc != BSK_OK) return rc;
    if (c->fin(bsk_ctx::FIN_AUX0))
        return pairb_fail(c, "order_bucket_finish", std::to_string(c->fin(bsk_ctx::FIN_AUX0)) + " records of the bucket do not have a position of their own inside "
                                                        "its bins (the shards of file 2 are added under the first_record they had in the match phase)");
    rc = ensure_out(c, total);
    if (rc != BSK_OK) return rc;
    {
        Timed tm(c, "pairb_order_emit", st);
        HIP_TRYX(c, launch_seq_emit(B.d_acc, c->table, F, d_fmt, d_off, c->d_out, st, total, N));
    }
    HIP_TRYX(c, hipStreamSynchronize(st));  // (the accumulation is cleared with the bucket)
    out->d_data = c->d_out;
    out->len = total;
    out->records = N;
    return BSK_OK;
}

int pair_order_bucket_finish(bsk_ctx* c, hipStream_t st, bsk_out* out) {
    bsk_ctx::PairBuckets& P = c->pab;
    int rc = pairb_require_ranked(c, "order_bucket_finish");
    if (rc == BSK_OK) rc = bucket_require_open(c, P.order, "pair_order", "finish");
    if (rc != BSK_OK) return rc;
    out->d_data = nullptr;
    out->len = 0;
    out->records = 0;
    rc = pairb_order_emit(c, st, out);
    bucket_close(&P.order);
    return rc;
}

}  // namespace bsk
