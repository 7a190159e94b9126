#pragma once
#include <hip/hip_runtime_api.h>

#include <functional>
#include <vector>

#include "../../include/bsk.h"
#include "ctx.hpp"

namespace bsk {
int kernel_error_to_status(bsk_ctx* c, uint64_t flags);
int build_index(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st);
struct FilterDev;
// not an API status: the fused pattern filter gave up (stream_filter.hpp) and the caller must build the full table
constexpr int BSK_ERR_FILTER_FALLBACK = -1000;
// internal: the head of a FASTQ shard shows records wrapped over several lines; the caller rewrites the shard
// (normalize_multiline_fastq) and runs the operator on the 4-line text
constexpr int BSK_ERR_MULTILINE_FASTQ = -1001;
bool fastq_head_multiline(const uint8_t* h, size_t hb);
// head / tail of the call's device shard in the context's pinned sample (c->h_head, c->head_len): one copy per call and shard
int sample_head(bsk_ctx* c, const uint8_t* d_buf, size_t n, hipStream_t st);
// kernel flags (stream_stats.hpp) with which the strict 4-line reader gives a FASTQ shard up: bad header 1, bad '+' line 2,
// unmatched lengths 4, truncated 8, a range that ends inside a record 16 -- a shard wrapped further down than its head
// raises one of them and is then read by the multi-line reader (c->last_kernel_flags)
constexpr uint64_t STRICT_FASTQ_FLAGS = 1u | 2u | 4u | 8u | 16u;
// d_out == null: c->table := where the records of the text begin (start[] only), *n_out := the byte behind the last one
int normalize_multiline_fastq(bsk_ctx* c, const uint8_t* d_buf, size_t n, hipStream_t st, const uint8_t** d_out, size_t* n_out);
int build_index_filtered(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, const FilterDev* F);
// the record table and, with hash != null (unfiltered FASTQ), the two keys of every record's sequence in c->d_keys / c->d_keys2
// k2 = false: k1 alone (the caller compares the bytes; c->d_keys2 is not written); group: k1 is the chain-free grouping key of
// hash_dev.hpp instead of XXH64 (only with k2 = false: a key whose value nothing but the grouping sees)
struct HashReq { bool fold; bool k2 = true; bool group = false; int mode() const { return k2 ? 1 : (group ? 2 : 0); } };
int build_index_light(bsk_ctx* c, const uint8_t* d_buf, size_t n, hipStream_t st);  // FASTA, from the '>' bytes alone (translate)
int build_index_ex(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, const FilterDev* F, const HashReq* hash);
void validate_seq_opts(bsk_ctx* c);
int seq_run_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, bsk_out* out);
void validate_grep_opts(bsk_ctx* c);
int grep_run_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, bsk_out* out);
void validate_subseq_opts(bsk_ctx* c);
int subseq_run_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, bsk_out* out);
void validate_translate_opts(bsk_ctx* c);
int translate_run_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, bsk_out* out);
void validate_rmdup_opts(bsk_ctx* c);
int rmdup_finish(bsk_ctx* c);
int rmdup_dist_keys(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, uint64_t* n_records);
int rmdup_dist_pack(bsk_ctx* c, uint64_t base, int world, uint64_t* d_send, uint64_t* counts, hipStream_t st);
int rmdup_dist_resolve(bsk_ctx* c, const uint64_t* d_tuples, uint64_t m, uint8_t* d_keep, hipStream_t st, uint64_t* d_surv = nullptr);
int rmdup_dist_emit(bsk_ctx* c, const uint64_t* d_send, const uint8_t* d_reply, uint64_t base, hipStream_t st, bsk_out* out,
                    const uint64_t* d_surv_reply = nullptr);
// round 6: the text comparison of duplicates whose survivor lives on another rank (ops_host_rmdup.cpp, include/bsk.h)
int rmdup_dist_xpack(bsk_ctx* c, const uint64_t* d_send, const uint8_t* d_reply, const uint64_t* d_surv, uint64_t base,
                     const uint64_t* rank_base, int world, uint64_t* req_cnt, uint64_t* byte_cnt, void** d_req, void** d_text, hipStream_t st);
int rmdup_dist_xcompare(bsk_ctx* c, const uint64_t* d_req_in, const uint64_t* req_from, const uint8_t* d_text_in, const uint64_t* bytes_from,
                        int world, uint8_t* d_verdict, hipStream_t st);
int rmdup_dist_xapply(bsk_ctx* c, const uint8_t* d_verdict_back, uint64_t* n_flagged, uint64_t* pairs_compared, hipStream_t st);
int rmdup_dist_flagged_get(bsk_ctx* c, void* buf, size_t cap, size_t* need, hipStream_t st);
int rmdup_dist_flagged_settle(bsk_ctx* c, const void* all, size_t n, hipStream_t st);
int rmdup_run_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, bsk_out* out);
void validate_locate_opts(bsk_ctx* c);
int locate_run_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, bsk_out* out);
void validate_replace_opts(bsk_ctx* c);
int replace_run_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, bsk_out* out);
void replace_free(bsk_ctx* c);
void validate_fa2fq_opts(bsk_ctx* c);
int fa2fq_run_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, bsk_out* out);
void fa2fq_free(bsk_ctx* c);
void validate_records_opts(bsk_ctx* c);
int range_resolve(bsk_ctx* c, int64_t n_records);
void validate_sample_opts(bsk_ctx* c);
int sample_resolve(bsk_ctx* c, uint64_t n_records);
// shuffle in buckets of the draw (ops_host_shuffle.cpp; include/bsk.h)
int shuffle_hist_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st, uint64_t* n_records);
int shuffle_bucket_begin(bsk_ctx* c, uint32_t lo_bin, uint32_t hi_bin);
int shuffle_bucket_add(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st);
int shuffle_bucket_finish(bsk_ctx* c, hipStream_t st, bsk_out* out);
// sort in buckets of the key (ops_host_sortbuckets.cpp; include/bsk.h)
std::vector<std::string> sort_pick_splitters(std::vector<std::string> keys, uint32_t max_bins);
int sort_sample_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, double rate, hipStream_t st,
                       uint64_t* n_records);
void sort_sample_reset(bsk_ctx* c);
int sort_splitters_install(bsk_ctx* c, const std::vector<std::string>& splitters);
int sort_splitters_build(bsk_ctx* c, uint32_t max_bins, uint32_t* n_bins);
int sort_hist_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, uint64_t* n_records);
int sort_bucket_begin(bsk_ctx* c, uint32_t lo_bin, uint32_t hi_bin);
int sort_bucket_add(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st);
int sort_bucket_finish(bsk_ctx* c, hipStream_t st, bsk_out* out);
// rmdup in buckets of the key (ops_host_rmdupbuckets.cpp; include/bsk.h)
int rmdup_hist_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, uint64_t* n_records);
int rmdup_verdict_begin(bsk_ctx* c, uint64_t total_records);
int rmdup_verdict_get(bsk_ctx* c, uint64_t first, uint64_t count, uint8_t* removed);
int rmdup_bucket_finish(bsk_ctx* c, hipStream_t st, uint64_t* n_removed, uint64_t* n_flagged);
int rmdup_emit_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st, bsk_out* out);
// ... the steps that `rename` and `common` in buckets of the key share with it, on an RmDup, a Rename or a Common context: the histogram without the
// refusal of rmdup's side files, the begin and the add of a bucket
int rdb_hist_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, uint64_t* n_records);
int rdb_bucket_begin(bsk_ctx* c, uint32_t lo_bin, uint32_t hi_bin);
int rdb_bucket_add(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st);
// rename in buckets of the key (ops_host_renamebuckets.cpp; include/bsk.h)
int rename_verdict_begin(bsk_ctx* c, uint64_t total_records);
int rename_verdict_get(bsk_ctx* c, uint64_t first, uint64_t count, uint32_t* ord);
int rename_bucket_finish(bsk_ctx* c, hipStream_t st, uint64_t* n_renamed, uint64_t* n_flagged);
int rename_emit_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st, bsk_out* out);
// common in buckets of the key (ops_host_commonbuckets.cpp; include/bsk.h): the histogram, the begin and the add of a bucket are
// the rdb_* steps above on a Common context
int common_verdict_begin(bsk_ctx* c, const uint64_t* file_records, uint32_t n_files);
int common_verdict_get(bsk_ctx* c, uint64_t first, uint64_t count, uint8_t* kept);
int common_bucket_finish(bsk_ctx* c, hipStream_t st, uint64_t* n_kept, uint64_t* n_flagged);
int common_emit_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st, bsk_out* out);
// pair in buckets of the key (ops_host_pairbuckets.cpp; include/bsk.h): the match histogram is rdb_hist_device on a Pair
// context, the begin and the add of a match bucket wrap rdb_bucket_begin / rdb_bucket_add; the order phase has its own passes
int pair_verdict_begin(bsk_ctx* c, const uint64_t* file_records);
int pair_verdict_get(bsk_ctx* c, uint64_t first, uint64_t count, uint64_t* pos);
int pair_bucket_begin(bsk_ctx* c, uint32_t lo_bin, uint32_t hi_bin);
int pair_bucket_add(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st);
int pair_bucket_finish(bsk_ctx* c, hipStream_t st, uint64_t* n_pairs, uint64_t* n_flagged);
int pair_order_begin(bsk_ctx* c, hipStream_t st, uint64_t* n_pairs, int* in_mate_order);
int pair_emit_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st, bsk_out* outs);
int pair_order_hist_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st, uint64_t* n_records);
int pair_order_hist_get(bsk_ctx* c, uint64_t* bytes, uint64_t* records);
int pair_order_bucket_begin(bsk_ctx* c, uint32_t lo_bin, uint32_t hi_bin);
int pair_order_bucket_add(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st);
int pair_order_bucket_finish(bsk_ctx* c, hipStream_t st, bsk_out* out);
// concat in buckets of the key (ops_host_concatbuckets.cpp; include/bsk.h): the match histogram is rdb_hist_device on a Concat
// context, the begin and the add of a match bucket wrap rdb_bucket_begin / rdb_bucket_add; the join phase has its own passes
int concat_verdict_begin(bsk_ctx* c, const uint64_t* file_records);
int concat_verdict_get(bsk_ctx* c, uint64_t first, uint64_t count, uint64_t* head);
int concat_bucket_begin(bsk_ctx* c, uint32_t lo_bin, uint32_t hi_bin);
int concat_bucket_add(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st);
int concat_bucket_finish(bsk_ctx* c, hipStream_t st, uint64_t* n_matched, uint64_t* n_flagged);
int concat_join_begin(bsk_ctx* c, hipStream_t st);
int concat_weigh_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st, uint64_t* n_records);
int concat_window_hist_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st, uint64_t* n_records);
int concat_window_hist_get(bsk_ctx* c, uint64_t* bytes, uint64_t* records);
int concat_window_begin(bsk_ctx* c, uint32_t lo_bin, uint32_t hi_bin);
int concat_window_add(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st);
int concat_window_finish(bsk_ctx* c, hipStream_t st, bsk_out* out);
int concat_tail_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, uint64_t first_record, hipStream_t st, bsk_out* out);
void validate_head_genome_opts(bsk_ctx* c);
void head_genome_reset(bsk_ctx* c);
int head_genome_run_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, bsk_out* out);
int fq2fa_run_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, bsk_out* out);
int records_run_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, bsk_out* out);
int rename_run_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, bsk_out* out);
void validate_sort_opts(bsk_ctx* c);
int sort_run_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, bsk_out* out);
void validate_faidx_opts(bsk_ctx* c);
int faidx_run_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, bsk_out* out);
int pair_run_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, size_t n_first, int format, hipStream_t st, bsk_out* outs);
void validate_common_opts(bsk_ctx* c);
int common_run_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, const uint64_t* file_ends, uint32_t nfiles, int format,
                      hipStream_t st, bsk_out* out);
int concat_run_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, size_t n_first, int format, hipStream_t st, bsk_out* out);
int faidx_query_run_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, bsk_out* out);
// faidx -d (fai_fetch.hpp / fai_fetch.cpp / ops_faidx_fetch.hip): the options of a Faidx context and the rows of an index -> a
// plan; one batch of the plan read from fd and written on the device (`out` as faidx_query_run_device leaves it) / on one
// host lane.  Every fetch leaves what it did with the calling thread (fai_last_info).
namespace fai { struct Plan; }
int fai_plan_build(bsk_ctx* c, const std::string& fai_text, uint64_t file_size, int format, uint64_t budget, fai::Plan* plan);
// gzi != null: fd is a BGZF file, gzi its block table (.gzi image), the plan's offsets are text offsets
int fai_fetch_device(bsk_ctx* c, int fd, const fai::Plan& plan, size_t batch, int threads, hipStream_t st, bsk_out* out, const void* gzi,
                     size_t gzi_len);
int fai_fetch_host(bsk_ctx* c, int fd, const fai::Plan& plan, size_t batch, std::string* text, const void* gzi, size_t gzi_len);
// the block table of a BGZF file by a header walk (BSIZE and ISIZE of every block, no inflate), and the bytes of text a table describes
int fai_gzi_build(int fd, std::string* image, uint64_t* text_size, std::string* err);
int fai_gzi_text_size(int fd, const void* gzi, size_t gzi_len, uint64_t* text_size, std::string* err);
void fai_last_info(uint64_t out[8]);
void store_drainer_free(bsk_ctx* c);  // store.cpp
int ensure_out(bsk_ctx* c, uint64_t bytes);
int ensure_record_scratch(bsk_ctx* c);
Alphabet partition_alphabet(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, int* rc);
// sequence bytes of the first record in `b` (up to `limit` bytes)
std::vector<uint8_t> head_first_seq(const std::vector<uint8_t>& b, int format, size_t limit);

// ---- shared by the entry points of capi.cpp and store.cpp (defined in capi.cpp)
typedef int (*run_fn)(bsk_ctx*, const uint8_t*, size_t, int, hipStream_t, bsk_out*);
// the record operator of c->op: what its bsk_<op>_run runs (null: none of this kind) and how bsk_run_to_store may feed it --
// not at all, as one piece (the result depends on the whole partition), or in record-aligned chunks
struct RecordOp {
    enum Store { NoStore, Whole, Chunks };
    run_fn fn = nullptr;
    Store store = NoStore;
};
RecordOp record_op(const bsk_ctx* c);
// op(d, ends) on the texts d[0, ends[0]), d[ends[0], ends[1]), ... (one text, or the files of pair / common / concat).  When the
// result calls for the multi-line FASTQ reader -- the head of a text is wrapped (BSK_ERR_MULTILINE_FASTQ), or, unless
// head_only, the strict reader gave up further down -- every text is rewritten as 4-line FASTQ and op runs once more on the
// rewrite.  head_only: bsk_run_to_store, whose chunk cuts assume 4-line records.
typedef std::function<int(const uint8_t* d, const uint64_t* ends)> TextsOp;
int run_multiline(bsk_ctx* c, const TextsOp& op, const uint8_t* d, const std::vector<uint64_t>& ends, int format, hipStream_t st,
                  bool head_only = false);
// c->d_stage[b] for `need` bytes: when need + slack exceeds what it holds it is replaced (after `st` has finished with it, if
// drain) by one of need + spare + slack bytes
int stage_reserve(bsk_ctx* c, int b, size_t need, size_t spare, size_t slack, bool drain, hipStream_t st);
// record starts that cut the host text h[0, n) into pieces of about `chunk` bytes, each holding whole records: {0, ..., n}
std::vector<size_t> record_cuts(const uint8_t* h, size_t n, int format, size_t chunk);
}  // namespace bsk
