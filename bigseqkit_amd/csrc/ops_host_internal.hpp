// Internal to the host side of libbsk (the ops_host*.cpp files): scratch helpers and the pieces of the
// seq-style "size -> scan -> emit" flow that several operators share.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/bsk.h"
#include "ctx.hpp"
#include "ops_host.hpp"
#include "ops_seq.hpp"
#include "ops_translate.hpp"  // TextTableH

namespace bsk {

#define HIP_TRYX(ctx, expr)                                                                  \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess) {                                                             \
            (ctx)->set_error(std::string(#expr) + ": " + hipGetErrorString(e__));           \
            return BSK_ERR_HIP;                                                              \
        }                                                                                    \
    } while (0)

template <class T>
inline int grow(bsk_ctx* c, T** p, uint64_t* cap, uint64_t need, uint64_t slack = 0) {
    if (need <= *cap && *p) return BSK_OK;
    if (*p) HIP_TRYX(c, hipFree(*p));
    *p = nullptr;
    const uint64_t n = need + slack;
    HIP_TRYX(c, hipMalloc((void**)p, std::max<uint64_t>(n, 1) * sizeof(T)));
    *cap = n;
    return BSK_OK;
}

// Scratch of the global operators (sort, rename, faidx): ONE grow-only allocation per context, carved per call.
// (hipMalloc / hipFree of gigabytes per call cost 110 of the 144 ms of `sort -l` on 25 GB.)
struct Arena {
    uint8_t* base = nullptr;
    uint64_t used = 0;
    uint64_t take(uint64_t bytes) { const uint64_t at = used; used = (used + bytes + 255) & ~255ull; return at; }
    template <class T> T* at(uint64_t off) const { return reinterpret_cast<T*>(base + off); }
};
inline int arena_reserve(bsk_ctx* c, Arena* a) {
    int rc = grow(c, &c->d_arena, &c->arena_cap, a->used, a->used / 8 + 256);
    a->base = c->d_arena;
    return rc;
}
// ... for an arena whose first `keep` bytes already hold values of this call (more was taken since the last reservation):
// they are carried over when the arena has to move, so the pointers are derived again afterwards and read the same
inline int arena_reserve_keep(bsk_ctx* c, Arena* a, uint64_t keep, hipStream_t st) {
    if (a->used > c->arena_cap) {
        uint8_t* nb = nullptr;
        const uint64_t cap = a->used + a->used / 8 + 256;
        HIP_TRYX(c, hipMalloc((void**)&nb, cap));
        HIP_TRYX(c, hipMemcpyAsync(nb, c->d_arena, keep, hipMemcpyDeviceToDevice, st));
        HIP_TRYX(c, hipStreamSynchronize(st));
        HIP_TRYX(c, hipFree(c->d_arena));
        c->d_arena = nb;
        c->arena_cap = cap;
    }
    a->base = c->d_arena;
    return BSK_OK;
}

// Open-addressing table of the key-grouping operators (rmdup, rename, pair, common, concat, grep --delete-matched):
// d_keys for N records and `cap` zeroed slots (a power of two >= 2 N) of 16 bytes {key, ~first record index}.
int key_table(bsk_ctx* c, uint64_t N, uint64_t* cap_out, uint64_t** table, hipStream_t st);
struct RmDupParams;
// c->d_keys: XXH64 keys -> first record of every record's group (+ d_has, c->d_out_len); see ops_host.cpp
int group_resolve(bsk_ctx* c, const uint8_t* d_buf, const TextTableH& tt, const RmDupParams& P, uint8_t* d_has, hipStream_t st);
// The prologue of an operator that groups the records of a shard by a key (rename, pair, common, concat), three steps:
//   group_index   before: the shard.  After: c->table and the text view `tt` of the shard, `P` zeroed but for fastq, id_mode,
//                 line_width and buf_end, c->d_keys and the record scratch grown for c->table.n records.  A shard of 2^32
//                 records or more is refused in the name of `op`.  The caller looks at c->table.n (0: nothing to group),
//                 sets the fields of P that are its own (by_name, by_seq, ignore_case) and carves its arena, d_has (one
//                 byte per record) included.
//   group_by_key  after: c->d_keys[i] = first record of record i's group, c->d_out_len[i] != 0 exactly for those firsts,
//                 d_has as group_resolve leaves it.  Launches only; the status is not read yet, so the caller queues the
//                 kernels whose result it wants in the same synchronisation (the count of file-1 records, ...)
//   group_status  the one synchronisation: the status word -- two subjects under one key refuse the call, MSG_HASH_COLLISION --
//                 and, if asked for, one more device word (d_extra -> *extra)
extern const char* const MSG_HASH_COLLISION;
int check_u32_records(bsk_ctx* c, const char* op);  // 32-bit permutations: 2^32 records or more in one shard are refused
int group_index(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, const char* op, hipStream_t st, TextTableH* tt, RmDupParams* P);
int group_by_key(bsk_ctx* c, const uint8_t* d_buf, size_t n, const TextTableH& tt, const RmDupParams& P, uint8_t* d_has, hipStream_t st);
int group_status(bsk_ctx* c, hipStream_t st, const uint64_t* d_extra = nullptr, uint64_t* extra = nullptr);
// The prologue of an operator that prints the record TEXT (range / head, duplicate, sample, shuffle and its bucket passes):
//   index_record_text   before: the shard and its format.  After: c->table; *fastq and *n are what the size kernels take -- a
//                 FASTQ shard whose records are wrapped (at its head, or the strict reader complained) is read by the
//                 multi-line reader and leaves as text from one record start to the next: *fastq = 0, *n = the byte behind
//                 the last record; a shard that is FASTQ under neither reader keeps the strict reader's complaint.  Then
//                 `queue(*n, *fastq)` -- the caller's size kernels and asynchronous read-backs -- has run, and the ONE
//                 synchronisation of the step has brought back its words and the status word, which is checked; complaints
//                 of the strict reader that show only there cost one retry (multi-line reader, `queue` again).
//                 An empty table (the caller looks at c->table.n): `queue` is not called, and nothing is read back -- the
//                 caller ends with empty_result, which reads the status -- unless `status_when_empty`: then the status is
//                 read and checked like that of any other shard (the histogram pass, which has no result to end with).
int index_record_text(bsk_ctx* c, const uint8_t* d_buf, size_t* n, int format, int* fastq, hipStream_t st, bool status_when_empty,
                      const std::function<int(size_t n, int fastq)>& queue);
// shuffle: `N` records -- record i = len[i] bytes (text + '\n') at text + off[i], inside text[0, extent), `total` bytes in all --
// leave in ascending order of their draws: one 64-bit radix sort with counting values, segment j = record perm[j], scan, the
// segmented copy (segcopy=off: byte by byte).  draws == null: draw(Seed, i), written here (stage stage_keys); the sort is
// stage_sort.  check_newline: a record may lack its '\n' in the text (the last one of a shard) and gets it in the output.
// stage_segments brackets the segment kernel alone, stage_emit (either may be null) everything from that kernel on.  The
// arena is carved here, in one reservation; the synchronisation is the one of seg_run (segcopy=off: none).
struct ShuffleRecords {
    const uint8_t* text; uint64_t extent;
    const uint64_t* off; const uint32_t* len;
    uint64_t N, total;
    const uint64_t* draws;
    bool check_newline;
    const char *stage_keys, *stage_sort, *stage_segments, *stage_emit;
};
int shuffle_order_emit(bsk_ctx* c, const ShuffleRecords& R, hipStream_t st, bsk_out* out);
// The accumulate step of an open bucket (shuffle in buckets of the draw, sort in buckets of the key), written once:
//   bucket_acc_reserve   the accumulation holds `bytes` bytes and -- with_records -- `recs` records; what it holds moves along
//   queue(n, fastq)      before: c->table describes the shard d_buf[0, n).  The record scratch, then `keep` and its scan carved
//                 out of the arena A (a caller with arrays of its own in the arena takes them from A BEFORE this call and derives
//                 their pointers inside `pick`, which runs after the reservation), pick(n, fastq, out_len, keep) -- the caller's
//                 launch: out_len[i] = text + '\n' of a record that joins the bucket, else 0; keep[i] = 1 / 0 --, the two scans,
//                 and the asynchronous read-backs of `total` and `kept`.  The caller synchronises (shuffle: the one
//                 synchronisation of index_record_text, whose `queue` this is)
//   collect()     after that synchronisation: 2^32 records in the bucket are refused in the name of `op`; the accumulation
//                 grown; launch_seg_build_text / seg_run, or the byte-wise copy with segcopy=off; the newline of a last record
//                 without one; append(N, keep_off, n0, bytes0) -- the caller's launch for what it keeps per record, null:
//                 nothing.  The segmented copy stores aligned 16-byte words, so a share starts on a 256-byte boundary of the
//                 accumulation -- unless `packed`: then the share is copied into c->d_out and from there to its packed place by
//                 one device-to-device copy, and the accumulation reads as one text.
struct BucketAccumulate {
    bsk_ctx* c;
    bsk_ctx::BucketAcc* B;
    const uint8_t* d_buf;
    hipStream_t st;
    const char* op;
    bool packed;
    std::function<int(size_t n, int fastq, uint32_t* out_len, uint32_t* keep)> pick;
    std::function<hipError_t(uint64_t N, const uint64_t* keep_off, uint64_t n0, uint64_t bytes0)> append;
    Arena A;
    uint64_t total = 0, kept = 0;
    int queue(size_t n, int fastq);
    int collect();
    uint64_t o_koff = 0;  // (between queue and collect)
    size_t n_eff = 0;
};
int bucket_acc_reserve(bsk_ctx* c, bsk_ctx::BucketAcc* B, uint64_t bytes, uint64_t recs, bool with_records, hipStream_t st,
                       uint64_t** extra = nullptr);  // extra: one more array of `recs` words (rmdup's keys), grown with the three
inline void bucket_acc_clear(bsk_ctx::BucketAcc* B) { B->n = 0; B->acc_used = 0; B->total = 0; }
// The life cycle of a bucket (bsk_ctx::BucketState), written once for shuffle, sort and rmdup.  `op` is "shuffle" / "sort" /
// "rmdup": the messages name bsk_<op>_bucket_<fn>.
//   bucket_hist_alloc / _get / _reset   the counters exist and are zero / copied to the host (null: not wanted) / zeroed
//   bucket_require_closed   INVALID_ARG "a bucket is open" in the name of bsk_<op>_<fn>
//   bucket_begin    refuses an open bucket; the bucket is bins [lo, hi), empty, next_first 0; with a histogram in this context
//                 its bytes and records over the bins are read back, 2^32 records refused, and reserve(bytes, recs) -- the
//                 caller's bucket_acc_reserve -- called when there are records; then open
//   bucket_require_open     INVALID_ARG "no bucket is open" in the name of bsk_<op>_bucket_<fn>
//   bucket_in_order   INVALID_ARG when first_record lies below next_first (bsk_<op>_bucket_add)
//   bucket_close    the end of finish, and of an add that failed for good
int bucket_hist_alloc(bsk_ctx* c, bsk_ctx::BucketState* B, hipStream_t st);
int bucket_hist_get(bsk_ctx* c, bsk_ctx::BucketState* B, uint64_t* bytes, uint64_t* records);
int bucket_hist_reset(bsk_ctx* c, bsk_ctx::BucketState* B);
int bucket_require_closed(bsk_ctx* c, const bsk_ctx::BucketState& B, const char* op, const char* fn);
int bucket_begin(bsk_ctx* c, bsk_ctx::BucketState* B, const char* op, uint32_t lo_bin, uint32_t hi_bin,
                 const std::function<int(uint64_t bytes, uint64_t recs)>& reserve);
int bucket_require_open(bsk_ctx* c, const bsk_ctx::BucketState& B, const char* op, const char* fn);
int bucket_in_order(bsk_ctx* c, const bsk_ctx::BucketState& B, const char* op, uint64_t first_record);
int bucket_too_many(bsk_ctx* c, const char* op);  // UNSUPPORTED: 2^32 or more records in one bucket of <op>
inline void bucket_close(bsk_ctx::BucketState* B) { B->open = false; bucket_acc_clear(B); }
// The steps of a bucket of `rmdup` that the buckets of `rename` and `common` and the match buckets of `pair` and `concat` take
// as well (ops_host_rmdupbuckets.cpp; all on c->rdb, the messages name the operator of the context -- rdb_op_name: "rmdup" /
// "rename" / "common" / "pair" / "concat"):
//   rdb_params          the subject of a record: rmdup's options (common's are the same three), or for rename the ID / the whole
//                 header (ByName) as it stands
//   rdb_verdict_open    the body of a *_verdict_begin behind the operator's own checks: the device is idle; *d_arr holds
//                 `words` zeroed 32-bit words (d_bits of rmdup, common and pair; d_ord of rename) and *cap says so; file_sums
//                 (one file: {total_records}) and total_records = its last entry are recorded, the verdict exists and no bin is
//                 decided.  What else an operator keeps (rename's count, the fields of PairBuckets) it sets itself afterwards.
//                 concat's d_head is 64-bit words of 0xFF and none for an empty input: it stays with concat
//   rdb_bucket_finish   bsk_<op>_bucket_finish: an open bucket is required; decide(c, st, &counted, &flagged) runs; the two
//                 counters go to the caller (null: not wanted) whatever decide returned; a decided bucket marks its bins; the
//                 bucket closes
//   rdb_flagged_read / rdb_flagged_settle   the middle of every decide, in two halves because `rename` and `pair` queue the
//                 kernels of their members between them: _read brings back m = c->d_xflag[0] with the control words in ONE
//                 synchronisation, *counted = FIN_AUX0 (what the verify kernel counted), *n_flagged = m, and refuses more than
//                 RDB_FLAG_MAX; _settle (m != 0) runs settle(c, m, st, &more) under the Timed stage and adds `more` to *counted.
//                 Neither synchronises at its end: what a decide does there is its own (rmdup: nothing)
//   rdb_verdict_bits    bits [first, first + count) of the bitmap d_bits as bytes (0 / 1); count != 0, the caller has checked
//                 the range
//   rdb_emit_tail       the end of an emit pass that prints records as Format(LineWidth) does: the block for `total` bytes,
//                 apply_long, emit_records, `out` filled
//   rdb_group_keys      the open bucket (B.n > 0): first[i] = the lowest accumulated index under the key of record i, at *o_first
//                 of the arena *A (carved and reserved there; more may be taken behind it with arena_reserve_keep); c->d_xflag
//                 holds RDB_FLAG_MAX + 1 words, the count in front zeroed
//   rdb_flagged_texts   after the comparison: the m flagged records (c->d_xflag) in input order, the global index of every
//                 accumulated record and the flagged subjects, gathered on the host; settle(list, gidx, blob, off) decides them --
//                 subject of list[j] = blob[off[j], off[j + 1]).  BSK_ERR_HIP from either gets the message
//   rdb_too_many_flagged   UNSUPPORTED: more than RDB_FLAG_MAX flagged records in one bucket
//   rdb_emit_ready / rdb_emit_in_range   the refusals of an emit pass: no verdict, the first undecided bin / a shard past the verdict
struct RmDupParams;
constexpr uint64_t RDB_FLAG_MAX = 1u << 20;  // (as XFLAG_MAX)
using RdbSettle = std::function<int(const std::vector<uint32_t>& list, const std::vector<uint64_t>& gidx, const std::string& blob,
                                    const std::vector<uint64_t>& off)>;
const char* rdb_op_name(const bsk_ctx* c);
RmDupParams rdb_params(bsk_ctx* c, const uint8_t* d_buf, size_t n, bool fastq);
int rdb_group_keys(bsk_ctx* c, hipStream_t st, Arena* A, uint64_t* o_first);
int rdb_flagged_texts(bsk_ctx* c, uint32_t m, hipStream_t st, const RdbSettle& settle);
int rdb_too_many_flagged(bsk_ctx* c);
int rdb_emit_ready(bsk_ctx* c);
int rdb_emit_in_range(bsk_ctx* c, uint64_t first_record, uint64_t N);
using RdbDecide = int (*)(bsk_ctx* c, hipStream_t st, uint64_t* n_counted, uint64_t* n_flagged);
int rdb_verdict_open(bsk_ctx* c, uint32_t** d_arr, uint64_t* cap, uint64_t words, std::vector<uint64_t> file_sums);
int rdb_bucket_finish(bsk_ctx* c, hipStream_t st, uint64_t* n_counted, uint64_t* n_flagged, RdbDecide decide);
int rdb_flagged_read(bsk_ctx* c, hipStream_t st, uint64_t* counted, uint64_t* n_flagged);
template <class Settle>
inline int rdb_flagged_settle(bsk_ctx* c, uint64_t m, const char* stage, hipStream_t st, uint64_t* counted, Settle settle) {
    if (!m) return BSK_OK;
    Timed t(c, stage, st);
    uint64_t more = 0;
    const int rc = settle(c, (uint32_t)m, st, &more);
    if (rc != BSK_OK) return rc;
    *counted += more;
    return BSK_OK;
}
int rdb_verdict_bits(bsk_ctx* c, const uint32_t* d_bits, uint64_t first, uint64_t count, uint8_t* bytes);
int rdb_emit_tail(bsk_ctx* c, const uint8_t* d_buf, size_t n, SeqParams* F, uint64_t total, uint64_t kept, hipStream_t st, bsk_out* out);
// The tail of `rename` (ops_host_next.cpp), shared by rename_run_device and the emit pass of the buckets: before, c->table and
// the text view `tt` of the shard, ren_ord[i] = the ordinal of record i (0: the record leaves as Format(LineWidth) prints it).
// The sizes, their scan, the block and the emit -- one kernel over all records when `many` of them are renamed, else
// emit_records -- and `out` filled
int rename_emit(bsk_ctx* c, const uint8_t* d_buf, size_t n, bool fastq, const TextTableH& tt, const uint32_t* ren_ord, bool many,
                hipStream_t st, bsk_out* out);
// the record table of a shard and the complaints of its index pass, read BEFORE any kernel walks the table (a shard that is
// wrapped behind its head goes to the multi-line reader, run_multiline): one synchronisation
int index_shard_status(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st);
// The key of `sort` on the host side (ops_host_next.cpp), shared by sort_run_device and the bucket passes
// (ops_host_sortbuckets.cpp): the parameters that the options and the shard give, and for -N (IDs / names) the rewritten keys
// in an allocation of their own -- P.nat / P.nat_off point into it, it lives as long as `nat`.  One synchronisation.
struct SortParams;
struct SortNatKeys { uint8_t* p = nullptr; ~SortNatKeys() { if (p) hipFree(p); } };
void sort_key_params(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, SortParams* P);
int sort_natural_keys(bsk_ctx* c, const uint8_t* d_buf, SortParams* P, hipStream_t st, SortNatKeys* nat);
// the temporary-storage query of a rocPRIM sort (the *_temp_bytes functions of ops_sort / ops_group / ops_sample)
int sort_query(bsk_ctx* c, hipError_t e);
// FASTA text view of the shard's records (text_dev.hpp); null pointers for FASTQ
int prepare_text(bsk_ctx* c, const uint8_t* d_buf, int format, hipStream_t st, TextTableH* tt, bool flatten = false,
                 bool keep_out_len = false, uint64_t buf_n = 0);  // buf_n: bytes in the shard (flatten: bounds its wide loads)
// the control block (status, counters, summary words) in c->h_ctl: one copy + one synchronisation
int ctl_readback(bsk_ctx* c, hipStream_t st);
// head / tail of the call's shard in c->h_head (one copy per call and shard)
int sample_head(bsk_ctx* c, const uint8_t* d_buf, size_t n, hipStream_t st);
// f(start, end, terminated) for every line of h[0, hb) -- end = position of its '\n', or hb for a last line without one.
// memchr per line: the samples are walked once per call, and a byte loop over 256 KiB costs a quarter of a millisecond
template <class F>
inline void for_lines(const uint8_t* h, size_t hb, F f) {
    size_t p = 0;
    while (p < hb) {
        const void* q = memchr(h + p, '\n', hb - p);
        const size_t e = q ? (size_t)((const uint8_t*)q - h) : hb;
        f(p, e, q != nullptr);
        p = e + 1;
    }
}
// size array -> scan -> total / kept / kernel status (also lists the records with a very large output)
int finish_sizes(bsk_ctx* c, hipStream_t st, uint64_t* total, uint64_t* kept);
void apply_long(const bsk_ctx* c, SeqParams* P);
// The tail of size -> scan -> emit.  Before: the size kernel of the operator has filled c->d_out_len.  After: the text in
// c->d_out and `out` filled (with allow_slices and out=slices: `out` may name segments of the shard instead, see
// try_records_as_slices).  emit_sized = finish_sizes + emit_result; an operator that looks at total / kept first (an empty
// result, a count) calls finish_sizes itself and then emit_result.  Steps in between, or another emit kernel: compose the
// pieces below instead (fa2fq, grep -c, rmdup, rename).
int emit_sized(bsk_ctx* c, const uint8_t* d_buf, size_t n, const SeqParams& P, hipStream_t st, bsk_out* out, bool allow_slices = false);
int emit_result(bsk_ctx* c, const uint8_t* d_buf, size_t n, const SeqParams& P, uint64_t total, uint64_t kept, hipStream_t st,
                bsk_out* out, bool allow_slices = false);
// the emit step of size -> scan -> emit into c->d_out (sizes in c->d_out_len / c->d_out_off): FASTQ records that leave
// unchanged go through the segmented copy when most records have output, everything else through k_seq_emit
int emit_records(bsk_ctx* c, const uint8_t* d_buf, size_t n, const SeqParams& P, uint64_t total, uint64_t kept, hipStream_t st);
// the same with the caller's size / offset arrays (offsets in RECORD order) and output place
int emit_records_at(bsk_ctx* c, const uint8_t* d_buf, size_t n, const SeqParams& P, const uint32_t* d_len, const uint64_t* d_off,
                    uint8_t* d_out, uint64_t total, uint64_t kept, hipStream_t st);
// out=slices: kept records that leave verbatim as segments of the shard (1: `out` is the result, nothing to emit; 0: emit as
// usual; < 0: -status).  Call after finish_sizes and BEFORE ensure_out: the block is not needed then.
int try_records_as_slices(bsk_ctx* c, const uint8_t* d_buf, size_t n, const SeqParams& P, uint64_t total, uint64_t kept, hipStream_t st,
                          bsk_out* out);
int empty_result(bsk_ctx* c, bsk_out* out);
// Is the segmented copy (ops_segcopy.hpp) on for this call?  Switch segcopy: "off" never, "force" always (tests); else
// when the output has SEGCOPY_MIN_BYTES and at least half of the n records are kept.  A site without thresholds passes the
// context alone (everything but "off" is yes), one with the byte threshold alone passes `total`.
constexpr uint64_t SEGCOPY_MIN_BYTES = 4u << 20;
inline bool segcopy_on(const bsk_ctx* c, uint64_t total = ~0ull, uint64_t kept = 0, uint64_t n = 0) {
    if (c->tune.is("segcopy", "off")) return false;
    if (c->tune.is("segcopy", "force")) return true;
    return total >= SEGCOPY_MIN_BYTES && kept * 2 >= n;
}
// The segmented verbatim copy as a step: output = segments k < nseg, off[k + 1] - off[k] bytes from address src[k] (0: not
// copied).  The word "other" counts what the list leaves out; it is FIN_OTHER of the control block.
//   seg_begin   c->d_seg_src grown to seg_words words (the caller carves its lists out of it), c->d_seg_first to the tiles
//               of `total` bytes, "other" zeroed.  Then the caller launches the kernel that fills its list and counts
//               into seg_other(c), and after it ONE of
//   seg_run     launch_seg_first + launch_seg_copy into d_out (stage "k_seg_copy"), then the read-back: *other.  Non-zero:
//               the caller's fix-up kernel writes the rest, or launch_seq_emit with SeqParams::seg_src = the list
//   seg_first / seg_copy   the two halves for a result that may leave as slices: seg_first reads "other" BEFORE any copy
//               (0: out_as_segments(..., c->d_seg_first, ...) and no block at all), seg_copy is the copy alone
struct SegList { const uint64_t* src; const uint64_t* off; uint64_t nseg; uint64_t total; };
inline uint64_t* seg_other(bsk_ctx* c) { return c->d_fin + bsk_ctx::FIN_OTHER; }
int seg_begin(bsk_ctx* c, uint64_t seg_words, uint64_t total, hipStream_t st);
int seg_first(bsk_ctx* c, const SegList& L, hipStream_t st, uint64_t* other);
int seg_copy(bsk_ctx* c, const SegList& L, uint8_t* d_out, const uint8_t* d_buf, size_t n, hipStream_t st);
int seg_run(bsk_ctx* c, const SegList& L, uint8_t* d_out, const uint8_t* d_buf, size_t n, hipStream_t st, uint64_t* other);
// Round 6, results as ordered slices (include/bsk.h bsk_out.d_seg_*): does the running call leave its text where it is?
inline bool slices_wanted(const bsk_ctx* c) { return c->out_slices && !c->force_contiguous; }
// ... the text as segments of the shard (kind 1: what launch_seg_copy would move) / as the per-range slices of a streaming
// pass (kind 2: what launch_slices_compact would gather; range_base = [nranges + 1] scanned bytes)
void out_as_segments(bsk_ctx* c, bsk_out* out, const uint64_t* seg_src, const uint64_t* seg_off, uint64_t nseg, const uint32_t* first4k,
                     const uint8_t* lo, const uint8_t* hi, uint64_t total, uint64_t records);
int out_as_slices(bsk_ctx* c, bsk_out* out, const uint8_t* slices, uint64_t slice_cap, const uint64_t* range_base, uint32_t nranges,
                  uint64_t total, uint64_t records, hipStream_t st);
// one block in c->d_out after all (out->d_data set, slice fields cleared); no-op on a contiguous result
int materialize_out(bsk_ctx* c, bsk_out* out, hipStream_t st);
// first4k of the pending result (kind 2 builds it on first use)
int pending_first4k(bsk_ctx* c, hipStream_t st);
// SeqParams that print the whole record unchanged == fastx.Record.Format(lineWidth)
SeqParams format_params(bsk_ctx* c, bool fastq);
void set_bits(uint32_t* set, const std::string& letters);
void check_id_regexp(bsk_ctx* c);
int id_mode_of(const bsk_ctx* c);
int id_spans(bsk_ctx* c, const uint8_t* d_buf, hipStream_t st);
// the context's feature set (ctx.features) uploaded and bound to P: name lookup, regions, suffixes, complement map
int bind_features(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, SeqParams* P);
// helpers shared by the per-operator files (ops_host_search / subseq / translate / rmdup / seq .cpp)
bool has_unquoted_comma(const std::string& p);
extern const char* const HELP_UNQUOTED_COMMA;
void parse_region_opt(const std::string& region, const char* cmd, int* start, int* end);  // reRegion + the range checks of Before()
// The steps around the kernel of a streaming pass (stream_*.hip, k_translate_stream), each written once:
//   ensure_range_arrays  before: a number of ranges.  After: c->d_anchors (anchors[nranges + 1], the queue word, k_prep's raw
//                 anchors), c->d_range_count [nranges + 1] and c->d_range_base [nranges + 2] hold that many, c->cap_ranges
//                 says so.  The ONLY code that allocates or frees the three or writes cap_ranges: they grow together.
//   range_queue   the queue word behind the anchors of `nranges` ranges
//   prep_ranges   before: the shard and the blocks of the pass.  After: the arrays grown, anchors and queue written by k_prep
//                 (queued, stage k_prep).  force_chunk != 0: ranges of that nominal size (a multiple of 16) instead of the
//                 number pick_nranges chooses
//   ensure_table  before: a capacity in records.  After: the five arrays of `t` hold `cap` records (start: cap + 1); a table
//                 that grows is a new, empty one (n = 0, no ID spans)
//   clear_status_bits    before: *status = the device status word as just read back.  After: `bits` cleared in *status and in
//                 c->d_status -- one copy, one synchronisation (the host word lives on the caller's stack)
//   head_record_count    records that begin in the head sample: FASTQ newlines / 4, FASTA "\n>" + 1
int ensure_range_arrays(bsk_ctx* c, uint32_t nranges);
inline uint32_t* range_queue(const bsk_ctx* c, uint32_t nranges) { return reinterpret_cast<uint32_t*>(c->d_anchors + (size_t)nranges + 1); }
int prep_ranges(bsk_ctx* c, const uint8_t* d_buf, size_t n, bool fastq, int blocks, hipStream_t st, uint32_t* nranges_out,
                uint64_t* chunk_out, uint64_t force_chunk = 0);
int ensure_table(bsk_ctx* c, RecordTable& t, uint64_t cap);
int clear_status_bits(bsk_ctx* c, uint64_t* status, uint64_t bits, hipStream_t st);
uint64_t head_record_count(const uint8_t* head, size_t hb, bool fastq);
// A FASTQ pass whose kernel writes the result itself, range r into slice r of c->d_slices (seq -n, subseq -r).
//   run_slice_pass  before: the shard.  After: `out` is the text -- gathered into c->d_out (stage_compact), or with out=slices
//                 the slices themselves (out_as_slices) -- and c->table.n = 0: no record table was built.  In between, in
//                 this order: prep_ranges for num_cus * per_cu blocks; the head sample (wrapped records:
//                 BSK_ERR_MULTILINE_FASTQ); ratio(head, hb, &r) = output bytes per input byte, or a status of its own
//                 (BSK_ERR_FILTER_FALLBACK: not this pass's input); slice_cap = chunk * r * 1.25 + 4096, rounded up to 16
//                 (with the test switch `scale_switch` set: r times its value, + 16); slices beyond `budget` bytes or of
//                 2^32: BSK_ERR_FILTER_FALLBACK; launch (stage_pass); the scan of bytes and records per range
//                 (k_range_scan); ONE read-back.  A slice that was too small: BSK_ERR_FILTER_FALLBACK, the bit cleared.
struct SlicePass {
    int per_cu;
    const char* scale_switch;
    uint64_t budget;
    const char *stage_pass, *stage_compact;
    std::function<int(const uint8_t* head, size_t hb, double* ratio)> ratio;
    std::function<hipError_t(int blocks, uint32_t nranges, uint32_t* queue, uint8_t* slices, uint64_t slice_cap, uint64_t* range_bytes,
                             uint64_t* range_count)> launch;
};
int run_slice_pass(bsk_ctx* c, const uint8_t* d_buf, size_t n, const SlicePass& S, hipStream_t st, bsk_out* out);
const char* alphabet_letters(Alphabet a);
void complement_table(Alphabet ab, uint8_t m[256]);
// lines of a text file ("\r\n" trimmed, empty lines skipped): pattern files, region files
std::vector<std::string> read_pattern_lines(const std::string& path);

}  // namespace bsk
