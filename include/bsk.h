/* ============================================================================
 * bsk.h -- C ABI of libbsk.so, the MI355X (gfx950) engine behind BigSeqKit's
 * per-record map/filter hot path.
 *
 * Every entry point replaces one executor-side operator of the reference's Go
 * plugin (bigseqkit.so, looked up as "New"+Name by IgnisHPC; see
 * /root/reference/bigseqkit/helper.go:21-23).  Citations are file:line relative
 * to /root/reference/.  The lifecycle of the reference operators
 *     Before(ctx)  ->  Call(partition)...  ->  After(ctx)
 * maps to
 *     bsk_create() ->  bsk_<op>_run()...   ->  bsk_destroy().
 * Options travel exactly as in the reference: the JSON text produced by
 * bigseqkit.OptionsToString (bigseqkit/helper.go:47-55), i.e. the Go struct of
 * the command with exported field names and a nested "Config" (KitConfig).
 *
 * Plain C: pointers and sizes only; no torch / HIP types in any signature
 * (streams are passed as void* = hipStream_t, device buffers as void*).
 * All functions return 0 (BSK_OK) on success, else a BSK_ERR_* code; the
 * message (the reference's own error text where one exists) is available from
 * bsk_last_error(ctx) or, for failures that have no ctx, bsk_global_error().
 * There is NO CPU fallback: without a usable HIP device every compute entry
 * point fails with BSK_ERR_NO_DEVICE.
 *
 * THREADS.  The reference calls Call() of ONE operator struct from Threads()
 * goroutines at once (bigseqkit-lib/helper.go:413-416 per-thread channels,
 * rmdup.go:100,224 a mutex around the shared maps).  A bsk_ctx is NOT that
 * struct: it owns the device state of a call -- output buffer, record table,
 * control block, staging buffers -- so the rule is
 *     ONE CONTEXT PER CALLER THREAD (create them from the same options JSON),
 *     any number of contexts per device, any thread may use any context,
 *     but only one call at a time runs on a context.
 * A second call that arrives while one is running on the same context is
 * refused with BSK_ERR_INVALID_ARG, never raced -- the text "context busy" is in
 * the REFUSED caller's bsk_global_error() (thread-local; the context's own error
 * text and per-call state belong to the call that is running) --; this covers
 * every entry point that touches the context's device state (the *_run
 * family, bsk_stats_*, bsk_index_*, bsk_out_to_host, bsk_store_put,
 * bsk_run_to_store, the bsk_rmdup_dist_* phases, bsk_profile_read).
 * The bsk_out a run returns points into the context's output buffer and is
 * valid until the next run on that context.  Objects meant to be SHARED by
 * the threads of an executor: a bsk_store (FileStore: parts may arrive from
 * any thread in any order; internally locked) and the input shard (read-only).
 * bsk_global_error() is thread-local; bsk_last_error(ctx) belongs to the ctx.
 * Results that the reference merges across threads merge the same way here:
 * stats vectors add (bsk_stats_merge, or one device vector passed to several
 * contexts' runs on ONE stream), grep counts add, rmdup needs ONE context for
 * the whole partition (duplicates are global), the store orders the parts.
 * ==========================================================================*/
#ifndef BSK_H
#define BSK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSK_OK 0
#define BSK_ERR_INVALID_ARG 1 /* bad pointer / size / op name                         */
#define BSK_ERR_OPTS 2        /* option validation failed (reference's Before() error) */
#define BSK_ERR_FORMAT 3      /* malformed record (reference's Call() error)           */
#define BSK_ERR_UNSUPPORTED 4 /* input layout the HIP path does not accept (PARITY.md) */
#define BSK_ERR_HIP 5         /* HIP runtime error                                     */
#define BSK_ERR_NO_DEVICE 6   /* no gfx950 device visible                              */
#define BSK_ERR_CAPACITY 7    /* caller-provided output buffer too small               */
#define BSK_ERR_OVERFLOW_EXCHANGE 8 /* bsk_stats_collect on a vector reduced over ranks: slot [5] counts more lengths >=
                                     * hist_cap than this context's list holds -- exchange the lists, collect again */

#define BSK_FORMAT_FASTA 0
#define BSK_FORMAT_FASTQ 1

typedef struct bsk_ctx bsk_ctx;

/* ---- library ------------------------------------------------------------ */
int bsk_version(void);
/* number of visible HIP devices (0 when none); never fails */
int bsk_device_count(void);
const char* bsk_global_error(void);         /* thread-local */
const char* bsk_last_error(const bsk_ctx*); /* per context  */

/* ---- operator lifecycle ---------------------------------------------------
 * op_name is the reference's plugin symbol without "New":
 *   "Stats"            NewStats            bigseqkit-lib/stats.go:16
 *   "SeqTransform"     NewSeqTransform     bigseqkit-lib/seq.go:17
 *   "Grep"             NewGrep             bigseqkit-lib/grep.go:24
 *   "Locate"           NewLocate           bigseqkit-lib/locate.go:19
 *   "SubseqTransform"  NewSubseqTransform  bigseqkit-lib/subseq.go:22
 *   "Translate"        NewTranslate        bigseqkit-lib/translate.go:21
 *   "RmDup"            NewRmDupPrepare + NewRmDupCheck  bigseqkit-lib/rmdup.go:23,92
 * bsk_create == Before(): decodes opts_json (StringToOptions, helper.go:57-66),
 * fills defaults (setDefaults of the command), validates with the reference's
 * messages, uploads pattern / codon tables.  device < 0: options are parsed and
 * validated only (no HIP call is made; usable without a GPU). */
int bsk_create(const char* op_name, const char* opts_json, int device, bsk_ctx** out);
void bsk_destroy(bsk_ctx* ctx); /* == After() */
/* canonical JSON of the options after defaults (the text the reference's
 * executor would see); returned pointer lives as long as ctx */
const char* bsk_opts_json(const bsk_ctx* ctx);
/* The reference's log.Warn / log.Info lines of this context so far ("[WARN] ...\n[INFO] ...\n"; they are also written
 * to stderr as they occur): option advice of Before() -- bigseqkit-lib/seq.go:52-69, grep.go:57-98, 140-207,
 * locate.go:50-70, 96-98, 143-145, subseq.go:98-100, 127-133, 157-159.  Config.Quiet suppresses exactly the messages the
 * reference guards with it. */
const char* bsk_log_text(const bsk_ctx* ctx);
/* Run-time switches of ONE context (which kernel variant runs, thresholds): key = a name of INTEGRATION.md "Switches"
 * ("segcopy", "rmdup_keys", "min_range_bytes", ...; the old environment spelling "BSK_SEGCOPY" is accepted), value = its
 * text, NULL = unset.  A context takes the process environment's BSK_<NAME> values once, in bsk_create; nothing reads the
 * environment on the call path.  Unknown keys: BSK_ERR_INVALID_ARG. */
int bsk_ctx_set(bsk_ctx* ctx, const char* key, const char* value);

/* ---- record boundaries: PlainFile(path, delim) + ReadFixer ---------------
 * bigseqkit/helper.go:148-178, bigseqkit-lib/helper.go:41-66.
 * Finds, on the HOST, the first record start at or after `from` in a window of
 * file bytes (used to cut a file into per-GPU shards that begin on a record).
 * FASTQ: four lines per record or wrapped over several lines (SeqParser reads both,
 * bigseqkit-lib/helper.go:252-269); the window should hold the three records behind
 * the answer (1 MiB does for reads).  Returns n if there is none. */
int bsk_find_record_start(const uint8_t* buf, size_t n, size_t from, int format, size_t* out);

/* ---- Stats  (bigseqkit-lib/stats.go:27-117, StatsReduce :128-137) ---------
 * The per-partition result of Stats.Call -- a map[int64]int64 of
 * length -> count plus keys -1 (Q20), -2 (Q30), -3 (gap sum), -4 (type) --
 * is kept DEVICE-RESIDENT as one flat vector of uint64 ("stats vector"):
 *     [0]=q20 [1]=q30 [2]=gap_sum [3]=num_records [4]=error flags
 *     [5]=number of overflow lengths [6]=sum of lengths [7]=reserved
 *     [8 + L] = count of records with sequence length L, 0 <= L < hist_cap
 * so that StatsReduce across GPUs is ONE sum all-reduce (RCCL) on that vector.
 * Lengths >= hist_cap go to a ctx-owned overflow list merged by
 * bsk_stats_collect(); slot [5] counts them, so after a reduction over ranks the
 * collecting context must hold that many list entries (bsk_stats_overflow_get /
 * _add move the lists between ranks; bsk_stats_collect fails otherwise instead of
 * dropping chromosome-sized records).  Slot [4] is a per-shard diagnostic. */
#define BSK_STATS_HDR 8
size_t bsk_stats_vector_len(const bsk_ctx* ctx);
/* One Stats.Call over a shard.  `shard` holds n bytes of FASTA/FASTQ text
 * starting on a record; on_device != 0: device pointer (HBM-resident, the
 * measured path), else host pointer (staged through a pinned double buffer).
 * d_vec: device stats vector to ACCUMULATE into (caller zeroes it once, e.g. a
 * torch tensor), or NULL to use the ctx-owned vector.  stream: hipStream_t or
 * NULL.  Asynchronous w.r.t. the host when on_device; errors detected by the
 * kernels are reported by bsk_stats_collect(). */
int bsk_stats_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, void* d_vec,
                  void* stream);
/* Device-buffer plumbing for callers that do not link the HIP runtime themselves (the cgo shim, the C++ CLI):
 * shards and operator outputs can be chained on the device (the output text of seq / grep / subseq / rmdup / translate
 * is FASTA / FASTQ again) without a host round trip.  Buffers live on the current device of the calling thread
 * (device 0 unless a context of another device ran last). */
#define BSK_COPY_H2D 1
#define BSK_COPY_D2H 2
#define BSK_COPY_D2D 3
int bsk_device_select(int device); /* the current device of the calling thread (hipSetDevice): where bsk_device_alloc allocates */
void* bsk_device_alloc(size_t n);
void bsk_device_free(void* p);
int bsk_device_copy(void* dst, const void* src, size_t n, int kind); /* synchronous */

/* Pinned (page-locked) host memory for host-resident shards: read the file into such a buffer and the H2D copies of
 * bsk_stats_run(on_device = 0) are DMA at PCIe rate, overlapped with the kernels chunk by chunk (256 MiB record-aligned
 * chunks, two device buffers; BSK_STAGE_BYTES overrides the chunk size).  NULL when the allocation fails. */
void* bsk_host_alloc(size_t n);
void bsk_host_free(void* p);

/* ReadFASTA[N] / ReadFASTQ[N] (bigseqkit/helper.go:148-178: worker.PlainFile[N] gives every executor its byte ranges of the
 * file): the bytes [offset, offset + n) of the open file `fd` into a NEW buffer on `device` (*d_shard, bsk_device_free).
 * `threads` readers (<= 0: 8) pread() pieces of 16 MiB (BSK_SHARD_PIECE_BYTES) into two pinned buffers each and copy them
 * on streams of their own: reading the file and crossing PCIe overlap, 32 MiB per reader is pinned.  The caller cuts the
 * file at record starts (bsk_find_record_start on a window around size * k / world).  Errors: bsk_global_error(). */
int bsk_shard_load(int fd, uint64_t offset, size_t n, int device, int threads, void** d_shard);

/* BGZF input (PARITY.md BGZF): what `bgzip` writes, one gzip member per block of at most 64 KiB.  The blocks are independent,
 * so one wavefront inflates one block; zlib defines the bytes.  Accepted: a file without the empty EOF block, blocks of ISIZE 0
 * anywhere, extra subfields beside BC, an empty file.  Refused: bytes behind the last block that are no block header, a block
 * that reaches past the end, ISIZE above 65536, a bad DEFLATE stream, a CRC32 or ISIZE that does not fit the bytes
 * (BSK_ERR_FORMAT; the text names the block, its offset in the file and the reason), and gzip that is not BGZF
 * (BSK_ERR_UNSUPPORTED; the text names bgzip).  Errors: bsk_global_error().
 *   bsk_bgzf_probe           what the first bytes of a file are: 0 not gzip, 1 BGZF (the magic, FLG bit 2, a BC subfield of
 *                            length 2), 2 gzip that is not BGZF.  18 bytes decide an ordinary header
 *   bsk_bgzf_inflate_device  d_comp[0, n_comp) in the memory of `device` -> a NEW buffer *d_text of *n_text bytes
 *                            (bsk_device_free).  An empty input and a lone EOF block give *n_text = 0
 *   bsk_bgzf_load            bsk_shard_load of the whole file `fd`, inflated; the compressed copy is freed
 *   bsk_bgzf_blocks_device   the block index: offset and size of every block in the file and the bytes it holds.  *count is
 *                            always the number of blocks; the arrays (may be NULL with cap 0) receive the first `cap`
 *   bsk_bgzf_inflate_host    the same decoder on `threads` host threads (<= 0: 8).  cap = 0 asks for the size: *n_out */
int bsk_bgzf_probe(const void* head, size_t n);
int bsk_bgzf_inflate_device(const void* d_comp, size_t n_comp, int device, void** d_text, size_t* n_text);
int bsk_bgzf_load(int fd, int device, int threads, void** d_text, size_t* n_text);
int bsk_bgzf_blocks_device(const void* d_comp, size_t n_comp, int device, uint64_t* coff, uint32_t* csize, uint32_t* usize, size_t cap,
                           size_t* count);
int bsk_bgzf_inflate_host(const void* comp, size_t n_comp, void* out, size_t cap, size_t* n_out, int threads);
/* CRC32 of data[0, n), n <= 65536, taken as the kernel takes it: chunks of 1 KiB measured from the end, folded with the
 * "advance by 1 KiB" operator.  For the tests, which compare it with zlib's. */
uint32_t bsk_selftest_bgzf_crc(const void* data, size_t n);
/* ---- plain gzip input (PARITY.md GZIP; ops_gzip.hip, gzip_spec_dev.hpp) ----
 * What gzip / pigz write: RFC 1952 members (FEXTRA / FNAME / FCOMMENT / FHCRC allowed) of stored, fixed and dynamic blocks, up
 * to 65 536 members, empty ones included.  zlib defines the bytes: the text is every member's, concatenated.  One DEFLATE
 * stream has no independent blocks, so the compressed bytes are cut into chunks of chunk_bytes, a start of a dynamic block is
 * searched in every chunk, every chunk is decoded from its candidate at once with the unknown 32 KiB in front of it as
 * markers, the chunks that the true chain of blocks lands on are kept and their markers resolved in order.  The text does not
 * depend on chunk_bytes or on what the search finds; every member is checked against its CRC32 and ISIZE (modulo 2^32).
 * Refused with BSK_ERR_FORMAT, the text naming the member, the file offset and the reason: a bad DEFLATE stream, a CRC32 or
 * ISIZE that does not fit, a stream that ends inside a member, bytes behind the last member that are no member header (zero
 * padding too).  More than 65 536 members: BSK_ERR_UNSUPPORTED with the count.  Text, symbols (twice the text) and input that
 * do not fit on the device together: BSK_ERR_CAPACITY with the sizes.  A BGZF file given to these calls is a gzip file of many
 * members and gives the same text.  The bsk_bgzf_* calls refuse plain gzip as before.
 *   bsk_gzip_inflate_device  d_comp[0, n_comp) in the memory of `device` -> a NEW buffer *d_text of *n_text bytes
 *                            (bsk_device_free).  chunk_bytes 0: BSK_GZIP_CHUNK_BYTES if set, else the compressed size over four
 *                            times the waves of the decode kernel that the device holds, at least 256 KiB; never below 1 KiB.
 *                            THE SIZE USED IS A POWER OF TWO: a chunk_bytes, a BSK_GZIP_CHUNK_BYTES or a default between two
 *                            powers is rounded DOWN (3000 -> 2048; the default may be as little as half the quotient above),
 *                            and a size that holds the whole input makes one chunk.  bsk_gzip_last_plan says which size
 *                            was used; the text does not depend on it
 *   bsk_gzip_load            bsk_shard_load of the whole file `fd`, inflated; the compressed copy is freed
 *   bsk_gzip_inflate_host    the same source with one host lane.  chunk_bytes 0 decodes in one piece, any other value runs the
 *                            whole method (find, size, chain, decode, windows, translate) on the host, chunk_bytes rounded as
 *                            above.  cap = 0 asks for the size: *n_out -- the text is inflated then, and kept for this
 *                            thread's next call with the same comp, n_comp and chunk_bytes, which only copies it
 *   bsk_gzip_last_plan       the numbers of the last of these calls on this thread: chunks, chunks with a candidate, chunks on
 *                            the chain, candidates that were not on the chain, members, text bytes, bytes decoded by chunks that
 *                            were dropped, chunk size used
 * Stages of bsk_profile_dump (process-wide, as for BGZF): gzip_find, gzip_size, gzip_decode, gzip_windows, gzip_translate,
 * gzip_crc.  Errors: bsk_global_error(). */
int bsk_gzip_inflate_device(const void* d_comp, size_t n_comp, int device, size_t chunk_bytes, void** d_text, size_t* n_text);
int bsk_gzip_load(int fd, int device, int threads, size_t chunk_bytes, void** d_text, size_t* n_text);
int bsk_gzip_inflate_host(const void* comp, size_t n_comp, void* out, size_t cap, size_t* n_out, size_t chunk_bytes);
void bsk_gzip_last_plan(uint64_t out[8]);
/* For the tests: the finder's answer per chunk from the library's predicate on the host (cand[k] = S_k in bits, ~0: none, and for
 * chunk 0; nchunks = ceil(n_comp / chunk_bytes)), and the predicate itself at one bit position (1: a non-final dynamic block
 * can start there). */
int bsk_selftest_gzip_find(const void* comp, size_t n_comp, size_t chunk_bytes, uint64_t* cand, size_t nchunks);
int bsk_selftest_gzip_header_ok(const void* comp, size_t n_comp, uint64_t bit);
/* ---- a BGZF file as record-aligned pieces (PARITY.md BGZF "pieces"; bgzf_stream.hpp, ops_bgzf_stream.hip) ----
 * bsk_bgzf_load holds the file and its text whole.  The reader hands the text out piece by piece instead -- every piece begins
 * on a record and holds about piece_text_bytes -- and holds neither: two buffers of compressed bytes (comp_chunk_bytes each,
 * pinned and on the device) and two buffers of text are allocated at open.  device >= 0: the pieces lie in the memory of that
 * device, chunk k + 1 is read (pread) and copied under the inflate of chunk k; device = -1: the same reader with host buffers
 * and the decoder on host threads, the same pieces.  `fd` stays the caller's.  0 for a size means 1 GiB of text, 1 MiB of
 * lookahead, 256 MiB of compressed bytes.
 *
 * Positions are BGZF VIRTUAL OFFSETS: coffset << 16 | uoffset, coffset the file offset of a block, uoffset < ISIZE a byte of its
 * text.  The reader's are normalised -- never in an empty block, never at a block's end -- and the end of the text is
 * file_size << 16.  A piece is [voff_lo, voff_hi): a caller that reads the file several times keeps two numbers per piece and
 * gets the same bytes back from bsk_bgzf_reader_piece on every pass.
 *
 * Which pieces: a function of the text and the block ends alone, not of comp_chunk_bytes and not of the device.  From the
 * piece's start s, whole blocks are inflated up to E, the first block end with E - s >= piece_text_bytes + lookahead_bytes, or
 * the end of the text, where the piece is the rest.  Else the piece ends at the answer of bsk_find_record_start on text[s, E)
 * from piece_text_bytes; if there is none before E, E moves on with the lookahead doubled: a record longer than a piece makes a
 * longer piece.  The text behind the cut is the head of the next piece.
 *
 *   bsk_bgzf_reader_next    the next piece: *ptr (device or host memory, as opened; a multiple of 256), *n bytes, its offsets,
 *                           *last != 0 with the piece that ends the text.  An empty file and a lone EOF block give one empty
 *                           last piece.  A PIECE STAYS VALID UNTIL THE SECOND CALL OF next / piece AFTER THE ONE THAT GAVE IT:
 *                           operators that take a device shard are asynchronous, so the piece in front of the current one may
 *                           still be read.  Before a buffer is written again the reader's stream waits for an event recorded
 *                           on the default stream at that call
 *   bsk_bgzf_reader_seek    the next piece begins at voff (uoffset != 0: inside a block)
 *   bsk_bgzf_reader_piece   the bytes [voff_lo, voff_hi), offsets as next gave them; consecutive pieces are read on without a
 *                           seek.  Validity as for next
 *   bsk_bgzf_reader_close   waits for the device, then frees the buffers: no piece is valid afterwards
 * Refusals: those of BGZF input above, the block numbered over the whole file and named with its file offset (behind a seek
 * to a place the reader has not handed out, the message says that the number counts from the seek).  Errors:
 * bsk_global_error(); after one the reader answers with it until the next seek. */
typedef struct bsk_bgzf_reader bsk_bgzf_reader;
int bsk_bgzf_reader_open(int fd, int device, int format, size_t piece_text_bytes, size_t lookahead_bytes, size_t comp_chunk_bytes,
                         bsk_bgzf_reader** out);
int bsk_bgzf_reader_next(bsk_bgzf_reader* r, const void** ptr, size_t* n, uint64_t* voff_lo, uint64_t* voff_hi, int* last);
int bsk_bgzf_reader_seek(bsk_bgzf_reader* r, uint64_t voff);
int bsk_bgzf_reader_piece(bsk_bgzf_reader* r, uint64_t voff_lo, uint64_t voff_hi, const void** ptr, size_t* n);
void bsk_bgzf_reader_close(bsk_bgzf_reader* r);
/* ---- BGZF under several workers (PARITY.md BGZF "workers"; bgzf_cuts.hpp, ops_bgzf.hip) ----
 * BGZF blocks are independent, so a compressed file can be cut for `world` workers without decompressing it: worker k owns the
 * text [voffs[k], voffs[k + 1]), virtual offsets as the reader's above (normalised; voffs[world] = size << 16).  The cut k lies
 * at the first record start at or behind the text of B_k, the first block start at or behind size * k / world (not in front
 * of B_{k-1}).  The chain from offset 0 is not walked: B_k is found from the block headers of the ~1 MiB in front of the
 * nominal cut, tested by their BSIZE chain and a full decode (CRC32, ISIZE) of its blocks -- so the cuts are a function of the
 * file and `world` alone.  A block whose DATA holds a whole valid block can mislead that test; the worker's own walk finds it
 * out (the join check), so a wrong candidate costs time or an explicit refusal, never bytes.
 *   bsk_bgzf_cut_points   voffs[0 .. world] of the open file `fd`.  Host only: no device is touched.  A file that is damaged at
 *                         a cut: BSK_ERR_FORMAT, the offsets named
 *   bsk_bgzf_shard_load   the text [voff_lo, voff_hi) in a NEW buffer on `device` (*d_text, *n_text; bsk_device_free).  The
 *                         compressed bytes from coffset(voff_lo) to the end of the block that holds the last byte come in by
 *                         bsk_shard_load (`threads` as there), are inflated as bsk_bgzf_load inflates a file, and freed.  Every
 *                         block is written into place behind 64 KiB of room, so *d_text is a multiple of 256 and the text is
 *                         not copied again; bsk_device_free knows the allocation behind *d_text.
 *                         The join check: the chain from coffset(voff_lo) must pass through coffset(voff_hi) -- for
 *                         voff_hi = size << 16 it ends with the file, under the rules of any BGZF file.  A chain that steps
 *                         over it: BSK_ERR_UNSUPPORTED, the offset that is no block start named, nothing decoded.
 *                         Refusals: those of BGZF input above; a shard that does not begin at offset 0 names a block by its
 *                         offset in the file and numbers it from the shard's first block, and says so.  The compressed bytes
 *                         and the text do not fit side by side: BSK_ERR_CAPACITY with both sizes.
 * Errors: bsk_global_error(). */
int bsk_bgzf_cut_points(int fd, int format, int world, uint64_t* voffs /* world + 1 */);
int bsk_bgzf_shard_load(int fd, uint64_t voff_lo, uint64_t voff_hi, int device, int threads, void** d_text, size_t* n_text);
/* Where the reader's kernel cuts text[0, n) (host memory) from `from`: bsk_find_record_start's answer, n where neither finds a
 * start, or ~0: declined, the host rule decides.  device = -1: the same function on the host.  For the tests. */
int bsk_selftest_bgzf_stream_cut(const void* text, size_t n, size_t from, int format, int device, uint64_t* cut);
/* ---- a plain gzip file of any size as record-aligned pieces (PARITY.md GZIP "segments"; gzip_stream.hpp, ops_gzip_stream.hip) ----
 * bsk_gzip_load holds the file, its text and twice its text in symbols on one device.  The reader holds a SEGMENT of the file
 * at a time instead: segment_bytes of compressed data from a RESUME POINT -- a bit position at which a non-final dynamic block
 * starts, where the chain of the speculative method has landed, with the 32 KiB of text in front of it, the open member's
 * number, start, CRC and length so far -- decoded by the same steps (find, size, chain, decode, windows, translate, crc), chunk 0
 * starting at the resume bit.  A segment ends in front of the chain chunk that runs into the end of its buffer, or that would
 * bring its text above 8 times segment_bytes; that chunk's start is the next resume point.  Memory follows the sizes given
 * here, not the file.  device >= 0: the pieces lie in the memory of that device, segment k + 1 is read (pread) and copied under
 * the decode of segment k; device = -1: the same reader with host buffers and one host lane, the same pieces.  `fd` stays the
 * caller's.  0 for a size means 1 GiB of text, 1 MiB of lookahead, 64 MiB of compressed bytes, and for chunk_bytes the rule of
 * bsk_gzip_inflate_device applied to a segment (host: a sixteenth of it); sizes are rounded as there; a segment holds at least 2 KiB.
 *
 * A stream in which no non-final dynamic block starts inside a segment -- stored or fixed blocks only, one very long block --
 * makes the segment double, up to 32 times segment_bytes: then BSK_ERR_CAPACITY with the sizes (never another answer).
 *
 * Positions are TEXT OFFSETS; a piece is [text_lo, text_hi).  Which pieces: a function of the text alone, not of the segment
 * size, the chunk size or the device.  From the piece's start s the window is text[s, min(s + piece_text_bytes +
 * lookahead_bytes, end)); if it reaches the end of the text the piece is the rest, else the piece ends at the answer of
 * bsk_find_record_start on the window from piece_text_bytes; no start in the window: the lookahead doubles.
 *
 *   bsk_gzip_reader_next    the next piece: *ptr (device or host memory, as opened; a multiple of 256), *n bytes, its offsets,
 *                           *last != 0 with the piece that ends the text.  THE SEQUENTIAL PASS CHECKS CRC32 AND ISIZE of every
 *                           member, at the call that decodes its trailer.  Validity of a piece as for bsk_bgzf_reader_next: until
 *                           the second call of next / piece after the one that gave it
 *   bsk_gzip_reader_piece   the bytes [text_lo, text_hi) again.  The reader re-enters at the last resume point it has recorded
 *                           (one per segment start, 32 KiB and a few words each, in host memory) at or in front of text_lo and
 *                           decodes forward; consecutive pieces are read on without re-entry.  It checks the DEFLATE stream only
 *   bsk_gzip_reader_info    segments decoded, access points, buffer doublings, chain chunks dropped, members, text bytes so far,
 *                           peak bytes of the reader's buffers, chunk size used
 *   bsk_gzip_reader_close   waits for the device, then frees the buffers: no piece is valid afterwards
 * Refusals: those of plain gzip input above, members and offsets counted over the whole file.  Stages of bsk_profile_dump: the
 * gzip_* stages above and gzip_stream_cut.  On the command line BSK_GZIP=1 BSK_GZIP_STREAM=1 sends `stats` on a file that is not
 * read whole and the bucket paths (BSK_<COMMAND>_BUDGET_BYTES) through this reader; BSK_STREAM_PIECE_BYTES, BSK_GZIP_LOOKAHEAD_BYTES,
 * BSK_GZIP_SEGMENT_BYTES and BSK_GZIP_CHUNK_BYTES set the sizes.  Errors: bsk_global_error(); after one the reader answers with
 * it until a piece is asked for by its offsets. */
typedef struct bsk_gzip_reader bsk_gzip_reader;
int bsk_gzip_reader_open(int fd, int device, int format, size_t piece_text_bytes, size_t lookahead_bytes, size_t segment_bytes, size_t chunk_bytes,
                         bsk_gzip_reader** out);
int bsk_gzip_reader_next(bsk_gzip_reader* r, const void** ptr, size_t* n, uint64_t* text_lo, uint64_t* text_hi, int* last);
int bsk_gzip_reader_piece(bsk_gzip_reader* r, uint64_t text_lo, uint64_t text_hi, const void** ptr, size_t* n);
int bsk_gzip_reader_info(bsk_gzip_reader* r, uint64_t out[8]);
void bsk_gzip_reader_close(bsk_gzip_reader* r);
/* ---- BGZF output (PARITY.md BGZFW; ops_bgzf_write.hip, bgzf_deflate_dev.hpp) ----
 * A text becomes the BGZF file that holds it: blocks of `block_text_bytes` of text (0: 65 280, bgzip's size; at most
 * 65 280), each encoded by one wavefront -- LZ77 matches inside the block, dynamic Huffman codes per block, and per block the
 * cheapest of dynamic, fixed and stored, so that no member is longer than its text + 31 bytes.  zlib judges the bytes:
 * gzip.decompress of the file is the text.  The host encoder and the device encoder write THE SAME bytes.  Errors:
 * bsk_global_error().
 *   bsk_bgzf_deflate_bound   the most bytes n_text bytes can become, the EOF block included
 *   bsk_bgzf_deflate_device  d_text[0, n_text) in the memory of `device` -> a NEW buffer *d_comp of *n_comp bytes
 *                            (bsk_device_free; a text beyond one round -- four blocks per resident wave, 256 MiB on an MI355X --
 *                            gets a buffer of the bound, of which *n_comp bytes are the file).  The workspace is sized by the
 *                            resident waves, not by the text.  eof != 0: the 28-byte EOF block follows.  An empty text gives the EOF block
 *                            alone, or nothing.  The outputs of several calls with eof = 0 and one EOF block, concatenated,
 *                            are one valid file: this is how a text is written in pieces
 *   bsk_bgzf_deflate_host    the same encoder on `threads` host threads (<= 0: 8), the same bytes.  *n_out is what the file
 *                            needs, also when `cap` is too small (BSK_ERR_CAPACITY) */
size_t bsk_bgzf_deflate_bound(size_t n_text, uint32_t block_text_bytes);
int bsk_bgzf_deflate_device(const void* d_text, size_t n_text, int device, uint32_t block_text_bytes, int eof, void** d_comp, size_t* n_comp);
int bsk_bgzf_deflate_host(const void* text, size_t n, uint32_t block_text_bytes, int eof, void* out, size_t cap, size_t* n_out, int threads);
int bsk_stats_reset(bsk_ctx* ctx, void* stream); /* zero the ctx-owned vector, error flags and overflow list */
/* The context's list of sequence lengths >= hist_cap (the part of the reference's map[int64]int64,
 * bigseqkit-lib/stats.go:86, that does not fit the dense vector).  _get copies it to the host (cap 0 + NULL: size
 * query); _add appends lengths that another rank's context collected, before bsk_stats_collect on a reduced vector. */
int bsk_stats_overflow_get(bsk_ctx* ctx, uint64_t* lens, size_t cap, size_t* n_out);
int bsk_stats_overflow_add(bsk_ctx* ctx, const uint64_t* lens, size_t n);
/* Synchronise, check the kernels' error flags (BSK_ERR_FORMAT /
 * BSK_ERR_UNSUPPORTED) and convert a stats vector (d_vec or the ctx-owned one)
 * into the reference's map form, sorted by key.  Key -4 is computed from the
 * first record seen by this ctx (bigseqkit-lib/stats.go:106-114). */
int bsk_stats_collect(bsk_ctx* ctx, const void* d_vec, int64_t* keys, int64_t* vals, size_t cap, size_t* n_out);
/* Slot [5] of the vector the LAST bsk_stats_collect of this context read (0 before any): after an all-reduce it is the
 * same number on every rank, so "is an exchange of the overflow lists needed" is decided by all ranks alike and WITHOUT a
 * device round trip of its own (the collect already brought the vector to the host).  Protocol of a reduced step:
 *   all-reduce -> collect; if the total is non-zero on a world of more than one rank: every rank exchanges its list
 *   (bsk_stats_overflow_get / _add), then collects again.  A collect that finds fewer list entries than slot [5] counts
 *   returns BSK_ERR_OVERFLOW_EXCHANGE (and still records the total). */
int bsk_stats_overflow_total(const bsk_ctx* ctx, uint64_t* total);
/* Same conversion for a stats vector that already lives in HOST memory (e.g. after a
 * reduction done elsewhere); needs no device.  first_record (may be NULL) is the text of
 * the first record of partition 0, used for the type column exactly like Take(1). */
int bsk_stats_collect_host(bsk_ctx* ctx, const uint64_t* h_vec, size_t vec_len, const uint8_t* first_record,
                           size_t first_len, int format, int64_t* keys, int64_t* vals, size_t cap, size_t* n_out);
/* StatsReduce.Call on two host maps (sums; PARITY.md Q2) */
int bsk_stats_merge(const int64_t* ka, const int64_t* va, size_t na, const int64_t* kb, const int64_t* vb, size_t nb,
                    int64_t* keys, int64_t* vals, size_t cap, size_t* n_out);

/* driver side: Stats() bigseqkit/stats.go:75-166 and StatInfo :290-311 */
typedef struct {
    char type[16]; /* "DNA" "RNA" "Protein" "Unlimit" "" ... */
    uint64_t num, len_sum, gap_sum, len_min, len_max, n50;
    int64_t l50;
    double len_avg, q1, q2, q3, q20, q30;
} bsk_statinfo;
int bsk_stats_finalize(const bsk_ctx* ctx, const int64_t* keys, const int64_t* vals, size_t n, bsk_statinfo* out);
/* StatsString() bigseqkit/stats.go:168-288 ; out is NUL-terminated */
int bsk_stats_string(const bsk_ctx* ctx, const char* name, const char* format, const bsk_statinfo* info, char* out,
                     size_t cap);

/* ---- record-producing operators ------------------------------------------
 * The reference operators return []string, one element per output record,
 * which FileStore writes as element + "\n" (bigseqkit-lib/helper.go:447).
 * Here the result of one Call() is that byte stream, left in a ctx-owned DEVICE
 * buffer (valid until the next run on the same ctx or bsk_destroy). */
typedef struct {
    void* d_data;     /* device pointer, `len` bytes -- or NULL while the text is an ordered list of slices (below) */
    size_t len;
    uint64_t records; /* number of elements (output records) */
    /* Round 6 -- the result as ORDERED SLICES (switch "out" = "slices", bsk_ctx_set; default "contiguous": these are 0).
     * The reference's Call returns []string whose elements are (for seq -n, subseq, rmdup ...) Go strings that share the
     * bytes of the partition or of per-goroutine buffers: nothing is moved into one block
     * (bigseqkit-lib/subseq.go:167-225, seq.go:81-269, rmdup.go:200-222).  With "slices" an operator whose output text
     * already sits somewhere in HBM in output order -- the survivors of rmdup inside the input shard, the per-range
     * buffers the streaming passes of `seq -n` and `subseq -r` write, the whole FASTQ records that `seq` (length / quality
     * filters) and `grep` KEEP (segments of the shard; a dropped record is a segment of no bytes) -- returns that: segment k is the
     * d_seg_off[k + 1] - d_seg_off[k] bytes at device address d_seg_src[k]; the text is their concatenation (len bytes).
     * bsk_out_to_host, bsk_store_put and the Go shim consume slices as they are (gathered piece by piece into the
     * staging buffers of the drain); bsk_out_materialize makes the one block for a consumer that needs it (the next
     * operator of a pipe).  LIFETIME: slices of rmdup / seq / grep point into the caller's SHARD -- it must stay until the output is
     * consumed (with "contiguous" it may go as soon as the run returns); like d_data they die with the context's next run. */
    const uint64_t* d_seg_src; /* device: [n_segments] source addresses */
    const uint64_t* d_seg_off; /* device: [n_segments + 1] offsets in the output text */
    uint64_t n_segments;       /* 0: d_data holds the text */
} bsk_out;
/* copy an operator result to host memory (synchronises) */
int bsk_out_to_host(bsk_ctx* ctx, const bsk_out* out, void* dst, size_t cap);
/* The same result as BGZF: compressed on the context's device, so only the compressed bytes cross to the host.  The text is
 * taken in pieces of 64 MiB (whole blocks: a piece boundary is a block boundary), gathered piece by piece where the result
 * is a list of slices.  eof != 0: the EOF block ends the file.  cap: bsk_bgzf_deflate_bound(out->len, 0) always suffices
 * (BSK_ERR_CAPACITY otherwise).  *n_comp: the bytes written to dst. */
int bsk_out_to_host_bgzf(bsk_ctx* ctx, const bsk_out* out, int eof, void* dst, size_t cap, size_t* n_comp);
/* a result that is still a list of slices becomes ONE block in the context's output buffer (today's second move of the
 * text: k_seg_copy / k_names_compact); out->d_data is set, the slice fields are cleared.  No-op on a contiguous result. */
int bsk_out_materialize(bsk_ctx* ctx, bsk_out* out, void* stream);

/* ---- record table: SeqParser.Read (bigseqkit-lib/helper.go:219-325) --------
 * Builds, for a device- or host-resident shard, the SoA table of record slices the
 * per-record operators work on.  Exposed for tests and for callers that want the
 * offsets (faidx-style); the operators below build it themselves.
 * starts[i] = offset of the marker byte, head_len[i] = header line length incl.
 * the marker, seq_len[i] = bases.  Any output pointer may be NULL. */
int bsk_index_build(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, void* stream,
                    uint64_t* n_records);
int bsk_index_copy(bsk_ctx* ctx, uint64_t* starts, uint32_t* head_len, uint32_t* seq_len, uint32_t* aux, size_t cap);

/* ---- SeqTransform (bigseqkit-lib/seq.go:28-269) --------------------------- */
int bsk_seq_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, void* stream,
                bsk_out* out);

/* ---- Grep (bigseqkit-lib/grep.go:24-549; exact patterns: by ID, by name -n, by
 * sequence -s on both strands, -i, -v, -R region, --circular, -C count).
 * With Count set the single element is the decimal count (GrepReduceCount sums
 * them across partitions, grep.go:598-611); bsk_grep_last_count returns it as a
 * number for a 1-word all-reduce. */
int bsk_grep_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, void* stream,
                 bsk_out* out);
int bsk_grep_last_count(const bsk_ctx* ctx, uint64_t* count);
/* grep -r: the regular expression compiler of the HIP path (Go regexp / RE2 syntax subset -> position automaton,
 * bigseqkit_amd/csrc/regex_nfa.hpp) run on the HOST against one target: *matched = re.Match(text).  Needs no device;
 * lets callers (and the CPU tests) check an expression before creating a Grep context. */
int bsk_regex_match(const char* expr, const uint8_t* text, size_t n, int* matched);

/* ---- SubseqTransform by region (bigseqkit-lib/subseq.go:22-225, 314-317) -- */
int bsk_subseq_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, void* stream,
                   bsk_out* out);

/* ---- Locate (bigseqkit-lib/locate.go:19-772; exact patterns on both strands, -i, -P,
 * --circular, -G non-greedy, TSV / -M / --gtf / --bed rows).  pid == 0 emits the header
 * row first (locate.go:198-204), exactly as MapPartitionsWithIndex does. */
int bsk_locate_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, void* stream,
                   bsk_out* out);

/* ---- Translate (bigseqkit-lib/translate.go:21-145): one element per (record, frame),
 * ">Name" or ">ID_frame=N Desc" + the protein wrapped at Config.LineWidth. */
int bsk_translate_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, void* stream,
                      bsk_out* out);

/* ---- Concat (bigseqkit/concat.go:41-90; ConcatPrepare + Union + GroupByKey + ConcatJoin, bigseqkit-lib/concat.go): for
 * every ID of both files, each record of file 1 joined with each record of file 2 of that ID: header = the ID, sequence
 * and quality = A followed by B.  With Full the records of IDs present in one file only are kept unchanged.  `shard` holds
 * file 1 followed by file 2, n_first = bytes of file 1 (ending in a newline). */
int bsk_concat_run(bsk_ctx* ctx, const void* shard, size_t n, size_t n_first, int on_device, int format, void* stream,
                   bsk_out* out);

/* ---- Common (bigseqkit/common.go:56-109; CommonPrepare + Union + GroupByKey + CommonJoin, bigseqkit-lib/common.go): the
 * records of the FIRST file whose ID (full name with ByName, sequence with BySeq; IgnoreCase) occurs in every file --
 * one record per key, file order.  `shard` holds the n_files files back to back (every file ends in a newline),
 * file_ends[f] = offset one past file f (host array, file_ends[n_files - 1] == n). */
int bsk_common_run(bsk_ctx* ctx, const void* shard, size_t n, const uint64_t* file_ends, uint32_t n_files, int on_device,
                   int format, void* stream, bsk_out* out);

/* ---- Pair (bigseqkit/pair.go:34-100; PairPrepare + Union + GroupByKey + Pair, bigseqkit-lib/pair.go:37-121): match up
 * the reads of two files by ID.  `shard` holds file 1 followed by file 2, n_first = bytes of file 1 (ending in a
 * newline).  outs[0], outs[1]: the paired records of file 1 / file 2, line for line in the same pair order (= PairIndex
 * 0 / 1); outs[2], outs[3]: the records without a mate (= UnpairedId "1" / "2"), filled with SaveUnpaired only. */
int bsk_pair_run(bsk_ctx* ctx, const void* shard, size_t n, size_t n_first, int on_device, int format, void* stream,
                 bsk_out outs[4]);

/* ---- Faidx index rows (FaidxOffset + Faidx, bigseqkit/faidx.go:61-95, bigseqkit-lib/faidx.go:29-229): one row per
 * record, "<ID>\t<length>\t<offset>\t<linebases>\t<linewidth>[\t<qualoffset>]" (the .fai columns; FullHead prints the
 * whole header as the name).  base_offset = file offset of the shard's first byte (what the FaidxOffset pass
 * accumulates per partition).  Records whose sequence lines do not have the .fai shape fail with the reference's
 * "different line length in sequence: <ID>" error. */
int bsk_faidx_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t base_offset,
                  void* stream, bsk_out* out);

/* Region queries of the same context (FaidxQuery, bigseqkit-lib/faidx.go:231-432): with Regions / RegionFile in the
 * options ("id", "id:b-e", "id:b", "id:b-", "id:-e"; negative positions count from the end; b > e = reverse complement),
 * every record whose ID has a query comes back as FASTA: ">ID" or ">ID:b-e" and the region.  With UseRegexp the
 * queries are regular expressions on the ID and the hits come back whole. */
int bsk_faidx_query_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, void* stream,
                        bsk_out* out);

/* ---- faidx -d: the same regions fetched THROUGH an index, the sequence file never loaded whole (PARITY.md FAIX).  With
 * the rows bsk_faidx_run wrote for the file, the batches of a plan, in order, are the bytes of bsk_faidx_query_run on the
 * whole file as one shard.  The context is a Faidx context with regions (Regions / RegionFile / UseRegexp); --id-regexp and
 * --id-ncbi cannot be restated from an index and are BSK_ERR_OPTS here.
 *   bsk_faidx_fetch_plan   host only, no file behind it: `fai` = the text of the index (5 columns, or 6 for FASTQ: format 0 / 1,
 *                          -1 = told from the first row), file_size = bytes of the sequence file, budget_bytes = what one batch may
 *                          read and write together (0: BSK_FAIDX_FETCH_BYTES, else 1 GiB).  A row that cannot be used is
 *                          BSK_ERR_FORMAT naming the row; one region above the budget is BSK_ERR_CAPACITY with the sizes.
 *   ..._plan_counts        out[0..7] = rows, hits, batches, 1 for a FASTQ index, bases of a tile (T), bytes the batches read,
 *                          bytes they write, bytes at the head of the file read for the alphabet of '-' regions (0: none)
 *   ..._plan_hits          8 words per hit, row order: row (0-based), p0, p1 (the region, 0-based half-open), 1 for '-',
 *                          the first and one past the last file byte of its lines, the offset of its end probe, output bytes
 *   ..._plan_header        the hit's ">name[:b-e]\n"
 *   ..._plan_batch         head[0..3] = first hit, one past the last, bytes read, bytes written; spans[2k], spans[2k + 1] = the
 *                          merged 4 KiB-rounded ranges of the file it reads (cap_spans pairs; *n_spans is the number it has)
 *   bsk_faidx_fetch_run    one batch: pread of its spans (threads <= 0: 4) into pinned memory, one copy, the fetch kernel.
 *                          `out` as bsk_faidx_query_run leaves it, valid until the context's next call.  Bytes that are not
 *                          what the index predicts (every byte of every line read is judged, and two bytes behind every hit
 *                          record's predicted end): BSK_ERR_FORMAT naming row and file offset.
 *   bsk_faidx_fetch_host   the same bytes from the same source on one host lane; needs no device.  *n_out is what the batch
 *                          needs, also when `cap` is too small (BSK_ERR_CAPACITY).
 *   BGZF                   gzi != NULL: fd is a BGZF file and gzi the image of its block table (htslib's .gzi: little-endian uint64
 *                          count, then compressed offset and text offset of every block behind the first); the plan was made with
 *                          file_size = the bytes of TEXT (bsk_bgzf_gzi_text_size) and the rows' offsets are text offsets.  Every
 *                          merged span becomes a run of whole blocks: on the device through the range load of bsk_bgzf_shard_load
 *                          (every refusal of PARITY BGZF, CRC included), on the host through the host lane.  An entry that does not
 *                          land on a block header, or whose block contradicts the next entry, on a block that is touched:
 *                          BSK_ERR_FORMAT naming the entry; entries of blocks that are not touched are not looked at.
 *   bsk_bgzf_gzi_build     the image of the table by a header walk (BSIZE and ISIZE of every block, no inflate); *n_bytes is what it
 *                          needs, also when cap is too small (BSK_ERR_CAPACITY); *text_size (may be NULL) the bytes of text
 *   bsk_faidx_fetch_info   of the calling thread's last fetch (as bsk_gzip_last_plan): out[0..7] = hits, merged spans, bytes read from the file, BGZF blocks
 *                          inflated (0: a plain file; whole blocks, a block counts once per span it serves), T, tiles, bytes written, 0 */
typedef struct bsk_fai_plan bsk_fai_plan;
int bsk_faidx_fetch_plan(bsk_ctx* ctx, const char* fai, size_t fai_len, uint64_t file_size, int format, uint64_t budget_bytes,
                         bsk_fai_plan** plan);
void bsk_faidx_fetch_plan_free(bsk_fai_plan* plan);
int bsk_faidx_fetch_plan_counts(const bsk_fai_plan* plan, uint64_t out[8]);
int bsk_faidx_fetch_plan_hits(const bsk_fai_plan* plan, uint64_t* words, size_t cap_hits);
int bsk_faidx_fetch_plan_header(const bsk_fai_plan* plan, size_t hit, char* dst, size_t cap, size_t* len);
int bsk_faidx_fetch_plan_batch(const bsk_fai_plan* plan, size_t batch, uint64_t head[4], uint64_t* spans, size_t cap_spans,
                               size_t* n_spans);
int bsk_faidx_fetch_run(bsk_ctx* ctx, int fd, const void* gzi, size_t gzi_len, const bsk_fai_plan* plan, size_t batch, int threads,
                        void* stream, bsk_out* out);
int bsk_faidx_fetch_host(bsk_ctx* ctx, int fd, const void* gzi, size_t gzi_len, const bsk_fai_plan* plan, size_t batch, void* dst,
                         size_t cap, size_t* n_out);
int bsk_bgzf_gzi_build(int fd, void* dst, size_t cap, size_t* n_bytes, uint64_t* text_size);
int bsk_bgzf_gzi_text_size(int fd, const void* gzi, size_t gzi_len, uint64_t* text_size);
int bsk_faidx_fetch_info(const bsk_ctx* ctx, uint64_t out[8]);

/* ---- Sort (bigseqkit/sort.go:91-147; SortParseInputString / SortParseInputInt + SortByKey, bigseqkit-lib/sort.go):
 * by ID (default), full name (ByName), sequence prefix (BySeq, SeqPrefixLength), length (ByLength) or non-gap bases
 * (ByBases); IgnoreCase, Reverse.  Records with equal keys keep file order.  Global: ONE call sees the whole input of
 * a rank.  InNaturalOrder: natural order of IDs / names (digit runs compare as numbers). */
int bsk_sort_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, void* stream,
                 bsk_out* out);

/* ---- Rename (RenamePrepare + GroupByKey + Rename, bigseqkit/rename.go:34-60, bigseqkit-lib/rename.go:39-131):
 * the k-th further record of an ID (of a whole name with ByName) becomes "<ID>_<k> <Desc>".  Global like rmdup:
 * ONE call must see the whole input of a rank; output in file order. */
int bsk_rename_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, void* stream,
                   bsk_out* out);

/* ---- Replace (bigseqkit-lib/replace.go:127-179, options bigseqkit/replace.go:9-37): the name (or, with BySeq, the
 * FASTA sequence) of every record through Go's Regexp.ReplaceAll with template expansion; {nr} / {kv} as the reference.
 * Every record is written with record.Format(LineWidth) (FASTQ: width 0).  {nr} counts the records of one call from 1:
 * bsk_replace_run and bsk_run_to_store start it again (the chunks of one bsk_run_to_store continue it), except that
 * with the switch pin_alphabet = 1 bsk_run_to_store continues from the context's previous call (one partition fed
 * through several calls).  A record whose output would reach 2^32 bytes is BSK_ERR_UNSUPPORTED.  A target holding a byte >= 0x80 is BSK_ERR_UNSUPPORTED
 * (Go matches UTF-8 runes, this engine bytes). */
int bsk_replace_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, void* stream,
                    bsk_out* out);
/* replace on the HOST, through the routines the device runs (regex_vm.hpp): out = Regexp.ReplaceAll(text, repl) for
 * the expression `expr`; *len = bytes of the result (BSK_ERR_CAPACITY when it exceeds `cap`).  Needs no device. */
int bsk_regex_replace(const char* expr, const char* repl, const uint8_t* text, size_t n, uint8_t* out, size_t cap, size_t* len);

/* ---- Fa2Fq (bigseqkit-lib/fa2fq.go:29-120, options bigseqkit/fa2fq.go:11-23; what is computed: PARITY.md FA2FQ): the
 * FASTQ records whose ID names a record of the FASTA file `FastaFile` (read by bsk_create; keyed by full name) and whose
 * sequence holds that record's sequence -- on the read as given, else, unless OnlyPositiveStrand, on its reverse
 * complement (qualities reversed).  Each is written as "@ID\n" + the matched slice + "\n+\n" + its qualities + "\n", in
 * input order; the others leave nothing.  The table is uploaded by the context's first run and stays until bsk_destroy.
 * A FASTA shard is BSK_ERR_FORMAT ("this command only works for FASTQ format"); a table that does not fit into device
 * memory beside the shard, or an output record of 2^32 bytes or more, is BSK_ERR_UNSUPPORTED.  The result is always one
 * block (out->d_data), also with the switch out = slices. */
int bsk_fa2fq_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, void* stream,
                  bsk_out* out);

/* ---- Fq2Fa (bigseqkit-lib/fq2fa.go:16-59): every record as FASTA, the sequence on one line (Format(0)). */
int bsk_fq2fa_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, void* stream,
                  bsk_out* out);

/* ---- Range / Head (driver: bigseqkit/range.go:36-103, head.go:34-44; executor: RangePrepare + RangeFilter,
 * bigseqkit-lib/range.go:14-43).  A context is created from RangeOptions {"Range": "a:b"} or HeadOptions {"N": n}; the
 * records whose index in the WHOLE input lies in the range come back unchanged.  first_record = index of the shard's
 * first record (what MapWithIndex hands to RangePrepare.Call).  Ranges with a position below -1 need input.Count()
 * (range.go:69-80): bsk_range_needs_count says so, bsk_range_set_count supplies it before the first run. */
int bsk_range_needs_count(const bsk_ctx* ctx, int* needs);
int bsk_range_set_count(bsk_ctx* ctx, uint64_t n_records);
/* the resolved 0-based half-open record range [start, end) (after bsk_range_set_count when that was needed) */
int bsk_range_bounds(const bsk_ctx* ctx, int64_t* start, int64_t* end);
int bsk_range_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                  void* stream, bsk_out* out);

/* ---- Sample (driver: bigseqkit/sample.go:48-76; options {"Seed": 11, "Number": 0, "Proportion": 0}; PARITY.md SAMPLE).
 * draw(seed, g) = splitmix64(splitmix64((uint64)(int64)seed) ^ g), g = index of the record in the WHOLE input; record g is
 * kept iff (draw >> 11) < ceil(fraction * 2^53), fraction = float64(float32(Proportion)) or, with Number > 0,
 * Number / Count() -- not an exact count.  The verdict depends on (seed, g) alone, so the result is the same however the
 * input is cut into shards.  Kept records come back unchanged, in file order; with the switch out = slices as ordered
 * slices of the shard.  first_record = index of the shard's first record.  With Number > 0 bsk_sample_needs_count says that
 * the record count is wanted and bsk_sample_set_count supplies it before the first run.  Through bsk_run_to_store the context
 * carries the running record index over the chunks of a call (and, with the switch pin_alphabet, over the calls that feed
 * one partition); it starts from bsk_sample_set_first_record's value (default 0). */
int bsk_sample_needs_count(const bsk_ctx* ctx, int* needs);
int bsk_sample_set_count(bsk_ctx* ctx, uint64_t n_records);
int bsk_sample_set_first_record(bsk_ctx* ctx, uint64_t first_record);
int bsk_sample_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                   void* stream, bsk_out* out);

/* ---- Shuffle (bigseqkit/shuffle.go:33-46; options {"Seed": 23}; PARITY.md SHUF): the records of the shard, unchanged, in
 * ascending order of draw(seed, g) (see Sample; the draws of one seed are distinct).  Global like Sort: ONE call sees the
 * whole input; 2^32 or more records are BSK_ERR_UNSUPPORTED.  The result is always one block. */
int bsk_shuffle_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, void* stream,
                    bsk_out* out);

/* ---- Shuffle in buckets of the draw: the same result for an input of any size on one device (PARITY.md SHUF).  The upper 12
 * bits of draw(seed, g) are the "fine bin" of record g (4096 bins); a bucket is a run of consecutive bins, and the shuffled
 * output is bucket 0's records in ascending order of their draws, then bucket 1's, ...  The bytes do not depend on the
 * buckets or on how the input is cut into shards.  The input is read once for the histogram and once per bucket:
 *   bsk_shuffle_hist_run      every shard in turn (first_record = index of its first record in the whole input; *n_records =
 *                             the records of the shard): bytes (text + newline) and records per fine bin accumulate in the context
 *   bsk_shuffle_hist_get      the histogram: bytes[4096], records[4096]
 *   bsk_shuffle_hist_reset    the histogram back to zero: the context is about to see another input
 *   bsk_shuffle_plan          pure host function, no context: consecutive bins are grouped greedily into buckets of at most
 *                             budget_bytes; bounds[b] = first bin of bucket b, bounds[*n_buckets] = 4096 (bounds: room for 4097).
 *                             Empty bins join their neighbour, an empty histogram is one bucket.  A single bin above the budget
 *                             is BSK_ERR_UNSUPPORTED (bsk_global_error names its bytes and the budget).
 *   bsk_shuffle_bucket_begin / _add / _finish
 *                             one bucket: begin names its bins [lo_bin, hi_bin_exclusive), add collects the shard's records whose
 *                             draw falls into them (every shard of the input, any order), finish sorts them by draw and returns
 *                             them as one block, valid until the next call on the context.  add or finish without begin, and begin
 *                             inside an open bucket, are BSK_ERR_INVALID_ARG; 2^32 or more records in one bucket are
 *                             BSK_ERR_UNSUPPORTED (the whole input may hold more).  An error in add or finish closes the bucket. */
int bsk_shuffle_hist_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                         void* stream, uint64_t* n_records);
int bsk_shuffle_hist_get(bsk_ctx* ctx, uint64_t* bytes, uint64_t* records);
int bsk_shuffle_hist_reset(bsk_ctx* ctx);
int bsk_shuffle_plan(const uint64_t* bytes, uint64_t budget_bytes, uint64_t* bounds, int* n_buckets);
int bsk_shuffle_bucket_begin(bsk_ctx* ctx, uint32_t lo_bin, uint32_t hi_bin_exclusive);
int bsk_shuffle_bucket_add(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                           void* stream);
int bsk_shuffle_bucket_finish(bsk_ctx* ctx, void* stream, bsk_out* out);

/* ---- Sort in buckets of the key: the bytes of bsk_sort_run for an input of any size on one device (PARITY.md SORT, "Buckets").
 * The canonical key of a record is a byte string -- ID or whole header (lower-cased with IgnoreCase), its natural-order rewrite
 * with InNaturalOrder, the sequence or its SeqPrefixLength prefix with BySeq, the 32-bit number as 4 big-endian bytes with
 * ByLength / ByBases -- and two keys compare as bytes with the shorter one zero-padded.  With splitters s_0 < ... < s_(k-1)
 * (k <= 4095, any byte strings) the "fine bin" of a record is the number of splitters <= its key; a bucket is a run of
 * consecutive bins, and the output is bucket 0 sorted, then bucket 1, ... (Reverse: the buckets from the last to the first;
 * every bucket is sorted descending by the context's own option).  The bytes depend neither on the splitters nor on the
 * buckets nor on how the input is cut into shards.  The input is read once for the sample, once for the histogram and once
 * per bucket:
 *   bsk_sort_sample_run       every shard in turn: the records whose draw -- a function of first_record + i alone -- falls under
 *                             `rate` (0 .. 1) leave their keys, cut at 256 bytes, in the context.  Above a cap (switch
 *                             sort_sample_cap, default 262144 keys) the sample thins itself: the rate halves and the stored
 *                             keys above it leave, so the sample is the same for any cut into shards.  *n_records = the records
 *                             of the shard
 *   bsk_sort_sample_reset     the sample cleared;  bsk_sort_sample_count: the keys it holds
 *   bsk_sort_pick_splitters   pure host function, no context: keys (key j = keys[key_offsets[j], key_offsets[j + 1])) -> at most
 *                             max_bins - 1 strictly ascending splitters at the quantiles, duplicates collapsed; offsets: room
 *                             for max_bins entries.  No key: no splitter, one bin
 *   bsk_sort_splitters_build  bsk_sort_pick_splitters on the context's sample, the result installed; *n_bins = splitters + 1
 *   bsk_sort_splitters_set    installs splitters by hand (k <= 4095, at most 1 MiB); a list that is not strictly ascending
 *                             under the padded comparison is BSK_ERR_INVALID_ARG
 *   bsk_sort_splitters_get    the installed splitters: *k, *n_bytes, and -- with buffers -- bytes and offsets[k + 1]
 *   bsk_sort_hist_run / _hist_get / _hist_reset
 *                             as bsk_shuffle_hist_*: bytes[4096] and records[4096] per fine bin (the bins above k stay empty),
 *                             so bsk_shuffle_plan is the plan.  The histogram belongs to the splitters it was taken with
 *   bsk_sort_bucket_begin / _add / _finish
 *                             one bucket: begin names its bins, add collects the shard's records whose bin falls into them --
 *                             every shard of the input, IN INPUT ORDER (ties keep file order): a first_record that goes
 *                             backwards is BSK_ERR_INVALID_ARG -- and finish sorts them as bsk_sort_run would and returns them
 *                             as one block, valid until the next call on the context.  add or finish without begin, and begin
 *                             inside an open bucket, are BSK_ERR_INVALID_ARG; 2^32 or more records in one bucket are
 *                             BSK_ERR_UNSUPPORTED (the whole input may hold more).  An error in add or finish closes the bucket --
 *                             but a bsk_sort_bucket_add that is refused before it runs (a bad argument, a context that is busy
 *                             with another call, a host shard that could not be staged) has not touched the bucket: it stays open.
 * Every one of them is BSK_ERR_INVALID_ARG, "not a Sort context", on a context of another operator. */
int bsk_sort_sample_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                        double rate, void* stream, uint64_t* n_records);
int bsk_sort_sample_reset(bsk_ctx* ctx);
int bsk_sort_sample_count(bsk_ctx* ctx, uint64_t* n_samples);
int bsk_sort_pick_splitters(const uint8_t* keys, const uint64_t* key_offsets, uint64_t n_keys, uint32_t max_bins, uint8_t* bytes,
                            uint64_t bytes_cap, uint64_t* offsets, uint32_t* k);
int bsk_sort_splitters_build(bsk_ctx* ctx, uint32_t max_bins, uint32_t* n_bins);
int bsk_sort_splitters_set(bsk_ctx* ctx, const uint8_t* bytes, const uint64_t* offsets, uint32_t k);
int bsk_sort_splitters_get(bsk_ctx* ctx, uint8_t* bytes, uint64_t bytes_cap, uint64_t* offsets, uint32_t* k, uint64_t* n_bytes);
int bsk_sort_hist_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                      void* stream, uint64_t* n_records);
int bsk_sort_hist_get(bsk_ctx* ctx, uint64_t* bytes, uint64_t* records);
int bsk_sort_hist_reset(bsk_ctx* ctx);
int bsk_sort_bucket_begin(bsk_ctx* ctx, uint32_t lo_bin, uint32_t hi_bin_exclusive);
int bsk_sort_bucket_add(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                        void* stream);
int bsk_sort_bucket_finish(bsk_ctx* ctx, void* stream, bsk_out* out);

/* ---- RmDup in buckets of the key: the bytes of bsk_rmdup_run for an input of any size on one device (PARITY.md RMDUPB).
 * The subject of a record is its ID, its whole header with ByName or its sequence with BySeq, lower-cased with IgnoreCase;
 * record g (global index over the whole input) is removed iff a record g' < g has the same subject bytes.  The "fine bin" of
 * a record is k1 >> 52 with k1 = XXH64(subject, seed 0), so equal subjects share a bin; a bucket is a run of consecutive
 * bins and accumulates the SUBJECTS of its records, not their text.  A bucket does not print: it ends in a verdict, one bit
 * per record of the whole input, and a last pass over the input emits the survivors in file order.  The keys only find
 * candidates: every duplicate is byte-compared with the survivor of its key group, and the records that differ ("flagged")
 * are settled exactly on the host, grouped by text.  The input is read once for the histogram, once per bucket and once for
 * the emit.  The result depends neither on the buckets nor on how the input is cut into shards.
 *   bsk_rmdup_hist_run / _hist_get / _hist_reset
 *                             as bsk_shuffle_hist_*: records[4096] per fine bin, and bytes[bin] = what the accumulation will
 *                             hold for the bin -- the subject bytes of its records plus BSK_RMDUP_BUCKET_RECORD_BYTES per record
 *                             (k1, global index, offset, length) -- so bsk_shuffle_plan is the plan.  -d / -D side files are
 *                             BSK_ERR_UNSUPPORTED here
 *   bsk_rmdup_verdict_begin   a zeroed removed-bitmap for the records [0, total_records) -- the caller knows the total from the
 *                             histogram pass -- and no bin decided
 *   bsk_rmdup_verdict_get     one byte per record of [first, first + count): 1 = removed
 *   bsk_rmdup_bucket_begin / _add / _finish
 *                             one bucket: begin names its bins, add collects the subjects of the shard's records whose bin falls
 *                             into them -- every shard of the input, IN INPUT ORDER: a first_record that goes backwards, and a
 *                             shard that reaches past total_records, are BSK_ERR_INVALID_ARG -- and finish groups them, compares
 *                             the bytes, settles the flagged records, sets the bits and marks the bins decided; *n_removed =
 *                             the bits it set, *n_flagged = the records whose subject differed from their key group's survivor
 *                             (more than 2^20 of them in one bucket fail the call).  add or finish without begin, begin inside an
 *                             open bucket and begin before bsk_rmdup_verdict_begin are BSK_ERR_INVALID_ARG; 2^32 or more
 *                             records in one bucket are BSK_ERR_UNSUPPORTED.  An error in add or finish closes the bucket --
 *                             with the exception bsk_sort_bucket_add documents: an add that is refused before it runs has not
 *                             touched the bucket
 *   bsk_rmdup_emit_run        the survivors of the shard, in order, each as Format(LineWidth), as one block valid until the next
 *                             call on the context; BSK_ERR_INVALID_ARG while some bin has not been decided (the message names
 *                             the first one).  out=slices is BSK_ERR_UNSUPPORTED here
 * Every one of them is BSK_ERR_INVALID_ARG, "not an RmDup context", on a context of another operator. */
#define BSK_RMDUP_BUCKET_RECORD_BYTES 32
int bsk_rmdup_hist_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                       void* stream, uint64_t* n_records);
int bsk_rmdup_hist_get(bsk_ctx* ctx, uint64_t* bytes, uint64_t* records);
int bsk_rmdup_hist_reset(bsk_ctx* ctx);
int bsk_rmdup_verdict_begin(bsk_ctx* ctx, uint64_t total_records);
int bsk_rmdup_verdict_get(bsk_ctx* ctx, uint64_t first, uint64_t count, uint8_t* removed);
int bsk_rmdup_bucket_begin(bsk_ctx* ctx, uint32_t lo_bin, uint32_t hi_bin_exclusive);
int bsk_rmdup_bucket_add(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                         void* stream);
int bsk_rmdup_bucket_finish(bsk_ctx* ctx, void* stream, uint64_t* n_removed, uint64_t* n_flagged);
int bsk_rmdup_emit_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                       void* stream, bsk_out* out);

/* ---- Rename in buckets of the key: the bytes of bsk_rename_run for an input of any size on one device (PARITY.md RENB).
 * The subject of a record is its ID, or its whole header with ByName, as it stands; ord[g] = the number of records g' < g
 * (global index over the whole input) with the same subject bytes, and record g is printed as bsk_rename_run prints a record
 * with that ordinal: header "<ID>_<ord> <Desc>" when ord > 0, else unchanged, each record as Format(LineWidth).  The fine bin,
 * the cost of a bin, the accumulation of SUBJECTS and the key grouping are those of the RmDup buckets above -- the histogram of
 * a Rename context equals that of an RmDup context with the same ByName --, and so are the reads of the input: once for the
 * histogram, once per bucket and once for the emit.  A bucket ends in its share of the verdict, which is one uint32_t per
 * record of the whole input: 4 * (total_records + 1) bytes of device memory OUTSIDE the budget of the buckets, allocated by
 * bsk_rename_verdict_begin.  Records whose subject differs from the first of their key group ("flagged") are ranked exactly
 * on the host, grouped by text.
 *   bsk_rename_hist_run / _hist_get / _hist_reset      as bsk_rmdup_hist_*; bsk_shuffle_plan is the plan
 *   bsk_rename_verdict_begin  zeroed ordinals for the records [0, total_records), no bin decided
 *   bsk_rename_verdict_get    ord[j] = the ordinal of record first + j, j < count
 *   bsk_rename_bucket_begin / _add / _finish
 *                             as bsk_rmdup_bucket_*, with the same refusals; finish writes the non-zero ordinals of the bucket's
 *                             records: *n_renamed = their number, *n_flagged = the records whose subject differed from the
 *                             first of their key group (more than 2^20 of them in one bucket fail the call)
 *   bsk_rename_emit_run       the records of the shard, in order, renamed, as one block valid until the next call on the
 *                             context; BSK_ERR_INVALID_ARG while some bin has not been decided (the message names the first
 *                             one).  out=slices is what it is on bsk_rename_run: the block all the same
 * Every one of them is BSK_ERR_INVALID_ARG, "not a Rename context", on a context of another operator; the bsk_rmdup_* entry
 * points refuse a Rename context likewise. */
int bsk_rename_hist_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                        void* stream, uint64_t* n_records);
int bsk_rename_hist_get(bsk_ctx* ctx, uint64_t* bytes, uint64_t* records);
int bsk_rename_hist_reset(bsk_ctx* ctx);
int bsk_rename_verdict_begin(bsk_ctx* ctx, uint64_t total_records);
int bsk_rename_verdict_get(bsk_ctx* ctx, uint64_t first, uint64_t count, uint32_t* ord);
int bsk_rename_bucket_begin(bsk_ctx* ctx, uint32_t lo_bin, uint32_t hi_bin_exclusive);
int bsk_rename_bucket_add(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                          void* stream);
int bsk_rename_bucket_finish(bsk_ctx* ctx, void* stream, uint64_t* n_renamed, uint64_t* n_flagged);
int bsk_rename_emit_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                        void* stream, bsk_out* out);

/* ---- Common in buckets of the key: the bytes of bsk_common_run for files of any size on one device (PARITY.md COMB).  The
 * files are unioned in command order, g is the global record index over the union, and file_records[f] the number of records
 * of file f.  The subject of a record is its ID, its whole header with ByName or its sequence with BySeq, lower-cased with
 * IgnoreCase; record g is kept iff it lies in the FIRST file, no record g' < g has the same subject bytes, and every file
 * holds a record with those bytes.  The fine bin, the cost of a bin, the accumulation of SUBJECTS and the key grouping are
 * those of the RmDup buckets above -- the histogram of a Common context over the union equals that of an RmDup context with
 * the same three options.  The verdict is one KEEP bit per record of the first file only, (file_records[0] + 31) / 32 + 1
 * words of device memory OUTSIDE the budget of the buckets.  The files are read once for the histogram, once per bucket, and
 * the first file once more for the emit.  Records whose subject differs from the first of their key group ("flagged") are
 * settled exactly on the host, grouped by text.
 *   bsk_common_hist_run / _hist_get / _hist_reset      as bsk_rmdup_hist_*, over the shards of every file; bsk_shuffle_plan is
 *                             the plan
 *   bsk_common_verdict_begin  zeroed keep bits for the records of the first file and no bin decided; n_files outside 2 .. 64
 *                             and a null array are BSK_ERR_INVALID_ARG
 *   bsk_common_verdict_get    kept[j] = 1 when record first + j of the first file is kept, j < count; reaching past
 *                             file_records[0] is BSK_ERR_INVALID_ARG
 *   bsk_common_bucket_begin / _add / _finish
 *                             as bsk_rmdup_bucket_*, with the same refusals; add receives every shard of EVERY file in input
 *                             order, the first file first, under its global first_record -- one that goes backwards, and a
 *                             shard that reaches past the sum of file_records, are BSK_ERR_INVALID_ARG.  finish sets the keep
 *                             bits of the bucket's subjects: *n_kept = their number, *n_flagged = the records whose subject
 *                             differed from the first of their key group (more than 2^20 of them in one bucket fail the call)
 *   bsk_common_emit_run       the kept records of a shard of the FIRST file, in order, each as Format(LineWidth), as one block
 *                             valid until the next call on the context; a shard that reaches past file_records[0] and an
 *                             undecided bin (the message names the first) are BSK_ERR_INVALID_ARG.  out=slices is
 *                             BSK_ERR_UNSUPPORTED here
 * Every one of them is BSK_ERR_INVALID_ARG, "not a Common context", on a context of another operator; the bsk_rmdup_* and
 * bsk_rename_* entry points refuse a Common context likewise.  bsk_common_run still runs on a context that has been through
 * the buckets. */
int bsk_common_hist_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                        void* stream, uint64_t* n_records);
int bsk_common_hist_get(bsk_ctx* ctx, uint64_t* bytes, uint64_t* records);
int bsk_common_hist_reset(bsk_ctx* ctx);
int bsk_common_verdict_begin(bsk_ctx* ctx, const uint64_t* file_records, uint32_t n_files);
int bsk_common_verdict_get(bsk_ctx* ctx, uint64_t first, uint64_t count, uint8_t* kept);
int bsk_common_bucket_begin(bsk_ctx* ctx, uint32_t lo_bin, uint32_t hi_bin_exclusive);
int bsk_common_bucket_add(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                          void* stream);
int bsk_common_bucket_finish(bsk_ctx* ctx, void* stream, uint64_t* n_kept, uint64_t* n_flagged);
int bsk_common_emit_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                        void* stream, bsk_out* out);

/* ---- Pair in buckets of the key: the four outputs of bsk_pair_run on file 1 followed by file 2, for files of any size on one
 * device (PARITY.md PAIRB).  g is the global record index over file 1, then file 2; file_records[f] the records of file f.  The
 * subject of a record is its ID under the context's ID rule; k(g) = the records g' < g of the same file with the same subject
 * bytes; with c1, c2 records of a subject in the two files, g is paired iff k(g) < min(c1, c2), and its mate is the record of the
 * other file with the same subject and the same k.  pos(g) of a paired record of file 1 = the paired records of file 1 in front
 * of it, pos of a record of file 2 = the pos of its mate; P = the number of pairs.  paired.1 = the paired records of file 1 in
 * file order, paired.2 = those of file 2 in ascending pos, unpaired.1 / unpaired.2 (SaveUnpaired) the rest in file order.
 * Two bucket phases:
 *   match   in buckets of the key.  The fine bin, the cost of a bin, the accumulation of SUBJECTS and the key grouping are
 *           those of the RmDup buckets above -- the histogram of a Pair context over the union equals that of an RmDup context
 *           with default options.  A bucket ends in its share of the verdict: one PAIRED bit per record of either file and 8
 *           bytes per record of file 2 (the mate, later pos), device memory OUTSIDE the budget of the buckets
 *   order   in buckets of pos.  With s the least shift with (P - 1) >> s < 4096, the order bin of a paired record of file 2 is
 *           pos >> s; a bin costs the bytes of its record text (text + newline; a wrapped FASTQ shard: its 4-line rewrite);
 *           bsk_shuffle_plan plans these too.  paired.2 = bucket 0's records in ascending pos, then bucket 1's, ...
 * File 2 is "in mate order" iff pos of every paired record of file 2 equals the paired records of file 2 in front of it: then
 * paired.2 is a filter of file 2, the emit pass prints it, and the order phase is not needed.
 *   bsk_pair_hist_run / _hist_get / _hist_reset      as bsk_rmdup_hist_*, over the shards of file 1, then file 2
 *   bsk_pair_verdict_begin    zeroed bits for file_records[0] + file_records[1] records, no bin decided, no positions
 *   bsk_pair_bucket_begin / _add / _finish
 *                             as bsk_rmdup_bucket_*, with the same refusals; add receives every shard of file 1, then of file 2,
 *                             in input order under its global first_record; a shard that straddles the two files or reaches
 *                             past the sum of file_records is BSK_ERR_INVALID_ARG.  finish: *n_pairs = the pairs the bucket
 *                             found, *n_flagged = the records whose subject differed from the first of their key group (they
 *                             are paired on the host by text; more than 2^20 of them in one bucket fail the call)
 *   bsk_pair_order_begin      the rank step, once every bin is decided (else BSK_ERR_INVALID_ARG, the message names the first
 *                             undecided bin): every mate becomes pos; *n_pairs = P, *in_mate_order = 1 / 0.  A second call
 *                             reports the same.  No match bucket can begin afterwards
 *   bsk_pair_verdict_get      pos[j] of global record first + j, j < count; ~0: unpaired.  Valid after bsk_pair_order_begin
 *   bsk_pair_emit_run         a shard of ONE file under its global first_record, after bsk_pair_order_begin.  File 1: outs[0] =
 *                             its share of paired.1, outs[1] = of unpaired.1.  File 2: outs[1] = its share of unpaired.2,
 *                             outs[2] = of paired.2 when file 2 is in mate order and the switch pair_order is not "buckets",
 *                             else empty.  Unpaired shares with SaveUnpaired only.  The blocks are valid until the next call on
 *                             the context.  out=slices is BSK_ERR_UNSUPPORTED here
 *   bsk_pair_order_hist_run / _hist_get
 *                             the histogram of the order bins over the shards of file 2 (bsk_pair_order_begin zeroes it)
 *   bsk_pair_order_bucket_begin / _add / _finish
 *                             add takes the shards of file 2 in input order under their global first_record; finish returns
 *                             the bucket's share of paired.2 and fails (BSK_ERR_INVALID_ARG) when the bucket did not receive
 *                             exactly the records of its bins
 * The switch pair_order=buckets (bsk_ctx_set; tests) makes the emit pass leave paired.2 to the order phase on ordered input too.
 * Every one of them is BSK_ERR_INVALID_ARG, "not a Pair context", on a context of another operator; the bsk_rmdup_*,
 * bsk_rename_* and bsk_common_* entry points refuse a Pair context likewise.  bsk_pair_run still runs on a context that has been
 * through the buckets. */
int bsk_pair_hist_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                      void* stream, uint64_t* n_records);
int bsk_pair_hist_get(bsk_ctx* ctx, uint64_t* bytes, uint64_t* records);
int bsk_pair_hist_reset(bsk_ctx* ctx);
int bsk_pair_verdict_begin(bsk_ctx* ctx, const uint64_t file_records[2]);
int bsk_pair_verdict_get(bsk_ctx* ctx, uint64_t first, uint64_t count, uint64_t* pos);
int bsk_pair_bucket_begin(bsk_ctx* ctx, uint32_t lo_bin, uint32_t hi_bin_exclusive);
int bsk_pair_bucket_add(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                        void* stream);
int bsk_pair_bucket_finish(bsk_ctx* ctx, void* stream, uint64_t* n_pairs, uint64_t* n_flagged);
int bsk_pair_order_begin(bsk_ctx* ctx, void* stream, uint64_t* n_pairs, int* in_mate_order);
int bsk_pair_emit_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                      void* stream, bsk_out outs[3]);
int bsk_pair_order_hist_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                            void* stream, uint64_t* n_records);
int bsk_pair_order_hist_get(bsk_ctx* ctx, uint64_t* bytes, uint64_t* records);
int bsk_pair_order_bucket_begin(bsk_ctx* ctx, uint32_t lo_bin, uint32_t hi_bin_exclusive);
int bsk_pair_order_bucket_add(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                              void* stream);
int bsk_pair_order_bucket_finish(bsk_ctx* ctx, void* stream, bsk_out* out);

/* ---- Concat in buckets of the key: the bytes of bsk_concat_run on file 1 followed by file 2, for files of any size on one
 * device (PARITY.md CONB).  g is the global record index over file 1 (n1 records), then file 2 (n2); the subject of a record is
 * its ID under the context's ID rule.  head(g) = the lowest g' < n1 with the subject bytes of g, ~0 when file 1 has none; for a
 * head h, C[h] = the records b of file 2 with head(b) == h and W[h] = the sum of their text costs t(b) (text + newline; a
 * wrapped FASTQ shard: its 4-line rewrite).  Two phases:
 *   match   in buckets of the key, as the match phase of Pair: fine bin, cost of a bin, accumulation of SUBJECTS and key
 *           grouping are those of the RmDup buckets -- the histogram of a Concat context over the union equals that of an RmDup
 *           context with default options.  A bucket ends in its share of the verdict: one 64-bit head per record of either
 *           file, device memory OUTSIDE the budget of the buckets
 *   join    in windows of file 1.  With s the least shift with (n1 - 1) >> s < 4096, the window bin of record a of file 1 is
 *           a >> s; a bin costs the sum of cost(a) = t(a) * (1 + C[h]) + 2 * W[h], h = head(a), over its records -- a planning
 *           bound, not a size; bsk_shuffle_plan plans these too, and refuses a bin above the budget.  A window [lo, hi) of bins
 *           accumulates its records of file 1 and every record of file 2 whose head is the head of one of them, and runs the
 *           one call on that: its share of the output.  The output = window 0's share, window 1's, ..., and with Full the tail:
 *           the records of file 2 without a head, in file order
 *   bsk_concat_hist_run / _hist_get / _hist_reset    as bsk_rmdup_hist_*, over the shards of file 1, then file 2
 *   bsk_concat_verdict_begin  heads for file_records[0] + file_records[1] records, no bin decided, the join phase not begun
 *   bsk_concat_bucket_begin / _add / _finish
 *                             as bsk_pair_bucket_*, with the same refusals; finish: *n_matched = the records of the bucket that
 *                             have a head, *n_flagged = the records whose subject differed from the first of their key group
 *                             (settled on the host by text; more than 2^20 of them in one bucket fail the call).  No match
 *                             bucket can begin after bsk_concat_join_begin
 *   bsk_concat_join_begin     once every bin is decided (else BSK_ERR_INVALID_ARG, the message names the first undecided bin):
 *                             zeroed W and C (16 bytes per record of file 1, outside the budget), the mark bits, the window
 *                             histogram.  Every call below needs it
 *   bsk_concat_verdict_get    head[j] of global record first + j, j < count; ~0: none
 *   bsk_concat_weigh_run      a shard of file 2 under its global first_record: its records counted into W and C, each shard once
 *   bsk_concat_window_hist_run / _window_hist_get
 *                             the histogram of the window bins over the shards of file 1; refused until exactly n2 records
 *                             have been weighed
 *   bsk_concat_window_begin / _window_add / _window_finish
 *                             add takes the shards of file 1, then of file 2, in input order under their global first_record (a
 *                             shard of file 1 wholly outside the window adds nothing and may be left out; a shard of file 1
 *                             after one of file 2 is BSK_ERR_INVALID_ARG); finish returns the window's share and fails
 *                             (BSK_ERR_INVALID_ARG) when the window did not receive exactly the records of file 1 of its bins,
 *                             or has not seen n2 records of file 2.  out=slices is BSK_ERR_UNSUPPORTED
 *   bsk_concat_tail_run       a shard of file 2 under its global first_record: with Full its records without a head, as the one
 *                             call prints an unmatched record; without Full an empty result.  out=slices is BSK_ERR_UNSUPPORTED
 * Every one of them is BSK_ERR_INVALID_ARG, "not a Concat context", on a context of another operator; the bsk_rmdup_*,
 * bsk_rename_*, bsk_common_* and bsk_pair_* entry points refuse a Concat context likewise.  bsk_concat_run still runs on a
 * context that has been through the buckets; the 32-bit size of the elements of one record of file 1 remains its limit here. */
int bsk_concat_hist_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                        void* stream, uint64_t* n_records);
int bsk_concat_hist_get(bsk_ctx* ctx, uint64_t* bytes, uint64_t* records);
int bsk_concat_hist_reset(bsk_ctx* ctx);
int bsk_concat_verdict_begin(bsk_ctx* ctx, const uint64_t file_records[2]);
int bsk_concat_verdict_get(bsk_ctx* ctx, uint64_t first, uint64_t count, uint64_t* head);
int bsk_concat_bucket_begin(bsk_ctx* ctx, uint32_t lo_bin, uint32_t hi_bin_exclusive);
int bsk_concat_bucket_add(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                          void* stream);
int bsk_concat_bucket_finish(bsk_ctx* ctx, void* stream, uint64_t* n_matched, uint64_t* n_flagged);
int bsk_concat_join_begin(bsk_ctx* ctx, void* stream);
int bsk_concat_weigh_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                         void* stream, uint64_t* n_records);
int bsk_concat_window_hist_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid,
                               uint64_t first_record, void* stream, uint64_t* n_records);
int bsk_concat_window_hist_get(bsk_ctx* ctx, uint64_t* bytes, uint64_t* records);
int bsk_concat_window_begin(bsk_ctx* ctx, uint32_t lo_bin, uint32_t hi_bin_exclusive);
int bsk_concat_window_add(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                          void* stream);
int bsk_concat_window_finish(bsk_ctx* ctx, void* stream, bsk_out* out);
int bsk_concat_tail_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, uint64_t first_record,
                        void* stream, bsk_out* out);

/* ---- HeadGenome (bigseqkit/head_genome.go, bigseqkit-lib/head_genome.go:53-108; options {"MiniCommonWords": 1}; PARITY.md
 * HEADG): the records of the first genome.  The words of a record are the maximal runs of its description other than ' '
 * and '\t'; the prefix is the words of the first record of the input; n_i = leading words of record i equal to the prefix's.
 * The output is the records before the first i >= 1 with n_i < MiniCommonWords or n_i != n_1, each as Format(LineWidth)
 * (== Seq without options).  A kept record without a description fails the call: "no description: <ID>".  ONE cut over
 * the whole input: the context carries the prefix, n_1, "cut reached" and the record count from call to call, so the shards
 * of an input are run IN ORDER on one context and give the same bytes however the input was cut; a shard behind the cut
 * gives nothing and costs nothing.  bsk_head_genome_state says whether the cut is reached (the caller stops reading) and
 * how many records were kept so far; bsk_head_genome_reset starts the next input.  Through bsk_run_to_store a call is an
 * input of its own unless the switch pin_alphabet says that several calls carry one.  On a device-resident shard the
 * search runs over growing windows of the text (switch head_genome_window, bytes; 0: the whole shard at once), so its cost
 * follows the first genome, not the shard. */
int bsk_head_genome_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, void* stream,
                        bsk_out* out);
int bsk_head_genome_reset(bsk_ctx* ctx);
int bsk_head_genome_state(const bsk_ctx* ctx, int* cut_reached, uint64_t* records);

/* ---- Duplicate (bigseqkit/duplicate.go:31-43, bigseqkit-lib/duplicate.go:13-30): every record Times times, copies
 * adjacent. */
int bsk_duplicate_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, void* stream,
                      bsk_out* out);

/* ---- RmDup (RmDupPrepare + GroupByKey + RmDupCheck, bigseqkit-lib/rmdup.go:23-242):
 * duplicates are global, so ONE call must see the whole input of a rank; the first
 * record of every subject (file order) survives. */
int bsk_rmdup_run(bsk_ctx* ctx, const void* shard, size_t n, int on_device, int format, int64_t pid, void* stream,
                  bsk_out* out);
/* RmDupCheck.After() (bigseqkit-lib/rmdup.go:244-279): writes what the runs of this context accumulated for
 * -d (--dup-seqs-file: text of the removed records) and -D (--dup-num-file: "<n>\t<id>, <id>, ...") to
 * <file>/<device index>, nothing when no record was removed.  bsk_destroy() calls it if the caller did not. */
int bsk_rmdup_finish(bsk_ctx* ctx);

/* ---- rmdup across ranks (one process per GPU).  Duplicates are global, so the reference shuffles whole records
 * with GroupByKey (bigseqkit/rmdup.go:97).  Here a record travels as a 24-byte tuple
 *     (XXH64 key, second XXH64 with another seed, global record index)
 * to its owner rank = key % world; the owner keeps the lowest global index of every key (first in file order,
 * PARITY.md Q10) and answers one keep byte per tuple; equal keys with different second keys raise
 * BSK_ERR_UNSUPPORTED instead of a guess.  The caller runs the collectives between the phases
 * (bigseqkit_amd/dist.py: all_gather of counts, all_to_all_single of tuples, all_to_all_single of keep bytes):
 *   keys    : record table + both keys of the HBM-resident shard            -> *n_records
 *   pack    : tuples bucketed by owner into d_send (u64[3 * n_records]), counts[world] on the host;
 *             base_index = number of records on lower ranks
 *   resolve : owner side, d_tuples = the m tuples received (u64[3 * m])       -> d_keep (u8[m], 1 = first of its key)
 *   emit    : d_reply (u8[n_records]) = keep bytes in the order of d_send    -> survivors of this shard, file order
 * keys ... emit must run on the same context without another run in between (it holds the record table). */
int bsk_rmdup_dist_keys(bsk_ctx* ctx, const void* d_shard, size_t n, int format, void* stream, uint64_t* n_records);
int bsk_rmdup_dist_pack(bsk_ctx* ctx, uint64_t base_index, int world, void* d_send, uint64_t* counts, void* stream);
int bsk_rmdup_dist_resolve(bsk_ctx* ctx, const void* d_tuples, uint64_t m, void* d_keep, void* stream);
int bsk_rmdup_dist_emit(bsk_ctx* ctx, const void* d_send, const void* d_reply, uint64_t base_index, void* stream,
                        bsk_out* out);
/* The same two phases with the survivor's identity (round 5): _resolve_ex also writes d_survivor (u64[m]: the global index of
 * the record that survives for every tuple's subject); routed back like the keep bytes (d_survivor_reply, u64[n_records] in
 * the order of d_send) it lets _emit_ex compare the BYTES of every duplicate whose survivor lives in the same shard with that
 * survivor's (RmDupCheck's own test, bigseqkit-lib/rmdup.go:193-199; `-s` on FASTQ) -- without the cross-rank check below a
 * difference fails the call and pairs that cross ranks rest on the two keys; with it (bsk_rmdup_dist_x*, which
 * bsk_rmdup_dist_run runs) every pair is compared and _emit_ex only emits.  Either pointer NULL: the plain phases.
 * *local_pairs_verified (may be NULL): how many pairs inside the shard were compared. */
int bsk_rmdup_dist_resolve_ex(bsk_ctx* ctx, const void* d_tuples, uint64_t m, void* d_keep, void* d_survivor, void* stream);
int bsk_rmdup_dist_emit_ex(bsk_ctx* ctx, const void* d_send, const void* d_reply, const void* d_survivor_reply, uint64_t base_index,
                           void* stream, bsk_out* out, uint64_t* local_pairs_verified);

/* ---- RmDupCheck's text comparison across ranks (round 6; bigseqkit-lib/rmdup.go:193-211 compares the subject text of every
 * member of a hash group -- the reference has the text there because GroupByKey, bigseqkit/rmdup.go:97, shuffles whole
 * records).  After the replies of _resolve_ex are back, every duplicate whose survivor lives on ANOTHER rank sends its
 * subject to that rank: a 24-byte request {survivor's global index, offset of the text in the destination's segment,
 * length | local record << 32} and the bytes.  Between the phases the caller runs three all-to-all exchanges:
 *   _xpack    : rank_base[r] = global index of rank r's first record (world + 1 entries); req_counts[r] / byte_counts[r] =
 *               requests / text bytes for rank r; *d_requests / *d_text = the context's send buffers, grouped by destination
 *               [requests, 24 B each, and text to their destinations]
 *   _xcompare : survivor side.  req_from[r] / bytes_from[r] = what arrived from rank r (buffers in rank order);
 *               d_verdict[j] = 1 equal, 0 differs (-i: case-folded)        [verdicts back, the same routes reversed]
 *   _xapply   : d_verdict_back in the order of *d_requests.  Also compares the pairs INSIDE the shard.  *n_flagged = records
 *               of this shard whose text differs from their survivor's (two subjects under one pair of keys); *pairs_compared
 *               = local + cross-rank pairs.  bsk_rmdup_dist_emit[_ex] after it does not compare again.
 * Only when the SUM of n_flagged over the ranks is not zero (about N^2 / 2^129; the tests mask the keys): every rank hands
 * its list (_flagged_get: entries {u64 global index, u64 length, text padded to 8}; call with buf NULL for the size) to
 * every other, and _flagged_settle(concatenation of all ranks' lists, any order) regroups them by TEXT -- the lowest global
 * index of every text survives, as RmDupCheck's map keyed by the subject decides.  bsk_rmdup_dist_run does all of this. */
int bsk_rmdup_dist_xpack(bsk_ctx* ctx, const void* d_send, const void* d_reply, const void* d_survivor_reply, uint64_t base_index,
                         const uint64_t* rank_base, int world, uint64_t* req_counts, uint64_t* byte_counts, void** d_requests, void** d_text,
                         void* stream);
int bsk_rmdup_dist_xcompare(bsk_ctx* ctx, const void* d_requests_in, const uint64_t* req_from, const void* d_text_in,
                            const uint64_t* bytes_from, int world, void* d_verdict, void* stream);
int bsk_rmdup_dist_xapply(bsk_ctx* ctx, const void* d_verdict_back, uint64_t* n_flagged, uint64_t* pairs_compared, void* stream);
int bsk_rmdup_dist_flagged_get(bsk_ctx* ctx, void* buf, size_t cap, size_t* need);
int bsk_rmdup_dist_flagged_settle(bsk_ctx* ctx, const void* all_lists, size_t n_bytes);
/* what the last exchange of this context compared: pairs inside the shard, pairs whose survivor lives on another rank (their
 * text went there), and the records of this shard that were flagged (any pointer may be NULL) */
int bsk_rmdup_dist_stats(const bsk_ctx* ctx, uint64_t* local_pairs, uint64_t* cross_pairs, uint64_t* flagged);

/* ---- collectives behind the C ABI (round 5): RCCL over xGMI, no Python, no torch -----------------------------------------
 * In the reference the driver gets Reduce and GroupByKey from IgnisHPC, in the same binary (bigseqkit/stats.go:91,
 * grep.go:175, rmdup.go:97; the executors from ignisDriver, bigseqkit-cli/helper.go:87-132).  A bsk_comm is one rank's
 * handle on a group of `world` ranks, each with its own GPU and its own bsk_ctx:
 *   one rank per PROCESS : rank 0 calls bsk_comm_unique_id, the host hands the 128 bytes to the other ranks (a file, a
 *                          socket, the launcher's environment), every rank calls bsk_comm_init_rank   (ncclCommInitRank)
 *   all ranks in ONE process, a thread each : bsk_comm_init_all(ndev, devices, comms)                 (ncclCommInitAll);
 *                          devices that repeat (ranks sharing a GPU: RCCL refuses that) get the "local" backend -- the
 *                          same calls through host memory between the threads (tests on a one-GPU box)
 * librccl is loaded at the first of these calls, not with libbsk.so.  Every collective must be entered by ALL ranks.
 * Errors: the code, and bsk_comm_error(comm) (bsk_comm_error(NULL): the calling thread's last failure without a comm). */
typedef struct bsk_comm bsk_comm;
#define BSK_COMM_ID_BYTES 128
int bsk_comm_unique_id(void* id128);
int bsk_comm_init_rank(int world, int rank, const void* id128, int device, bsk_comm** out);
int bsk_comm_init_all(int ndev, const int* devices, bsk_comm** out /* [ndev] */);
int bsk_comm_destroy(bsk_comm* comm);
int bsk_comm_info(const bsk_comm* comm, int* world, int* rank, int* device, int* over_rccl);
const char* bsk_comm_error(const bsk_comm* comm);
int bsk_comm_barrier(bsk_comm* comm, void* stream);
/* in place on `count` device words; op: 0 sum, 1 max, 2 min */
int bsk_comm_allreduce_u64(bsk_comm* comm, void* d_buf, size_t count, int op, void* stream);
/* one word of every rank -> out[world] on the host (record counts, shard and part sizes: Range / Head, bigseqkit/range.go:69-103;
 * FaidxOffset, faidx.go:69-80; the offsets of FileStore's ordered single file, bigseqkit-lib/helper.go:399-429); synchronises */
int bsk_comm_allgather_u64(bsk_comm* comm, uint64_t value, uint64_t* out, void* stream);
/* GrepReduceCount (bigseqkit-lib/grep.go:598-611 through Reduce, bigseqkit/grep.go:175): *inout becomes the sum over ranks */
int bsk_count_allreduce(bsk_comm* comm, uint64_t* inout, void* stream);
/* StatsReduce (bigseqkit-lib/stats.go:128-137 through Reduce, bigseqkit/stats.go:91) + the driver's collect: ONE sum
 * all-reduce of the stats vector (d_vec, or the context's own when NULL) and bsk_stats_collect; only when the reduced vector
 * counts sequence lengths beyond the dense histogram do the ranks exchange their overflow lists and collect again.  Every
 * rank receives the whole map. */
int bsk_stats_collect_reduced(bsk_ctx* ctx, bsk_comm* comm, void* d_vec, void* stream, int64_t* keys, int64_t* vals, size_t cap,
                              size_t* n_out);
/* RmDup over the shards of all ranks in ONE call (GroupByKey, bigseqkit/rmdup.go:97): the four phases above with their
 * collectives in between -- all-gather of the record counts, tuples to their owners by grouped ncclSend / ncclRecv (in
 * rounds of at most 512 MiB per message), one keep byte per tuple back the same way.  `out`: the survivors of THIS rank's
 * shard in file order; the concatenation over the ranks equals the single-GPU output. */
int bsk_rmdup_dist_run(bsk_ctx* ctx, bsk_comm* comm, const void* d_shard, size_t n, int format, void* stream, bsk_out* out);

/* host-side self-test of the position-reporting regular-expression matcher (custom --id-regexp, locate -r):
 * leftmost-first match at or after `from`; caps4 = {match start, match end, group-1 start, group-1 end} (0xFFFFFFFF:
 * group 1 did not take part).  1 = match, 0 = none, -1 = expression rejected (bsk_global_error) */
int bsk_selftest_regex_find(const char* expr, const uint8_t* text, size_t n, size_t from, uint32_t* caps4, uint32_t* ngroups);

/* ---- FileStore / StoreFASTXN  (bigseqkit-lib/helper.go:378-460 NewFileStore; bigseqkit/helper.go:186-195 StoreFASTX[N]) ----
 * merge != 0: ONE file at `path`, the parts (partitions) in the order of their numbers whatever the order of the calls --
 * the reference passes an MPI token from executor to executor (helper.go:418-436), here a part that comes before its
 * turn waits in host memory.  merge == 0: directory `path` with one file part%05d per partition (SaveAsTextFile).
 * Parts must be numbered 0, 1, 2, ... without gaps for the single file to grow while the parts arrive. */
typedef struct bsk_store bsk_store;
int bsk_store_open(const char* path, int merge, bsk_store** out);
const char* bsk_store_error(const bsk_store* s);
/* the output of an operator call (device memory of `ctx`), copied to the host in 64 MiB pieces through two pinned
 * buffers -- the copy of a piece runs while the piece before it is written */
int bsk_store_put(bsk_store* s, bsk_ctx* ctx, uint64_t part, const bsk_out* out);
/* on != 0, before the first put: what is put stays text, what is written is BGZF.  bsk_store_put compresses every piece
 * of the drain on the device in front of its D2H copy, bsk_store_put_host on host threads; parts are appended in order as
 * before (one that arrives early waits compressed).  bsk_store_close ends the single file with ONE EOF block; in directory
 * mode the files are named part%05d.gz and each ends with its own.  on == 0: nothing changes, names included.
 * on == 2: BGZF as with 1, but no file gets an EOF block -- the file is a piece of a larger one, whose writer appends the one
 * EOF block behind the last piece (the spools of the command line's --devices --merge). */
int bsk_store_set_bgzf(bsk_store* s, int on);
int bsk_store_put_host(bsk_store* s, uint64_t part, const void* data, size_t n);
int bsk_store_close(bsk_store* s, uint64_t* total_bytes); /* also frees s */
/* Call(partition) + FileStore for a partition in HOST memory (best: pinned, bsk_host_alloc): record-aligned chunks of
 * 256 MiB (BSK_STAGE_BYTES) through two device buffers -- H2D of chunk i+1, the kernels of chunk i, and D2H + write of
 * the output of chunk i-1 overlap (three streams and a writer thread).  seq, grep, locate, subseq, translate, fq2fa,
 * duplicate are chunked; rmdup, rename, sort, grep -C / --delete-matched see the whole partition (their output is still
 * drained in pieces).  out_bytes / out_records may be NULL. */
int bsk_run_to_store(bsk_ctx* ctx, const void* host_shard, size_t n, int format, int64_t pid, bsk_store* s, uint64_t part,
                     uint64_t* out_bytes, uint64_t* out_records);

/* ---- synthetic inputs (bench + tests only) --------
 * Deterministic, counter-based: byte k of record i depends on (seed, i, k)
 * only, so any shard can be produced on the host or directly in HBM. */
#define BSK_SYNTH_FASTQ150 0 /* 317 B/record                          */
#define BSK_SYNTH_FASTA1K 1  /* 1027 B/record, 60-column lines        */
#define BSK_SYNTH_FASTA5K_CDS 2
#define BSK_SYNTH_FASTA5K_VAR 3 /* the same CDS records with unpadded numbers in the header and 1 % of them 3 bases shorter /
                                 * longer: records of several sizes (bsk_synth_record_bytes = 0, bsk_synth_offset) */
#define BSK_SYNTH_FLAG_MOTIF 1u /* C3: plant ACGTTGCAAGCT / its revcomp */
#define BSK_SYNTH_FLAG_DUPS 2u  /* C5: 20 % sequence duplicates         */
size_t bsk_synth_record_bytes(int kind);
/* file offset of record `record` (== bytes of the records below it); n bytes from there: bsk_synth_host / _device */
uint64_t bsk_synth_offset(int kind, uint64_t record);
/* fill dst[0..n) with the bytes [first_record*record_bytes, ...+n) of the
 * synthetic file; n need not be a whole number of records */
int bsk_synth_host(int kind, uint64_t seed, unsigned flags, uint64_t first_record, uint8_t* dst, size_t n);
int bsk_synth_device(int kind, uint64_t seed, unsigned flags, uint64_t first_record, void* d_dst, size_t n, int device,
                     void* stream);

/* ---- timing helper for bench.py: HIP events on the stream the kernels use */
int bsk_event_create(void** ev);
int bsk_event_record(void* ev, void* stream);
int bsk_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on stop */
int bsk_event_destroy(void* ev);
/* accumulated device time of the dominant kernel of the last run(s), measured
 * with HIP events around each launch when profiling is enabled */
int bsk_profile_enable(bsk_ctx* ctx, int on);
int bsk_profile_read(bsk_ctx* ctx, const char* kernel, double* total_ms, uint64_t* launches);
int bsk_profile_reset(bsk_ctx* ctx);
/* all timed stages of the context: "name=total_ms/launches;..." (NUL-terminated) */
int bsk_profile_dump(bsk_ctx* ctx, char* buf, size_t cap);

/* ---- device self tests used by tests/ (-m gpu) ---------------------------- */
int bsk_selftest_scan(int use_dpp, const uint32_t* in64, uint32_t* out64);
/* the two 64-bit keys (XXH64 seed 0, and the second key of csrc/hash_dev.hpp) of every record of the shard of the last
 * bsk_rmdup_dist_keys call, in record order.  k2 == NULL: k1 alone -- after a bsk_rmdup_run (-s on FASTQ, keys verified by
 * bytes) that is the chain-free GROUPING key of csrc/hash_dev.hpp, which the tests restate in Python */
int bsk_selftest_rmdup_keys(bsk_ctx* ctx, uint64_t* k1, uint64_t* k2, size_t cap, size_t* n_out);
/* streaming read of d_buf[0..n) with k_stats' tile/queue pattern and no per-byte work:
 * the read ceiling of that pattern and the FETCH_SIZE calibration run */
int bsk_selftest_stream_read(const void* d_buf, size_t n, int reps, int blocks_per_cu, float* avg_ms);

#ifdef __cplusplus
}
#endif
#endif /* BSK_H */
