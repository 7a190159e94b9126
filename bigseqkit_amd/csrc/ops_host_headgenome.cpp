// Host side of `head-genome` (HeadGenome.Call, bigseqkit-lib/head_genome.go:39-111; PARITY.md HEADG): the search for the cut
// over growing windows of a device-resident shard, and the kept prefix through seq's size -> scan -> emit flow.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/bsk.h"
#include "ctx.hpp"
#include "ops_headgenome.hpp"
#include "ops_host.hpp"
#include "ops_host_internal.hpp"
#include "ops_seq.hpp"

namespace bsk {

// The first window and its growth.  Every window costs a fixed handful of launches and two or three synchronisations
// whatever its size, so the first one is large enough to hold a bacterial genome and each next one is four times the last:
// a shard of 2 GB that is never cut is read in five windows.  Neither number has been measured (DESIGN f8).
constexpr uint64_t HG_WINDOW_BYTES = 16ull << 20;
constexpr uint64_t HG_WINDOW_GROWTH = 4;

void validate_head_genome_opts(bsk_ctx* c) {
    const Options& o = c->opts;
    c->alphabet = alphabet_from_seqtype(o.cs("SeqType"));
    // getFlagPositiveInt (cli/helper.go:250-257); from the library as well: the loop as written re-arms its "second sequence"
    // state on a count of 0, and that is not meant (PARITY HEADG)
    if (o.i("MiniCommonWords") < 1) throw OptError("value of flag --mini-common-words should be greater than 0");
    check_id_regexp(c);
}

void head_genome_reset(bsk_ctx* c) { c->hg = bsk_ctx::HeadGenomeState(); }

// the prefix: stringutil.Split(Desc, "\t ") of the header text h[0, n) (marker excluded); Desc as parseHeadIDAndDesc yields it
// (helper.go:329-369; text_dev.hpp id_span_of / desc_of are the device twins), empty unless the default --id-regexp is in use
static void prefix_words(bsk_ctx::HeadGenomeState* S, const uint8_t* h, size_t n, int id_mode) {
    S->words.clear();
    S->off.assign(1, 0);
    S->have_prefix = true;
    S->uploaded = false;
    if (id_mode != 0) return;
    size_t il = n;
    const void* sp = memchr(h, ' ', n);
    const void* tb = memchr(h, '\t', n);
    if (sp && (const uint8_t*)sp > h) il = (size_t)((const uint8_t*)sp - h);
    else if (tb && (const uint8_t*)tb > h) il = (size_t)((const uint8_t*)tb - h);
    if (il >= n) return;
    size_t j = il + 1;
    for (; j < n; j++) {  // (the skip-two loop, as written)
        if (h[j] == ' ' || h[j] == '\t') j++;
        else break;
    }
    while (j < n) {
        while (j < n && (h[j] == ' ' || h[j] == '\t')) ++j;
        const size_t w0 = j;
        while (j < n && h[j] != ' ' && h[j] != '\t') ++j;
        if (j > w0) {
            S->words.append((const char*)h + w0, j - w0);
            S->off.push_back((uint32_t)S->words.size());
        }
    }
}

static int upload_prefix(bsk_ctx* c, hipStream_t st) {
    bsk_ctx::HeadGenomeState& S = c->hg;
    if (S.uploaded) return BSK_OK;
    int rc = grow(c, &c->d_hg_words, &c->hg_words_cap, S.words.size(), 64);
    if (rc == BSK_OK) rc = grow(c, &c->d_hg_off, &c->hg_off_cap, S.off.size(), 16);
    if (rc != BSK_OK) return rc;
    if (!S.words.empty()) HIP_TRYX(c, hipMemcpyAsync(c->d_hg_words, S.words.data(), S.words.size(), hipMemcpyHostToDevice, st));
    HIP_TRYX(c, hipMemcpyAsync(c->d_hg_off, S.off.data(), S.off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRYX(c, hipStreamSynchronize(st));
    S.uploaded = true;
    return BSK_OK;
}

// the kept prefix d_buf[0, kept) as `seq` without options prints it: Format(LineWidth), FASTQ with LineWidth 0
static int emit_kept(bsk_ctx* c, const uint8_t* d_buf, size_t kept, int format, bool table_is_kept, hipStream_t st, bsk_out* out) {
    const bool fastq = format == BSK_FORMAT_FASTQ;
    Timed tm(c, "hg_emit", st);
    if (!table_is_kept) {
        HIP_TRYX(c, hipMemsetAsync(c->d_status, 0, 8 * sizeof(uint64_t), st));
        const int rc = build_index(c, d_buf, kept, format, st);
        if (rc != BSK_OK) return rc;
    }
    if (c->table.n == 0) return empty_result(c, out);
    SeqParams P = format_params(c, fastq);
    P.buf_end = d_buf + kept;
    TextTableH tt{nullptr, nullptr, nullptr};
    int rc = prepare_text(c, d_buf, format, st, &tt);
    if (rc != BSK_OK) return rc;
    P.text_w = tt.text_w; P.lin_off = tt.lin_off; P.lin = tt.lin;
    rc = ensure_record_scratch(c);
    if (rc != BSK_OK) return rc;
    HIP_TRYX(c, launch_seq_size(d_buf, c->table, P, c->d_out_len, c->d_status, st));
    return emit_sized(c, d_buf, kept, P, st, out, /*allow_slices=*/true);
}

static int find_cut(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, size_t* kept_out, bool* table_is_kept) {
    const bool fastq = format == BSK_FORMAT_FASTQ;
    const int id_mode = id_mode_of(c);
    const uint32_t min_words = (uint32_t)std::min<int64_t>(c->opts.i("MiniCommonWords"), 0x7FFFFFFF);
    bsk_ctx::HeadGenomeState& S = c->hg;
    uint64_t w = HG_WINDOW_BYTES;
    if (const char* e = c->tune.get("head_genome_window")) w = strtoull(e, nullptr, 10);  // (0: one window, the whole shard)
    if (!c->d_hg_res) HIP_TRYX(c, hipMalloc((void**)&c->d_hg_res, HG_WORDS * sizeof(uint64_t)));
    uint64_t res[HG_WORDS];
    uint64_t pos = 0;
    *table_is_kept = false;
    for (;;) {
        uint64_t wlen = (w == 0 || n - pos <= w) ? n - pos : w;
        if (pos + wlen < n && fastq) {
            // a window that does not reach the end of the shard ends on a record start: the 4-line rule of the staging code
            HIP_TRYX(c, launch_hg_fastq_start(d_buf, n, pos + wlen, c->d_hg_res, st));
            HIP_TRYX(c, hipMemcpyAsync(&res[HG_END], c->d_hg_res + HG_END, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
            HIP_TRYX(c, hipStreamSynchronize(st));
            wlen = (res[HG_END] > pos && res[HG_END] <= n ? res[HG_END] : n) - pos;
        }
        const bool last = pos + wlen == n;
        {
            Timed tm(c, "hg_window_index", st);
            const int rc = build_index(c, d_buf + pos, wlen, format, st);
            if (rc != BSK_OK) return rc;
        }
        c->hg_indexed_bytes += wlen;
        // FASTA: the last record of such a window may be open -- it is dropped and opens the next window
        const uint64_t n_use = (last || fastq) ? c->table.n : (c->table.n ? c->table.n - 1 : 0);
        if (n_use == 0) {
            if (!last) {  // a record larger than the window just makes the window grow
                w = w > (1ull << 58) ? 0 : w * HG_WINDOW_GROWTH;
                continue;
            }
            uint64_t status = 0;
            HIP_TRYX(c, hipMemcpyAsync(&status, c->d_status, sizeof status, hipMemcpyDeviceToHost, st));
            HIP_TRYX(c, hipStreamSynchronize(st));
            if (status) return kernel_error_to_status(c, status);
            *kept_out = n;
            *table_is_kept = pos == 0;
            return BSK_OK;
        }
        uint64_t skip = HG_NONE, first_cmp = 0;
        if (!S.have_prefix) {  // the first record of the input: its words are the prefix, it is not compared
            uint64_t s0 = 0;
            uint32_t lh = 0;
            HIP_TRYX(c, hipMemcpyAsync(&s0, c->table.start, sizeof s0, hipMemcpyDeviceToHost, st));
            HIP_TRYX(c, hipMemcpyAsync(&lh, c->table.l_head, sizeof lh, hipMemcpyDeviceToHost, st));
            HIP_TRYX(c, hipStreamSynchronize(st));
            std::vector<uint8_t> head(lh > 0 ? lh - 1 : 0);
            if (!head.empty()) HIP_TRYX(c, hipMemcpy(head.data(), d_buf + pos + s0 + 1, head.size(), hipMemcpyDeviceToHost));
            prefix_words(&S, head.data(), head.size(), id_mode);
            skip = 0;
            first_cmp = 1;
        }
        int rc = upload_prefix(c, st);
        if (rc == BSK_OK) rc = grow(c, &c->d_hg_counts, &c->hg_counts_cap, n_use, n_use / 8 + 256);
        if (rc != BSK_OK) return rc;
        {
            Timed tm(c, "hg_verdict", st);
            HIP_TRYX(c, hipMemsetAsync(c->d_hg_res, 0xFF, 2 * sizeof(uint64_t), st));  // HG_CUT, HG_NODESC := HG_NONE
            const HgPrefix P{c->d_hg_words, c->d_hg_off, (uint32_t)(S.off.size() - 1)};
            HIP_TRYX(c, launch_hg_counts(d_buf + pos, wlen, c->table, n_use, id_mode, P, skip, c->d_hg_counts, st));
            HIP_TRYX(c, launch_hg_cut(c->d_hg_counts, n_use, first_cmp, S.n1 >= 0 ? 1 : 0, (uint32_t)std::max<int64_t>(S.n1, 0), min_words,
                                      c->d_hg_res, st));
            HIP_TRYX(c, launch_hg_finish(d_buf + pos, c->table, c->d_hg_counts, n_use, first_cmp, id_mode, c->d_hg_res, st));
        }
        HIP_TRYX(c, hipMemcpyAsync(res, c->d_hg_res, sizeof res, hipMemcpyDeviceToHost, st));
        rc = ctl_readback(c, st);  // (the synchronisation of the window: its verdict and the status word of its index pass)
        if (rc != BSK_OK) return rc;
        if (c->status_word()) return kernel_error_to_status(c, c->status_word());
        const uint64_t keep = std::min(res[HG_CUT], n_use);
        if (res[HG_NODESC] < keep) {  // head_genome.go:68-70: the lowest kept record without a description
            std::string id((size_t)res[HG_ND_IDLEN], '\0');
            if (!id.empty())
                HIP_TRYX(c, hipMemcpy(&id[0], d_buf + pos + res[HG_ND_START] + 1 + res[HG_ND_IDOFF], id.size(), hipMemcpyDeviceToHost));
            c->set_error("no description: " + id);
            return BSK_ERR_FORMAT;
        }
        if (S.n1 < 0 && res[HG_N1] != HG_NONE) S.n1 = (int64_t)res[HG_N1];
        S.records += keep;
        if (res[HG_CUT] < n_use) {
            S.cut = true;
            *kept_out = pos + res[HG_CUT_BYTE];
            return BSK_OK;
        }
        if (last) {
            *kept_out = n;
            *table_is_kept = pos == 0;  // one window held the shard: its table is the table of what is kept
            return BSK_OK;
        }
        pos = fastq ? pos + wlen : pos + res[HG_CUT_BYTE];  // (FASTA: where the dropped record begins)
        w = w > (1ull << 58) ? 0 : w * HG_WINDOW_GROWTH;
    }
}

int head_genome_run_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, bsk_out* out) {
    out->d_data = nullptr;
    out->len = 0;
    out->records = 0;
    if (c->hg.cut || n == 0) return BSK_OK;  // a shard behind the cut produces nothing; an empty input is an empty result
    // (a call that fails leaves the state as it found it: the multi-line FASTQ reader runs the shard a second time)
    const bsk_ctx::HeadGenomeState before = c->hg;
    size_t kept = 0;
    bool table_is_kept = false;
    int rc = find_cut(c, d_buf, n, format, st, &kept, &table_is_kept);
    if (rc == BSK_OK && kept > 0) rc = emit_kept(c, d_buf, kept, format, table_is_kept, st, out);
    if (rc != BSK_OK) c->hg = before;
    return rc;
}

}  // namespace bsk
