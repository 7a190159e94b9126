// `faidx -d`: the planner and the batch steps of fai_fetch.hpp bound to a Faidx context -- its queries and options in, the
// spans of a batch read from the file, the tiles on the device (ops_faidx_fetch.hip) or on one host lane.  PARITY.md FAIX.
#include "fai_fetch.hpp"

#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <cstdlib>
#include <thread>

#include "bgzf_inflate_dev.hpp"
#include "ops_bgzf.hpp"
#include "ops_faidx_fetch.hpp"
#include "ops_host_internal.hpp"
#include "regex_nfa.hpp"

namespace bsk {

namespace {

// what partition_alphabet reads of a shard that is the whole file: the head it samples
uint64_t alphabet_head_bytes(const bsk_ctx* c) {
    const int64_t thr = c->opts.ci("AlphabetGuessSeqLength");
    return (uint64_t)std::max<int64_t>(thr, 10000) * 2 + 65536;
}

// spans of a batch into buf (fai::layout): pieces of at most 4 MiB, handed to `threads` readers
int read_spans(bsk_ctx* c, int fd, const fai::Batch& b, const fai::Layout& L, uint8_t* buf, int threads) {
    struct Piece { uint64_t off, at, n; };
    std::vector<Piece> pieces;
    constexpr uint64_t PIECE = 4ull << 20;
    for (size_t k = 0; k < b.spans.size(); ++k)
        for (uint64_t o = b.spans[k].lo; o < b.spans[k].hi; o += PIECE)
            pieces.push_back({o, L.slot[k] + (o - b.spans[k].lo), std::min(PIECE, b.spans[k].hi - o)});
    std::atomic<size_t> next{0};
    std::atomic<int> bad{0};
    auto work = [&] {
        for (size_t i = next.fetch_add(1); i < pieces.size(); i = next.fetch_add(1)) {
            uint64_t done = 0;
            while (done < pieces[i].n) {
                const ssize_t k = pread(fd, buf + pieces[i].at + done, pieces[i].n - done, (off_t)(pieces[i].off + done));
                if (k < 0 && errno == EINTR) continue;
                if (k <= 0) { bad.store(k < 0 ? errno : -1); return; }  // (a file shorter than the index was planned for)
                done += (uint64_t)k;
            }
        }
    };
    const size_t nt = std::min<size_t>(threads > 0 ? (size_t)threads : 4, pieces.size());
    if (nt <= 1) work();
    else {
        std::vector<std::thread> pool;
        for (size_t t = 0; t < nt; ++t) pool.emplace_back(work);
        for (auto& t : pool) t.join();
    }
    if (bad.load()) {
        c->set_error(bad.load() > 0 ? std::string("faidx -d: reading the sequence file failed: ") + strerror(bad.load())
                                    : std::string("faidx -d: the sequence file is shorter than the size the plan was made for"));
        return BSK_ERR_INVALID_ARG;
    }
    return BSK_OK;
}

// the complement table of the whole-file path (PARITY.md ALPHA, the file as one partition): the context's alphabet, or the
// one guessed from the head of the file as partition_alphabet guesses it from the head of the shard
void complement_of(bsk_ctx* c, const fai::Plan& plan, const fai::Batch& b, const fai::Layout& L, const uint8_t* buf, uint8_t comp[256]) {
    Alphabet ab = c->alphabet;
    if (ab == AB_NONE) {
        const int64_t thr = c->opts.ci("AlphabetGuessSeqLength");
        const uint64_t want = plan.alphabet_bytes;  // == min(alphabet_head_bytes, file size): span 0 begins with it
        const std::vector<uint8_t> h(buf + L.slot[0], buf + L.slot[0] + want);
        const int format = plan.fastq ? BSK_FORMAT_FASTQ : BSK_FORMAT_FASTA;
        std::vector<uint8_t> s = head_first_seq(h, format, (size_t)std::max<int64_t>(thr, 1));
        if (thr == 0) s = head_first_seq(h, format, h.size());
        ab = guess_alphabet_less_conservatively(s.data(), s.size(), thr);
        (void)b;
    }
    complement_table(ab, comp);
}

bool batch_has_minus(const fai::Plan& plan, const fai::Batch& b) {
    for (uint32_t k = b.hit0; k < b.hit1; ++k)
        if (plan.hits[k].minus) return true;
    return false;
}

thread_local uint64_t g_last_info[8] = {0};  // what the last fetch of this thread did (the precedent of bsk_gzip_last_plan)

void note_info(const fai::Batch& b, const fai::Tables& T, uint64_t blocks) {
    const uint64_t v[8] = {b.hit1 - b.hit0, b.spans.size(), b.read_bytes, blocks, fai::FETCH_T, T.tiles.size(), T.out_bytes, 0};
    memcpy(g_last_info, v, sizeof v);
}

int check_batch(bsk_ctx* c, const fai::Plan& plan, size_t batch) {
    if (batch >= plan.batches.size()) {
        c->set_error("libbsk: faidx fetch: the plan has " + std::to_string(plan.batches.size()) + " batches");
        return BSK_ERR_INVALID_ARG;
    }
    if (plan.batches[batch].tiles >= (1ull << 32)) {
        c->set_error("faidx -d: a batch of 2^32 tiles or more; lower BSK_FAIDX_FETCH_BYTES");
        return BSK_ERR_UNSUPPORTED;
    }
    return BSK_OK;
}

}  // namespace

void fai_last_info(uint64_t out[8]) { memcpy(out, g_last_info, sizeof g_last_info); }

int fai_plan_build(bsk_ctx* c, const std::string& fai_text, uint64_t file_size, int format, uint64_t budget, fai::Plan* plan) {
    const Options& o = c->opts;
    if (c->features.empty() && c->regexes.empty()) {
        c->set_error("faidx -d: the context has no regions (Regions, RegionFile)");
        return BSK_ERR_OPTS;
    }
    if (id_mode_of(c) != 0) {
        c->set_error("faidx -d: the names of an index are parseHeadID's (the default ID rule) and cannot restate --id-regexp / --id-ncbi; "
                     "run without -d");
        return BSK_ERR_OPTS;
    }
    std::string err;
    int rc = fai::parse_rows(fai_text, file_size, format, o.b("FullHead"), plan, &err);
    if (rc != 0) { c->set_error(err); return rc; }
    fai::Options fo;
    for (const bsk_ctx::Feature& f : c->features) fo.queries.push_back(fai::Query{f.name_lower, f.suffix, f.s, f.e, f.minus});
    if (!c->regexes.empty())
        fo.regex = [c](const std::string& id) {
            for (const RegexProgram& p : c->regexes)
                if (regex_match(p, reinterpret_cast<const uint8_t*>(id.data()), id.size())) return true;
            return false;
        };
    fo.ignore_case = o.b("IgnoreCase");
    fo.full_head = o.b("FullHead");
    const int64_t lw = o.ci("LineWidth");
    fo.line_width = lw > 0 ? (uint32_t)lw : 0;
    if (budget == 0) {
        const char* e = getenv("BSK_FAIDX_FETCH_BYTES");
        budget = e && atoll(e) > 0 ? (uint64_t)atoll(e) : fai::DEFAULT_BUDGET;
    }
    fo.budget = budget;
    fo.alphabet_bytes = c->alphabet == AB_NONE ? alphabet_head_bytes(c) : 0;
    rc = fai::make_plan(fo, plan, &err);
    if (rc != 0) { c->set_error(err); return rc; }
    return BSK_OK;
}

namespace {

// ---- a BGZF sequence file: spans of the text come from runs of whole blocks, named by the block table
bool pread_all(int fd, void* p, size_t n, uint64_t off) {
    size_t done = 0;
    while (done < n) {
        const ssize_t k = pread(fd, (uint8_t*)p + done, n - done, (off_t)(off + done));
        if (k < 0 && errno == EINTR) continue;
        if (k <= 0) return false;
        done += (size_t)k;
    }
    return true;
}

// header and trailer of the block at `off`: BSIZE and ISIZE, no inflate.  false: no whole BGZF block begins there
bool block_sizes(int fd, uint64_t off, uint64_t fsize, uint32_t* bsize, uint32_t* isize) {
    uint8_t head[12 + 65535];
    size_t n = (size_t)std::min<uint64_t>(fsize - off, 64);
    if (off >= fsize || !pread_all(fd, head, n, off)) return false;
    bgzf::BlockHeader h{0, 0};
    int rc = bgzf::parse_header(head, n, &h);
    if (rc == -1) {
        n = (size_t)std::min<uint64_t>(fsize - off, sizeof head);
        if (!pread_all(fd, head, n, off)) return false;
        rc = bgzf::parse_header(head, n, &h);
    }
    if (rc != 1 || h.bsize < 12u + h.xlen + 8u || off + h.bsize > fsize) return false;
    uint8_t t[4];
    if (!pread_all(fd, t, 4, off + h.bsize - 4)) return false;
    *bsize = h.bsize;
    *isize = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
    return *isize <= bgzf::MAX_ISIZE;
}

uint64_t file_bytes(int fd) {
    const off_t n = lseek(fd, 0, SEEK_END);
    return n < 0 ? 0 : (uint64_t)n;
}

// The blocks that hold the span, each checked against the table: entry k lands on a block header, the block ends where entry
// k + 1 begins and holds the bytes that lie between their text offsets.  *cend / *uend: where the run ends in the file / text
int span_blocks(bsk_ctx* c, int fd, const fai::Gzi& g, uint64_t fsize, const fai::Span& sp, size_t* first, size_t* last, uint64_t* cend,
                uint64_t* uend) {
    fai::gzi_blocks(g, sp.lo, sp.hi, first, last);
    for (size_t k = *first; k <= *last; ++k) {
        uint32_t bsize = 0, isize = 0;
        const std::string entry = "faidx -d: block table entry " + std::to_string(k) + " (compressed offset " + std::to_string(g.coff[k]) +
                                  ", text offset " + std::to_string(g.uoff[k]) + ")";
        if (!block_sizes(fd, g.coff[k], fsize, &bsize, &isize)) {
            c->set_error(entry + " does not land on a block header of this file; build the table again");
            return BSK_ERR_FORMAT;
        }
        if (k + 1 < g.coff.size() && (g.coff[k] + bsize != g.coff[k + 1] || g.uoff[k] + isize != g.uoff[k + 1])) {
            c->set_error(entry + ": the block holds " + std::to_string(bsize) + " bytes and " + std::to_string(isize) +
                         " bytes of text, which contradicts the next entry; build the table again");
            return BSK_ERR_FORMAT;
        }
        *cend = g.coff[k] + bsize;
        *uend = g.uoff[k] + isize;
    }
    if (sp.hi > *uend) {
        c->set_error("faidx -d: the block table ends at text offset " + std::to_string(*uend) + ", the plan reads up to " + std::to_string(sp.hi));
        return BSK_ERR_FORMAT;
    }
    return BSK_OK;
}

int parse_table(bsk_ctx* c, const void* gzi, size_t gzi_len, fai::Gzi* g) {
    std::string err;
    const int rc = fai::gzi_parse((const uint8_t*)gzi, gzi_len, g, &err);
    if (rc != 0) c->set_error(err);
    return rc;
}

}  // namespace

int fai_gzi_build(int fd, std::string* image, uint64_t* text_size, std::string* err) {
    const uint64_t fsize = file_bytes(fd);
    fai::Gzi g;
    g.coff.clear(); g.uoff.clear();
    uint64_t off = 0, text = 0;
    while (off < fsize) {
        uint32_t bsize = 0, isize = 0;
        if (!block_sizes(fd, off, fsize, &bsize, &isize)) {
            *err = "libbsk: bgzf: block " + std::to_string(g.coff.size()) + " at offset " + std::to_string(off) + " of the file is no whole BGZF block";
            return BSK_ERR_FORMAT;
        }
        g.coff.push_back(off);
        g.uoff.push_back(text);
        off += bsize;
        text += isize;
    }
    if (g.coff.empty()) { *err = "libbsk: bgzf: an empty file has no blocks"; return BSK_ERR_FORMAT; }
    if (image) *image = fai::gzi_image(g);
    if (text_size) *text_size = text;
    return BSK_OK;
}

int fai_gzi_text_size(int fd, const void* gzi, size_t gzi_len, uint64_t* text_size, std::string* err) {
    fai::Gzi g;
    int rc = fai::gzi_parse((const uint8_t*)gzi, gzi_len, &g, err);
    if (rc != 0) return rc;
    uint32_t bsize = 0, isize = 0;
    if (!block_sizes(fd, g.coff.back(), file_bytes(fd), &bsize, &isize)) {
        *err = "faidx -d: block table entry " + std::to_string(g.coff.size() - 1) + " (compressed offset " + std::to_string(g.coff.back()) +
               ") does not land on a block header of this file; build the table again";
        return BSK_ERR_FORMAT;
    }
    *text_size = g.uoff.back() + isize;
    return BSK_OK;
}

namespace {

// the spans of a batch of a BGZF file into the host buffer: the run of blocks of every span, inflated on the host lane
int read_spans_bgzf_host(bsk_ctx* c, int fd, const fai::Gzi& g, const fai::Batch& b, const fai::Layout& L, uint8_t* buf, uint64_t* blocks) {
    const uint64_t fsize = file_bytes(fd);
    for (size_t k = 0; k < b.spans.size(); ++k) {
        size_t first = 0, last = 0;
        uint64_t cend = 0, uend = 0;
        int rc = span_blocks(c, fd, g, fsize, b.spans[k], &first, &last, &cend, &uend);
        if (rc != BSK_OK) return rc;
        std::vector<uint8_t> comp((size_t)(cend - g.coff[first])), text((size_t)(uend - g.uoff[first]) + 1);
        if (!pread_all(fd, comp.data(), comp.size(), g.coff[first])) { c->set_error("faidx -d: reading the sequence file failed"); return BSK_ERR_INVALID_ARG; }
        size_t n = 0;
        std::string err;
        rc = bgzf_inflate_host(comp.data(), comp.size(), text.data(), text.size(), &n, 1, err);
        if (rc != BSK_OK) { c->set_error(err); return rc; }
        if (n != uend - g.uoff[first]) { c->set_error("faidx -d: the blocks of a span hold another number of bytes than the block table says"); return BSK_ERR_FORMAT; }
        memcpy(buf + L.slot[k], text.data() + (b.spans[k].lo - g.uoff[first]), (size_t)(b.spans[k].hi - b.spans[k].lo));
        *blocks += last - first + 1;
    }
    return BSK_OK;
}

// ... into the device buffer: every run of blocks through the range load of PARITY BGZF "workers" (every refusal of a BGZF
// block, CRC included), the span copied to its slot on the device
int read_spans_bgzf_device(bsk_ctx* c, int fd, const fai::Gzi& g, const fai::Batch& b, const fai::Layout& L, uint8_t* d_buf, int threads,
                           hipStream_t st, uint64_t* blocks) {
    const uint64_t fsize = file_bytes(fd);
    for (size_t k = 0; k < b.spans.size(); ++k) {
        size_t first = 0, last = 0;
        uint64_t cend = 0, uend = 0;
        int rc = span_blocks(c, fd, g, fsize, b.spans[k], &first, &last, &cend, &uend);
        if (rc != BSK_OK) return rc;
        void *base = nullptr, *d_text = nullptr;
        size_t n = 0;
        std::string err;
        rc = bgzf_shard_load(fd, g.coff[first] << 16, cend << 16, c->device, threads, &base, &d_text, &n, err);
        if (rc != BSK_OK) { c->set_error(err); return rc; }
        hipError_t e = hipSuccess;
        if (n != uend - g.uoff[first]) rc = BSK_ERR_FORMAT;
        else {
            e = hipMemcpyAsync(d_buf + L.slot[k], (const uint8_t*)d_text + (b.spans[k].lo - g.uoff[first]), (size_t)(b.spans[k].hi - b.spans[k].lo),
                               hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
        }
        (void)hipFree(base);
        if (rc != BSK_OK) { c->set_error("faidx -d: the blocks of a span hold another number of bytes than the block table says"); return rc; }
        if (e != hipSuccess) { c->set_error(std::string("faidx -d: copying a span: ") + hipGetErrorString(e)); return BSK_ERR_HIP; }
        *blocks += last - first + 1;
    }
    return BSK_OK;
}

}  // namespace

int fai_fetch_host(bsk_ctx* c, int fd, const fai::Plan& plan, size_t batch, std::string* text, const void* gzi, size_t gzi_len) {
    int rc = check_batch(c, plan, batch);
    if (rc != BSK_OK) return rc;
    const fai::Batch& b = plan.batches[batch];
    const fai::Layout L = fai::layout(b);
    std::vector<uint8_t> buf(L.bytes, 0);
    uint64_t blocks = 0;
    if (gzi) {
        fai::Gzi g;
        rc = parse_table(c, gzi, gzi_len, &g);
        if (rc == BSK_OK) rc = read_spans_bgzf_host(c, fd, g, b, L, buf.data(), &blocks);
    } else {
        rc = read_spans(c, fd, b, L, buf.data(), 1);
    }
    if (rc != BSK_OK) return rc;
    fai::Tables T;
    std::string err;
    rc = fai::prepare(plan, batch, L, buf.data(), &T, &err);
    if (rc != 0) { c->set_error(err); return rc; }
    uint8_t comp[256] = {0};
    if (batch_has_minus(plan, b)) complement_of(c, plan, b, L, buf.data(), comp);
    text->assign(T.out_bytes, '\0');
    const uint64_t word = fai::run_host(T, buf.data(), plan.line_width, comp, reinterpret_cast<uint8_t*>(&(*text)[0]));
    note_info(b, T, blocks);
    if (word != fai::FETCH_NO_FAULT) {
        c->set_error(fai::fault_text(plan, batch, T, word));
        return BSK_ERR_FORMAT;
    }
    return BSK_OK;
}

int fai_fetch_device(bsk_ctx* c, int fd, const fai::Plan& plan, size_t batch, int threads, hipStream_t st, bsk_out* out, const void* gzi,
                     size_t gzi_len) {
    int rc = check_batch(c, plan, batch);
    if (rc != BSK_OK) return rc;
    const fai::Batch& b = plan.batches[batch];
    const fai::Layout L = fai::layout(b);
    struct Pinned {
        uint8_t* p = nullptr;
        ~Pinned() { if (p) (void)hipHostFree(p); }
    } pin;
    HIP_TRYX(c, hipHostMalloc((void**)&pin.p, L.bytes, hipHostMallocDefault));
    memset(pin.p + L.bytes - 16, 0, 16);
    // one arena: the spans, the tables, the complement map, the header texts, the status word
    uint64_t hdr_bytes = 0;
    for (uint32_t k = b.hit0; k < b.hit1; ++k) hdr_bytes += plan.hits[k].header.size();
    Arena A;
    const uint64_t o_buf = A.take(L.bytes), o_hits = A.take((uint64_t)(b.hit1 - b.hit0) * sizeof(fai::FetchHit)),
                   o_tiles = A.take(b.tiles * sizeof(fai::FetchTile)), o_comp = A.take(256), o_hdr = A.take(hdr_bytes + 1), o_status = A.take(8);
    rc = arena_reserve(c, &A);
    if (rc != BSK_OK) return rc;
    uint64_t blocks = 0;
    if (gzi) {  // the text exists on the device only: the spans are put together there and come back for the end probes
        fai::Gzi g;
        rc = parse_table(c, gzi, gzi_len, &g);
        if (rc != BSK_OK) return rc;
        HIP_TRYX(c, hipMemsetAsync(A.at<uint8_t>(o_buf), 0, L.bytes, st));
        rc = read_spans_bgzf_device(c, fd, g, b, L, A.at<uint8_t>(o_buf), threads, st, &blocks);
        if (rc != BSK_OK) return rc;
        HIP_TRYX(c, hipMemcpyAsync(pin.p, A.at<uint8_t>(o_buf), L.bytes, hipMemcpyDeviceToHost, st));
        HIP_TRYX(c, hipStreamSynchronize(st));
    } else {
        rc = read_spans(c, fd, b, L, pin.p, threads);
        if (rc != BSK_OK) return rc;
    }
    fai::Tables T;
    std::string err;
    rc = fai::prepare(plan, batch, L, pin.p, &T, &err);  // (the end probes: read where the bytes already are)
    if (rc != 0) { c->set_error(err); return rc; }
    uint8_t comp[256] = {0};
    if (batch_has_minus(plan, b)) complement_of(c, plan, b, L, pin.p, comp);
    note_info(b, T, blocks);
    if (T.tiles.empty()) return empty_result(c, out);
    rc = ensure_out(c, T.out_bytes + 16);
    if (rc != BSK_OK) return rc;
    const uint64_t none = fai::FETCH_NO_FAULT;
    if (!gzi) HIP_TRYX(c, hipMemcpyAsync(A.at<uint8_t>(o_buf), pin.p, L.bytes, hipMemcpyHostToDevice, st));
    HIP_TRYX(c, hipMemcpyAsync(A.at<uint8_t>(o_hits), T.hits.data(), T.hits.size() * sizeof(fai::FetchHit), hipMemcpyHostToDevice, st));
    HIP_TRYX(c, hipMemcpyAsync(A.at<uint8_t>(o_tiles), T.tiles.data(), T.tiles.size() * sizeof(fai::FetchTile), hipMemcpyHostToDevice, st));
    HIP_TRYX(c, hipMemcpyAsync(A.at<uint8_t>(o_comp), comp, 256, hipMemcpyHostToDevice, st));
    HIP_TRYX(c, hipMemcpyAsync(A.at<uint8_t>(o_hdr), T.headers.data(), T.headers.size(), hipMemcpyHostToDevice, st));
    HIP_TRYX(c, hipMemcpyAsync(A.at<uint8_t>(o_status), &none, 8, hipMemcpyHostToDevice, st));
    {
        Timed t(c, "k_faidx_fetch", st);
        HIP_TRYX(c, launch_faidx_fetch(A.at<uint8_t>(o_buf), A.at<fai::FetchHit>(o_hits), A.at<fai::FetchTile>(o_tiles),
                                       (uint32_t)T.tiles.size(), plan.line_width, A.at<uint8_t>(o_comp), A.at<uint8_t>(o_hdr), c->d_out,
                                       A.at<uint64_t>(o_status), c->num_cus, st));
    }
    uint64_t word = 0;
    HIP_TRYX(c, hipMemcpyAsync(&word, A.at<uint8_t>(o_status), 8, hipMemcpyDeviceToHost, st));
    HIP_TRYX(c, hipStreamSynchronize(st));  // (also ends the copies out of the pinned buffer and the tables)
    if (word != fai::FETCH_NO_FAULT) {
        c->set_error(fai::fault_text(plan, batch, T, word));
        return BSK_ERR_FORMAT;
    }
    out->d_data = c->d_out;
    out->len = T.out_bytes;
    out->records = T.hits.size();
    return BSK_OK;
}

}  // namespace bsk
