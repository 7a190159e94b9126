// `faidx -d IDX`: the planner of the indexed fetch and the steps around a batch that device and host share.  Pure host code
// over the standard library and fai_fetch_dev.hpp: it runs without a device and without a file (tests/host_c/
// fai_fetch_check.cpp includes this header and nothing of the library).  PARITY.md FAIX, DESIGN.md f21.
//
//   fai::parse_rows   the text of a .fai file -> rows, every refusal of FAIX "Rows" by its text
//   fai::make_plan    rows + queries + file size -> hits (row order), their line-extended spans and end probes, batches of
//                     whole hits under a byte budget, per batch the spans to read: rounded out to 4 KiB, merged where
//                     they touch or overlap.  All offsets are 64-bit.
//   fai::layout       a batch's spans -> their 16-byte aligned slots in one buffer
//   fai::prepare      after the spans were read into the buffer: the end probe of every hit record (check 2 of FAIX) and
//                     the tables the tiles take (FetchHit, FetchTile, header texts)
//   fai::run_host     the tiles of a batch on one lane
//   fai::fault_text   the status word of check 1 -> the refusal, row and file offset named
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>

#include "fai_fetch_dev.hpp"

namespace bsk {
namespace fai {

constexpr uint64_t PAGE = 4096;
constexpr uint64_t DEFAULT_BUDGET = 1ull << 30;  // BSK_FAIDX_FETCH_BYTES
constexpr int ERR_FORMAT = 3, ERR_CAPACITY = 7;  // BSK_ERR_FORMAT, BSK_ERR_CAPACITY (include/bsk.h)
inline const char* const MSG_NOT_THIS_FILE =
    "the index does not describe this file, or the record has lines of two widths; re-index / reformat with seq";

struct Row { std::string name; uint64_t length, offset, linebases, linewidth; };
struct Query { std::string name, suffix; int64_t s, e; bool minus; };  // bsk_ctx::Feature: validate_faidx_opts writes them
struct Options {
    std::vector<Query> queries;                          // the first query of a name wins (validate_faidx_opts dropped the others)
    std::function<bool(const std::string&)> regex;       // -r: does one of the expressions match the name?  (else null)
    bool ignore_case = false, full_head = false;
    uint32_t line_width = 60;
    uint64_t budget = DEFAULT_BUDGET;
    uint64_t alphabet_bytes = 0;  // minus-strand hits with a guessed alphabet: file bytes [0, alphabet_bytes) are one more span
};
struct Span { uint64_t lo, hi; };
struct Hit {
    uint32_t row, p0, p1;
    bool minus;
    std::string header;   // ">name[:b-e]\n"
    Span lines;           // first byte of the line of p0 .. behind the newline that ends the line of p1 - 1 (cut at the file's end)
    uint64_t probe;       // file offset behind the record's predicted last base
    uint64_t out_len;
};
struct Batch {
    uint32_t hit0, hit1;
    std::vector<Span> spans;
    uint64_t read_bytes, out_bytes, tiles;
};
struct Plan {
    bool fastq = false;
    uint64_t file_size = 0;
    uint32_t line_width = 60;
    uint64_t alphabet_bytes = 0;
    std::vector<Row> rows;
    std::vector<Hit> hits;
    std::vector<Batch> batches;
};

// Seq.SubLocation as ops_seq.hpp's sub_location has it (that header needs the HIP runtime's; the CPU tests hold the two
// against the same oracle): 1-based inclusive, negative = from the end; -> 0-based [b, e), b == e when empty
inline void sub_location(uint32_t length, int start, int end, uint32_t* b, uint32_t* e) {
    *b = *e = 0;
    if (length == 0) return;
    long long L = (long long)length, s = start, t = end;
    if (s < 0) { s = L + s + 1; if (s < 1) s = 1; }
    if (s == 0) s = 1;
    if (t < 0) t = L + t + 1;
    if (t > L) t = L;
    if (s > L || t < 1 || s > t) return;
    *b = (uint32_t)(s - 1);
    *e = (uint32_t)t;
}

// parseHeadID's default rule (faidx_run_device names its records by it): up to the first space, else the first tab
inline std::string head_id(const std::string& head) {
    size_t sp = head.find(' ');
    if (sp != std::string::npos && sp > 0) return head.substr(0, sp);
    sp = head.find('\t');
    if (sp != std::string::npos && sp > 0) return head.substr(0, sp);
    return head;
}

inline bool number(const std::string& t, uint64_t* v) {
    if (t.empty() || t.size() > 19) return false;
    uint64_t x = 0;
    for (char ch : t) {
        if (ch < '0' || ch > '9') return false;
        x = x * 10 + (uint64_t)(ch - '0');
    }
    *v = x;
    return true;
}

// predicted file offset behind the last base of a row with length > 0
inline uint64_t predicted_end(const Row& r) {
    return r.offset + ((r.length - 1) / r.linebases) * r.linewidth + (r.length - 1) % r.linebases + 1;
}

// format: 0 FASTA (5 columns), 1 FASTQ (6), -1: FASTQ when the first row has at least five tabs and reads as a FASTQ row
// (linewidth - linebases is 1 and the quality offset lies behind the sequence offset).  Columns are split from the right.
inline int parse_rows(const std::string& text, uint64_t file_size, int format, bool full_head, Plan* plan, std::string* err) {
    plan->rows.clear();
    plan->file_size = file_size;
    size_t at = 0, rowno = 0;
    int ncol = format == 1 ? 6 : 5;
    while (at < text.size()) {
        size_t nl = text.find('\n', at);
        if (nl == std::string::npos) nl = text.size();
        const std::string line = text.substr(at, nl - at);
        at = nl + 1;
        if (line.empty()) continue;
        ++rowno;
        auto split = [&](int cols, std::string f[6]) {
            size_t end = line.size();
            for (int k = cols - 1; k >= 1; --k) {
                const size_t tab = end ? line.rfind('\t', end - 1) : std::string::npos;
                if (tab == std::string::npos) return false;
                f[k] = line.substr(tab + 1, end - tab - 1);
                end = tab;
            }
            f[0] = line.substr(0, end);
            return true;
        };
        std::string f[6];
        if (rowno == 1 && format < 0) {
            uint64_t v[5];
            bool fq = split(6, f);
            for (int k = 1; fq && k < 6; ++k) fq = number(f[k], &v[k - 1]);
            ncol = fq && v[3] - v[2] == 1 && v[4] > v[1] ? 6 : 5;
        }
        const std::string where = "faidx -d: index row " + std::to_string(rowno);
        if (!split(ncol, f)) { *err = where + ": fewer than " + std::to_string(ncol) + " tab-separated columns: " + line; return ERR_FORMAT; }
        const std::string named = where + " (" + f[0] + ")";
        static const char* const colname[] = {"name", "length", "offset", "linebases", "linewidth", "qualoffset"};
        uint64_t v[5] = {0, 0, 0, 0, 0};
        for (int k = 1; k < ncol; ++k)
            if (!number(f[k], &v[k - 1])) { *err = named + ": column " + colname[k] + " is not a number: " + f[k]; return ERR_FORMAT; }
        Row r{f[0], v[0], v[1], v[2], v[3]};
        if (r.length >= (1ull << 32)) { *err = named + ": length " + f[1] + " is 2^32 or more"; return ERR_FORMAT; }
        const bool both_zero = r.linebases == 0 && r.linewidth == 0;
        if (!both_zero && r.linewidth - r.linebases != 1) {
            *err = named + ": linewidth " + f[4] + " - linebases " + f[3] + " is not 1 (the index of a file with \\r\\n line ends? "
                   "the \\r is data here: re-index with this program)";
            return ERR_FORMAT;
        }
        if (r.length > 0 && r.linebases == 0) { *err = named + ": linebases 0 with length " + f[1]; return ERR_FORMAT; }
        if (r.offset > file_size || (r.length > 0 && (r.linebases >= (1ull << 32) || predicted_end(r) > file_size))) {
            *err = named + ": offset " + f[2] + " or the predicted end of the sequence lies beyond the file (" + std::to_string(file_size) + " bytes)";
            return ERR_FORMAT;
        }
        if (!full_head && r.name.find_first_of(" \t") != std::string::npos) {
            *err = named + ": the name holds a blank or tab (an index written with -f is read with -f)";
            return ERR_FORMAT;
        }
        plan->rows.push_back(r);
    }
    plan->fastq = ncol == 6;
    return 0;
}

inline Span round_out(Span s, uint64_t file_size) {
    s.lo &= ~(PAGE - 1);
    s.hi = (s.hi + PAGE - 1) & ~(PAGE - 1);
    if (s.hi > file_size) s.hi = file_size;
    return s;
}
inline uint64_t span_cost(Span s, uint64_t file_size) { const Span r = round_out(s, file_size); return r.hi > r.lo ? r.hi - r.lo : 0; }
inline Span probe_span(const Hit& h, uint64_t file_size) { return Span{std::min(h.probe, file_size), std::min(h.probe + 2, file_size)}; }

// spans rounded out to 4 KiB, sorted, merged where they touch or overlap
inline std::vector<Span> merge_spans(std::vector<Span> in, uint64_t file_size) {
    std::vector<Span> v;
    for (Span s : in) {
        s = round_out(s, file_size);
        if (s.hi > s.lo) v.push_back(s);
    }
    std::sort(v.begin(), v.end(), [](const Span& a, const Span& b) { return a.lo < b.lo || (a.lo == b.lo && a.hi < b.hi); });
    std::vector<Span> out;
    for (const Span& s : v) {
        if (!out.empty() && s.lo <= out.back().hi) out.back().hi = std::max(out.back().hi, s.hi);
        else out.push_back(s);
    }
    return out;
}

// plan->rows are parsed; hits, batches.  0, or ERR_CAPACITY (one hit above the budget) with the sizes in *err
inline int make_plan(const Options& o, Plan* plan, std::string* err) {
    plan->hits.clear();
    plan->batches.clear();
    plan->line_width = o.line_width;
    plan->alphabet_bytes = std::min(o.alphabet_bytes, plan->file_size);
    std::unordered_map<std::string, size_t> by_name;
    for (size_t q = 0; q < o.queries.size(); ++q) by_name.emplace(o.queries[q].name, q);
    for (size_t i = 0; i < plan->rows.size(); ++i) {
        const Row& r = plan->rows[i];
        if (r.length == 0) continue;  // SubLocation of an empty sequence is not ok: never a hit
        const std::string id = o.full_head ? head_id(r.name) : r.name;
        Hit h;
        h.row = (uint32_t)i;
        std::string suffix;
        if (o.regex) {
            if (!o.regex(id)) continue;
            h.p0 = 0; h.p1 = (uint32_t)r.length; h.minus = false;
        } else {
            std::string key = id;
            if (o.ignore_case) for (auto& ch : key) if (ch >= 'A' && ch <= 'Z') ch += 32;
            auto it = by_name.find(key);
            if (it == by_name.end()) continue;
            const Query& q = o.queries[it->second];
            sub_location((uint32_t)r.length, (int)q.s, (int)q.e, &h.p0, &h.p1);
            if (h.p0 == h.p1) continue;
            h.minus = q.minus;
            suffix = q.suffix;
        }
        h.header = ">" + id + suffix + "\n";
        const uint64_t l0 = h.p0 / r.linebases, l1 = (h.p1 - 1) / r.linebases;
        h.lines.lo = r.offset + l0 * r.linewidth;
        h.lines.hi = std::min(plan->file_size, r.offset + l1 * r.linewidth + std::min(r.linebases, r.length - l1 * r.linebases) + 1);
        h.probe = predicted_end(r);
        h.out_len = h.header.size() + wrapped_len64(h.p1 - h.p0, o.line_width) + 1;
        plan->hits.push_back(h);
    }
    // batches of whole hits: what a hit reads at most (its lines, its probe, both rounded out) and what it writes
    auto close_batch = [&](uint32_t h0, uint32_t h1) {
        Batch b;
        b.hit0 = h0; b.hit1 = h1;
        b.out_bytes = 0; b.tiles = 0;
        std::vector<Span> want;
        bool minus = false;
        for (uint32_t k = h0; k < h1; ++k) {
            const Hit& h = plan->hits[k];
            want.push_back(h.lines);
            want.push_back(probe_span(h, plan->file_size));
            b.out_bytes += h.out_len;
            b.tiles += ((uint64_t)(h.p1 - h.p0) + FETCH_T - 1) / FETCH_T;
            minus = minus || h.minus;
        }
        if (minus && plan->alphabet_bytes) want.push_back(Span{0, plan->alphabet_bytes});
        b.spans = merge_spans(want, plan->file_size);
        b.read_bytes = 0;
        for (const Span& s : b.spans) b.read_bytes += s.hi - s.lo;
        plan->batches.push_back(b);
    };
    uint64_t used = 0;
    uint32_t first = 0;
    for (uint32_t k = 0; k < plan->hits.size(); ++k) {
        const Hit& h = plan->hits[k];
        const uint64_t cost = span_cost(h.lines, plan->file_size) + span_cost(probe_span(h, plan->file_size), plan->file_size) + h.out_len +
                              (h.minus ? plan->alphabet_bytes : 0);
        if (cost > o.budget) {
            *err = "faidx -d: the region of index row " + std::to_string(h.row + 1) + " (" + plan->rows[h.row].name + ") reads and writes " +
                   std::to_string(cost) + " bytes, the budget of a batch is " + std::to_string(o.budget) + " (BSK_FAIDX_FETCH_BYTES)";
            return ERR_CAPACITY;
        }
        if (k > first && used + cost > o.budget) { close_batch(first, k); first = k; used = 0; }
        used += cost;
    }
    if (first < plan->hits.size()) close_batch(first, (uint32_t)plan->hits.size());
    return 0;
}

// ---- a batch in one buffer: span k at slot[k] (16-byte aligned), `bytes` in all with 16 bytes of padding behind the last
struct Layout { std::vector<uint64_t> slot; uint64_t bytes = 0; };
inline Layout layout(const Batch& b) {
    Layout L;
    uint64_t at = 0;
    for (const Span& s : b.spans) {
        L.slot.push_back(at);
        at += (s.hi - s.lo + 15) & ~15ull;
    }
    L.bytes = at + 16;
    return L;
}
// buffer index of file offset x (inside span k or not: the arithmetic is the same), and the span that holds [lo, hi)
inline uint64_t buf_index(const Batch& b, const Layout& L, size_t k, uint64_t x) { return L.slot[k] + (x - b.spans[k].lo); }
inline size_t span_of(const Batch& b, uint64_t lo) {
    size_t a = 0, z = b.spans.size();
    while (z - a > 1) { const size_t m = (a + z) / 2; if (b.spans[m].lo <= lo) a = m; else z = m; }
    return a;
}

struct Tables {
    std::vector<FetchHit> hits;
    std::vector<FetchTile> tiles;
    std::string headers;
    uint64_t out_bytes = 0;
};

inline std::string not_this_file(const Plan& plan, uint32_t row, uint64_t file_offset) {
    return "faidx -d: index row " + std::to_string(row + 1) + " (" + plan.rows[row].name + "), file offset " + std::to_string(file_offset) +
           ": " + MSG_NOT_THIS_FILE;
}

// After the batch's spans stand in buf: check 2 of FAIX per hit record -- the two bytes behind the predicted last base: the
// first is '\n' or the end of the file, the second the end of the file, '\n', '>' (FASTA index) or '+' (FASTQ) -- and the tables
inline int prepare(const Plan& plan, size_t batch, const Layout& L, const uint8_t* buf, Tables* T, std::string* err) {
    const Batch& b = plan.batches[batch];
    T->hits.clear(); T->tiles.clear(); T->headers.clear();
    uint64_t out = 0;
    for (uint32_t k = b.hit0; k < b.hit1; ++k) {
        const Hit& h = plan.hits[k];
        const Row& r = plan.rows[h.row];
        if (h.probe < plan.file_size) {
            const size_t sp = span_of(b, h.probe);
            const uint8_t c0 = buf[buf_index(b, L, sp, h.probe)];
            bool ok = c0 == '\n';
            if (ok && h.probe + 1 < plan.file_size) {
                const uint8_t c1 = buf[buf_index(b, L, sp, h.probe + 1)];
                ok = c1 == '\n' || c1 == (plan.fastq ? '+' : '>');
            }
            if (!ok) { *err = not_this_file(plan, h.row, h.probe); return ERR_FORMAT; }
        }
        const size_t sp = span_of(b, h.lines.lo);
        FetchHit d;
        memset(&d, 0, sizeof d);
        d.src = buf_index(b, L, sp, r.offset);  // (may wrap below zero: only indices of the hit's lines are ever formed)
        d.eof = buf_index(b, L, sp, plan.file_size);
        d.out = out;
        d.hdr = T->headers.size();
        d.hdr_len = (uint32_t)h.header.size();
        d.length = (uint32_t)r.length;
        d.linebases = (uint32_t)r.linebases;
        d.p0 = h.p0; d.p1 = h.p1;
        d.minus = h.minus ? 1u : 0u;
        d.tile0 = (uint32_t)T->tiles.size();
        T->headers += h.header;
        for (uint64_t q = 0; q < h.p1 - h.p0; q += FETCH_T) T->tiles.push_back(FetchTile{(uint32_t)T->hits.size(), (uint32_t)q});
        T->hits.push_back(d);
        out += h.out_len;
    }
    T->out_bytes = out;
    return 0;
}

// the status word of check 1 -> the refusal
inline std::string fault_text(const Plan& plan, size_t batch, const Tables& T, uint64_t word) {
    const uint32_t tile = std::min<uint32_t>((uint32_t)(word >> 32), (uint32_t)T.tiles.size() - 1);
    const FetchTile& t = T.tiles[tile];
    const FetchHit& d = T.hits[t.hit];
    const Hit& h = plan.hits[plan.batches[batch].hit0 + t.hit];
    const TileGeo g = tile_geo(d, t.q0);
    return not_this_file(plan, h.row, plan.rows[h.row].offset + g.j_lo + (word & 0xFFFFFFFFull));
}

// ---- a BGZF sequence file: the block table (htslib's .gzi: little-endian uint64 count, then (compressed offset, text offset)
// of every block behind the first) turns a span of the TEXT into a run of whole blocks
struct Gzi {
    std::vector<uint64_t> coff, uoff;  // every block, the first one (0, 0) included
};
inline uint64_t le64(const uint8_t* p) { uint64_t v = 0; for (int k = 7; k >= 0; --k) v = v << 8 | p[k]; return v; }
inline void put64(std::string* s, uint64_t v) { for (int k = 0; k < 8; ++k) s->push_back((char)(v >> (8 * k) & 0xFF)); }
inline std::string gzi_image(const Gzi& g) {
    std::string s;
    put64(&s, g.coff.size() - 1);
    for (size_t k = 1; k < g.coff.size(); ++k) { put64(&s, g.coff[k]); put64(&s, g.uoff[k]); }
    return s;
}
inline int gzi_parse(const uint8_t* p, size_t n, Gzi* g, std::string* err) {
    g->coff.assign(1, 0);
    g->uoff.assign(1, 0);
    if (n < 8 || (n - 8) % 16 != 0 || le64(p) != (n - 8) / 16) { *err = "faidx -d: the block table is not a .gzi file (a count and that many pairs of 64-bit offsets)"; return ERR_FORMAT; }
    for (size_t k = 0; k < (n - 8) / 16; ++k) {
        const uint64_t c = le64(p + 8 + 16 * k), u = le64(p + 16 + 16 * k);
        if (c <= g->coff.back() || u < g->uoff.back()) { *err = "faidx -d: block table entry " + std::to_string(k + 1) + " does not ascend"; return ERR_FORMAT; }
        g->coff.push_back(c);
        g->uoff.push_back(u);
    }
    return 0;
}
// the blocks [first, last] that hold text [lo, hi), lo < hi: the last block that begins at or before lo (empty blocks in front
// of it hold nothing of the span) through the block of byte hi - 1
inline void gzi_blocks(const Gzi& g, uint64_t lo, uint64_t hi, size_t* first, size_t* last) {
    *first = (size_t)(std::upper_bound(g.uoff.begin(), g.uoff.end(), lo) - g.uoff.begin()) - 1;
    *last = (size_t)(std::upper_bound(g.uoff.begin(), g.uoff.end(), hi - 1) - g.uoff.begin()) - 1;
}

struct HostPolicy {
    static constexpr uint32_t LANES = 1;
    const uint8_t* buf;
    uint8_t* out;
    uint64_t status;
    uint32_t lane() const { return 0; }
    void sync() const {}
    Vec16 load16(uint64_t i) const { Vec16 v; memcpy(&v, buf + i, 16); return v; }
    uint8_t byte(uint64_t i) const { return buf[i]; }
    void store16(uint64_t o, const Vec16& v) const { memcpy(out + o, &v, 16); }
    void store8(uint64_t o, uint8_t b) const { out[o] = b; }
    void fail(uint64_t word) { if (word < status) status = word; }
};

// the tiles of a prepared batch on one lane: `out` has T.out_bytes bytes.  -> the status word (FETCH_NO_FAULT: none)
inline uint64_t run_host(const Tables& T, const uint8_t* buf, uint32_t line_width, const uint8_t comp[256], uint8_t* out) {
    HostPolicy p{buf, out, FETCH_NO_FAULT};
    std::vector<FetchShared> S(1);
    for (size_t t = 0; t < T.tiles.size(); ++t)
        fetch_tile(p, S[0], T.hits[T.tiles[t].hit], (uint32_t)t, T.tiles[t].q0, line_width, comp, reinterpret_cast<const uint8_t*>(T.headers.data()));
    return p.status;
}

}  // namespace fai

}  // namespace bsk
