// Host side of `replace` (bigseqkit-lib/replace.go): Before() (:36-104) with the reference's messages in its order,
// readKVs (:183-218), and the Call (:106-179) flow on the device (ops_replace.hip).  C-ABI in include/bsk.h.
#include <hip/hip_runtime_api.h>

#include <cerrno>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/bsk.h"
#include "ctx.hpp"
#include "ops_host.hpp"
#include "ops_host_internal.hpp"
#include "ops_replace.hpp"
#include "ops_seq.hpp"

struct ReplaceState {
    bsk::VmProgram prog;
    std::vector<std::string> names;
    int ncap = 4;
    bool kv = false, byte_class = false, class_group1 = false;
    uint32_t cls[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<std::pair<std::string, std::string>> pairs;
    // device copies (uploaded by the first run)
    uint8_t* d_blob = nullptr;
    uint8_t* d_stage = nullptr;
    uint64_t stage_cap = 0;
    bsk::ReplParams R;
};

namespace bsk {

namespace {

bool is_sym(const std::string& t, size_t i, const char* lo) {  // {nr} {NR} / {kv} {KV}
    if (i + 4 > t.size() || t[i] != '{' || t[i + 3] != '}') return false;
    return (t[i + 1] == lo[0] && t[i + 2] == lo[1]) || (t[i + 1] == lo[0] - 32 && t[i + 2] == lo[1] - 32);
}
bool has_sym(const std::string& t, const char* lo) {
    for (size_t i = 0; i < t.size(); ++i) if (is_sym(t, i, lo)) return true;
    return false;
}
bool word(char ch) { return isalnum((unsigned char)ch) || ch == '_'; }

// highest group the template can reference (extract() of Go's expand); -1 when a reference runs into a {nr} / {kv}
// (its name is only known per record)
int max_ref(const std::string& t, const std::vector<std::string>& names, int ngroups) {
    int m = 0;
    for (size_t i = 0; i < t.size(); ++i) {
        if (t[i] != '$') continue;
        if (i + 1 < t.size() && t[i + 1] == '$') { ++i; continue; }
        size_t j = i + 1;
        const bool brace = j < t.size() && t[j] == '{';
        if (brace && (is_sym(t, j, "nr") || is_sym(t, j, "kv"))) return -1;
        if (brace) ++j;
        const size_t n0 = j;
        while (j < t.size() && word(t[j])) ++j;
        if (is_sym(t, j, "nr") || is_sym(t, j, "kv")) return -1;
        if (j == n0 || (brace && (j >= t.size() || t[j] != '}'))) continue;
        const std::string name = t.substr(n0, j - n0);
        bool digits = name.size() <= 8;
        for (char ch : name) digits &= ch >= '0' && ch <= '9';
        if (digits && !(name[0] == '0' && name.size() > 1)) {
            const int g = std::stoi(name);
            if (g <= ngroups && g > m) m = g;
        } else {
            for (int g = 1; g <= ngroups; ++g) if (names[g] == name) { if (g > m) m = g; break; }
        }
    }
    return m;
}

uint64_t fnv1a64_host(const std::string& k) {  // fnv1a64 of pattern_match_dev.hpp (no folding: keys are stored folded)
    uint64_t h = 1469598103934665603ull;
    for (unsigned char ch : k) h = (h ^ ch) * 1099511628211ull;
    return h ? h : 1ull;
}

std::string go_errno(int e) {  // Go's syscall error text: strerror, lower-cased first letter
    std::string s = strerror(e);
    if (!s.empty()) s[0] = (char)tolower((unsigned char)s[0]);
    return s;
}

}  // namespace

void replace_free(bsk_ctx* c) {
    if (!c->repl) return;
    if (c->repl->d_blob) hipFree(c->repl->d_blob);
    if (c->repl->d_stage) hipFree(c->repl->d_stage);
    delete c->repl;
    c->repl = nullptr;
}

void validate_replace_opts(bsk_ctx* c) {
    const Options& o = c->opts;
    c->alphabet = alphabet_from_seqtype(o.cs("SeqType"));
    check_id_regexp(c);
    const std::string& pat = o.s("Pattern");
    const std::string& repl = o.s("Replacement");
    if (pat.empty()) throw OptError("flags -p (--pattern) needed");
    const std::string p = o.b("IgnoreCase") ? "(?i)" + pat : pat;
    std::vector<std::string> names;
    VmProgram prog = compile_vm(p, 1, &names);
    const std::string& kvf = o.s("KvFile");
    if (!kvf.empty()) {
        if (repl.empty()) throw OptError("flag -r (--replacement) needed when given flag -k (--kv-file)");
        if (!has_sym(repl, "kv"))
            throw OptError("replacement symbol \"{kv}\"/\"{KV}\" not found in value of flag -r (--replacement) when flag -k (--kv-file) given");
    }
    std::unique_ptr<ReplaceState> S(new ReplaceState());
    S->kv = has_sym(repl, "kv");
    if (S->kv) {
        bool paren = false;  // regexp `\(.+\)` on the pattern as given
        for (size_t i = 0; i < pat.size() && !paren; ++i) {
            if (pat[i] != '(') continue;
            for (size_t j = i + 1; j < pat.size() && pat[j] != '\n'; ++j)
                if (pat[j] == ')' && j > i + 1) { paren = true; break; }
        }
        if (!paren) throw OptError("value of -p (--pattern) must contains \"(\" and \")\" to capture data which is used specify the KEY");
        if (o.b("BySeq")) throw OptError("replaceing with key-value pairs was not supported for sequence");
        if (kvf.empty())
            throw OptError("since replacement symbol \"{kv}\"/\"{KV}\" found in value of flag -r (--replacement), tab-delimited key-value file should be given by flag -k (--kv-file)");
        c->info("read key-value file: " + kvf, true);
        std::ifstream f(kvf, std::ios::binary);
        if (!f) throw OptError("read key-value file: open " + kvf + ": " + go_errno(errno));
        std::stringstream ss;
        ss << f.rdbuf();
        const std::string text = ss.str();
        std::unordered_map<std::string, size_t> at;
        for (size_t a = 0; a < text.size();) {
            size_t b = text.find('\n', a);
            if (b == std::string::npos) b = text.size();
            std::string line = text.substr(a, b - a);
            a = b + 1;
            while (!line.empty() && (line.back() == '\r' || line.back() == '\n')) line.pop_back();
            const size_t tab = line.find('\t');
            if (tab == std::string::npos) continue;
            std::string k = line.substr(0, tab);
            const size_t tab2 = line.find('\t', tab + 1);
            std::string v = line.substr(tab + 1, tab2 == std::string::npos ? std::string::npos : tab2 - tab - 1);
            if (o.b("IgnoreCase")) for (auto& ch : k) if (ch >= 'A' && ch <= 'Z') ch += 32;
            auto it = at.find(k);
            if (it == at.end()) { at[k] = S->pairs.size(); S->pairs.emplace_back(k, v); }
            else S->pairs[it->second].second = v;  // later lines overwrite earlier ones
        }
        if (S->pairs.empty()) throw OptError("no valid data in key-value file: " + kvf);
        c->info(std::to_string(S->pairs.size()) + " pairs of key-value loaded", true);
    }
    // capture slots: the groups the template (and -I) can name; a reference whose name is only known per record, a kept
    // key or a value that is itself a template may name any group
    const int ng = (int)prog.ngroups;
    int need = max_ref(repl, names, ng);
    if (S->kv) need = ng;
    if (need < 0) need = ng;
    if (S->kv && o.i("KeyCaptIdx") <= ng && o.i("KeyCaptIdx") > need) need = (int)o.i("KeyCaptIdx");
    if (o.i("KeyCaptIdx") < 0) throw OptError("value of flag -I (--key-capt-idx) should be positive");
    if (need > 9)
        throw OptError("libbsk: replace: the replacement may reference capture group " + std::to_string(need) +
                       "; more than 9 groups is not supported by the HIP path: `" + p + "`");
    S->ncap = need <= 1 ? 4 : need <= 3 ? 8 : 20;
    S->prog = compile_vm(p, need, &S->names);
    S->names = names;
    // -s with an expression that is one byte class: every byte is a match or not, a per-byte map (tune replace=vm: the matcher)
    // The program must be exactly SAVE0 CHAR SAVE1 MATCH (no group is referenced) or SAVE0 SAVE2 CHAR SAVE3 SAVE1 MATCH
    // (group 1 is the byte itself): an empty group beside the class, `()N`, takes the matcher.
    if (o.b("BySeq") && need <= 1 && !c->tune.is("replace", "vm")) {
        const VmProgram& P = S->prog;
        auto at = [&P](uint32_t k, uint8_t op, int arg) { return P.inst[k].op == op && (arg < 0 || P.inst[k].arg == arg); };
        int ci = -1;
        if (P.n == 4 && at(0, VM_SAVE, 0) && at(1, VM_CHAR, -1) && at(2, VM_SAVE, 1) && at(3, VM_MATCH, -1)) ci = 1;
        if (P.n == 6 && at(0, VM_SAVE, 0) && at(1, VM_SAVE, 2) && at(2, VM_CHAR, -1) && at(3, VM_SAVE, 3) && at(4, VM_SAVE, 1) &&
            at(5, VM_MATCH, -1)) { ci = 2; S->class_group1 = true; }
        if (ci >= 0) {
            S->byte_class = true;
            for (int w = 0; w < 8; ++w) S->cls[w] = P.sets[P.inst[ci].arg][w];
        }
    }
    replace_free(c);
    c->repl = S.release();
}

namespace {

int upload(bsk_ctx* c, hipStream_t st) {
    ReplaceState& S = *c->repl;
    if (S.d_blob) return BSK_OK;
    const Options& o = c->opts;
    ReplParams& R = S.R;
    memset(&R, 0, sizeof R);
    // layout: program | err | name_off | kv_off | kv_keys | kv_idx | bytes (template, names, miss, kv blob)
    const std::string& tmpl = o.s("Replacement");
    const std::string& miss = o.s("KeyMissRepl");
    std::vector<uint32_t> name_off{0};
    std::string names;
    for (auto& nm : S.names) { names += nm; name_off.push_back((uint32_t)names.size()); }
    uint64_t cap = 1;
    while (cap < 2 * S.pairs.size() + 2) cap <<= 1;
    std::vector<uint64_t> keys(S.kv ? cap : 1, 0), kv_off{0};
    std::vector<uint32_t> idx(S.kv ? cap : 1, 0);
    std::string kvb;
    for (size_t e = 0; e < S.pairs.size(); ++e) {
        kvb += S.pairs[e].first; kv_off.push_back(kvb.size());
        kvb += S.pairs[e].second; kv_off.push_back(kvb.size());
        const auto& k = S.pairs[e].first;
        const uint64_t h = fnv1a64_host(k);
        uint64_t s = h & (cap - 1);
        while (keys[s]) s = (s + 1) & (cap - 1);
        keys[s] = h; idx[s] = (uint32_t)e;
    }
    std::vector<uint8_t> blob;
    auto put = [&](const void* p, size_t nb) { const size_t at = (blob.size() + 15) & ~(size_t)15; blob.resize(at + nb); if (nb) memcpy(blob.data() + at, p, nb); return at; };
    const size_t a_prog = put(&S.prog, sizeof S.prog);
    std::vector<uint64_t> err(REPL_ERR_KINDS, ~0ull);
    const size_t a_err = put(err.data(), err.size() * 8);
    const size_t a_noff = put(name_off.data(), name_off.size() * 4);
    const size_t a_kvoff = put(kv_off.data(), kv_off.size() * 8);
    const size_t a_keys = put(keys.data(), keys.size() * 8);
    const size_t a_idx = put(idx.data(), idx.size() * 4);
    const size_t a_tmpl = put(tmpl.data(), tmpl.size() + 1);
    const size_t a_names = put(names.data(), names.size() + 1);
    const size_t a_miss = put(miss.data(), miss.size() + 1);
    const size_t a_kvb = put(kvb.data(), kvb.size() + 1);
    HIP_TRYX(c, hipMalloc((void**)&S.d_blob, blob.size()));
    HIP_TRYX(c, hipMemcpyAsync(S.d_blob, blob.data(), blob.size(), hipMemcpyHostToDevice, st));
    HIP_TRYX(c, hipStreamSynchronize(st));
    uint8_t* b = S.d_blob;
    R.prog = reinterpret_cast<const VmProgram*>(b + a_prog);
    R.err = reinterpret_cast<unsigned long long*>(b + a_err);
    R.name_off = reinterpret_cast<const uint32_t*>(b + a_noff);
    R.names = b + a_names;
    R.ngroups = S.prog.ngroups;
    R.tmpl = b + a_tmpl;
    R.tmpl_len = (uint32_t)tmpl.size();
    R.nr_width = (int)o.i("NrWidth");
    R.kv = S.kv;
    R.keep_untouch = o.b("KeepUntouch");
    R.keep_key = o.b("KeepKey");
    R.icase = o.b("IgnoreCase");
    R.capt_idx = (int)o.i("KeyCaptIdx");
    R.capt_over = o.i("KeyCaptIdx") > (int64_t)S.prog.ngroups;  // > len(found) - 1 (replace.go:153)
    if (R.capt_over) R.capt_idx = 0;
    R.kv_keys = reinterpret_cast<const uint64_t*>(b + a_keys);
    R.kv_idx = reinterpret_cast<const uint32_t*>(b + a_idx);
    R.kv_mask = cap - 1;
    R.kv_blob = b + a_kvb;
    R.kv_off = reinterpret_cast<const uint64_t*>(b + a_kvoff);
    R.miss = b + a_miss;
    R.miss_len = (uint32_t)miss.size();
    R.line_width = (int)o.ci("LineWidth");
    R.byte_class = S.byte_class;
    R.class_group1 = S.class_group1;
    R.fastq = 0;
    for (int w = 0; w < 8; ++w) R.cls[w] = S.cls[w];
    return BSK_OK;
}

// the reference's Call error (or this engine's refusal) for the lowest offending record
int record_errors(bsk_ctx* c, const uint8_t* d_buf, hipStream_t st) {
    ReplaceState& S = *c->repl;
    uint64_t err[REPL_ERR_KINDS];
    HIP_TRYX(c, hipMemcpyAsync(err, S.R.err, sizeof err, hipMemcpyDeviceToHost, st));
    HIP_TRYX(c, hipStreamSynchronize(st));
    int kind = -1;
    for (int k = 0; k < REPL_ERR_KINDS; ++k) if (err[k] != ~0ull && (kind < 0 || err[k] < err[kind])) kind = k;
    if (kind < 0) return BSK_OK;
    const uint64_t i = err[kind];
    uint64_t start = 0;
    uint32_t lh = 0;
    HIP_TRYX(c, hipMemcpy(&start, c->table.start + i, 8, hipMemcpyDeviceToHost));
    HIP_TRYX(c, hipMemcpy(&lh, c->table.l_head + i, 4, hipMemcpyDeviceToHost));
    std::string name(lh > 0 ? lh - 1 : 0, '\0');
    if (!name.empty()) HIP_TRYX(c, hipMemcpy(&name[0], d_buf + start + 1, name.size(), hipMemcpyDeviceToHost));
    const std::string& pat = c->opts.s("Pattern");
    switch (kind) {
        case REPL_ERR_MULTI:
            c->set_error("pattern \"" + pat + "\" matches multiple targets in \"" + name + "\", this will cause chaos");
            return BSK_ERR_FORMAT;
        case REPL_ERR_CAPT: c->set_error("value of flag -I (--key-capt-idx) overflows"); return BSK_ERR_FORMAT;
        case REPL_ERR_NONASCII:
            c->set_error("libbsk: replace: the target of record \"" + name +
                         "\" holds a byte >= 0x80 (Go matches UTF-8 characters, the HIP path bytes)");
            return BSK_ERR_UNSUPPORTED;
        case REPL_ERR_SIZE:
            c->set_error("libbsk: replace: the output of record \"" + name + "\" would reach 2^32 bytes (the HIP path writes records below 4 GiB)");
            return BSK_ERR_UNSUPPORTED;
        default:
            c->set_error("libbsk: replace: the replacement of record \"" + name + "\" exceeds " +
                         std::to_string(REPL_TMPL_MAX) + " bytes after {nr} / {kv}");
            return BSK_ERR_UNSUPPORTED;
    }
}

}  // namespace

int replace_run_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, bsk_out* out) {
    const Options& o = c->opts;
    const bool fastq = format == BSK_FORMAT_FASTQ;
    out->d_data = nullptr; out->len = 0; out->records = 0;
    int rc = build_index(c, d_buf, n, format, st);
    if (rc != BSK_OK) return rc;
    if (c->table.n == 0) return empty_result(c, out);
    if (o.b("BySeq") && fastq) { c->set_error("editing FASTQ is not supported"); return BSK_ERR_FORMAT; }
    rc = upload(c, st);
    if (rc != BSK_OK) return rc;
    ReplaceState& S = *c->repl;
    ReplParams R = S.R;
    R.nr_base = c->nr_base;
    R.fastq = fastq;
    HIP_TRYX(c, hipMemsetAsync(R.err, 0xFF, REPL_ERR_KINDS * sizeof(uint64_t), st));
    const uint64_t N = c->table.n;
    TextTableH tt{nullptr, nullptr, nullptr};
    rc = prepare_text(c, d_buf, format, st, &tt);
    if (rc != BSK_OK) return rc;
    rc = ensure_record_scratch(c);
    if (rc != BSK_OK) return rc;
    if (o.b("BySeq")) {
        uint64_t total = 0, kept = 0;
        {
            Timed t(c, "k_repl_seq_size", st);
            HIP_TRYX(c, launch_repl_seq(S.ncap, false, d_buf, c->table, tt.text_w, tt.lin_off, tt.lin, R, c->d_out_len, nullptr, nullptr, st));
        }
        rc = record_errors(c, d_buf, st);
        if (rc != BSK_OK) return rc;
        rc = finish_sizes(c, st, &total, &kept);
        if (rc != BSK_OK) return rc;
        rc = ensure_out(c, total);
        if (rc != BSK_OK) return rc;
        {
            Timed t(c, "k_repl_seq_write", st);
            HIP_TRYX(c, launch_repl_seq(S.ncap, true, d_buf, c->table, tt.text_w, tt.lin_off, tt.lin, R, c->d_out_len, c->d_out_off, c->d_out, st));
        }
        out->d_data = c->d_out;
        out->len = total;
        out->records = kept;
    } else {
        Arena A;
        const uint64_t o_len = A.take(N * 4), o_off = A.take((N + 1) * 8);
        rc = arena_reserve(c, &A);
        if (rc != BSK_OK) return rc;
        uint32_t* d_len = A.at<uint32_t>(o_len);
        uint64_t* d_off = A.at<uint64_t>(o_off);
        {
            Timed t(c, "k_repl_heads_size", st);
            HIP_TRYX(c, launch_repl_heads(S.ncap, false, d_buf, c->table, R, d_len, nullptr, nullptr, st));
        }
        HIP_TRYX(c, launch_scan_u32(d_len, d_off, N, c->d_scan_tmp, st));
        rc = record_errors(c, d_buf, st);
        if (rc != BSK_OK) return rc;
        uint64_t staged = 0;
        HIP_TRYX(c, hipMemcpyAsync(&staged, d_off + N, 8, hipMemcpyDeviceToHost, st));
        HIP_TRYX(c, hipStreamSynchronize(st));
        rc = grow(c, &S.d_stage, &S.stage_cap, staged + 16, staged / 8 + 256);
        if (rc != BSK_OK) return rc;
        {
            Timed t(c, "k_repl_heads_write", st);
            HIP_TRYX(c, launch_repl_heads(S.ncap, true, d_buf, c->table, R, d_len, d_off, S.d_stage, st));
        }
        SeqParams P = format_params(c, fastq);
        P.buf_end = d_buf + n;
        P.text_w = tt.text_w; P.lin_off = tt.lin_off; P.lin = tt.lin;
        P.rep_len = d_len; P.rep_off = d_off; P.rep_stage = S.d_stage;
        HIP_TRYX(c, launch_seq_size(d_buf, c->table, P, c->d_out_len, c->d_status, st));
        rc = emit_sized(c, d_buf, n, P, st, out);
        if (rc != BSK_OK) return rc;
    }
    c->nr_base += N;
    return BSK_OK;
}

}  // namespace bsk

extern "C" int bsk_regex_replace(const char* expr, const char* repl, const uint8_t* text, size_t n, uint8_t* out, size_t cap,
                                 size_t* len) {
    if (!expr || !repl || (!text && n) || !len || (!out && cap)) return bsk::global_error_set(BSK_ERR_INVALID_ARG, "libbsk: null argument");
    try {
        std::vector<std::string> names;
        const bsk::VmProgram P = bsk::compile_vm(expr, 9, &names);
        auto group_of = [&names](const uint8_t* s, uint32_t nl) {
            for (size_t g = 1; g < names.size(); ++g)
                if (names[g].size() == nl && memcmp(names[g].data(), s, nl) == 0) return (int)g;
            return -1;
        };
        size_t k = 0;
        auto put = [&](uint8_t ch) { if (k < cap) out[k] = ch; ++k; };
        auto at = [text](uint32_t i) { return text[i]; };
        bsk::vm_replace_all<20>(P, at, (uint32_t)n, (const uint8_t*)repl, (uint32_t)strlen(repl), group_of, put);
        *len = k;
        return k > cap ? bsk::global_error_set(BSK_ERR_CAPACITY, "libbsk: output buffer too small") : BSK_OK;
    } catch (const std::exception& e) { return bsk::global_error_set(BSK_ERR_OPTS, e.what()); }
}
