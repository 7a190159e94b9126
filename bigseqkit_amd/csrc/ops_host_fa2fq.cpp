// Host side of `fa2fq` (bigseqkit-lib/fa2fq.go): Before() (:29-57) with the reference's messages in its order, the
// FASTA table (fastx.GetSeqsMap keyed by full name, PARITY.md PFILE) and the Call flow on the device (ops_fa2fq.hip;
// what it computes: PARITY.md FA2FQ).  C-ABI in include/bsk.h.
#include <hip/hip_runtime_api.h>

#include <cerrno>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/bsk.h"
#include "ctx.hpp"
#include "ops_fa2fq.hpp"
#include "ops_host.hpp"
#include "ops_host_internal.hpp"

struct Fa2FqState {
    std::vector<std::pair<std::string, std::string>> recs;  // full name -> sequence (distinct names)
    uint8_t* d_blob = nullptr;                               // device copy (uploaded by the first run)
    uint8_t* d_comp = nullptr;                               // complement map of the running partition
    bsk::Fa2FqParams P;
};

namespace bsk {

namespace {

uint64_t fnv1a64_host(const std::string& k) {  // fnv1a64 of pattern_match_dev.hpp, no folding
    uint64_t h = 1469598103934665603ull;
    for (unsigned char ch : k) h = (h ^ ch) * 1099511628211ull;
    return h ? h : 1ull;
}

// fastx.GetSeqsMap(file, seq.Unlimit, ..., "") (fa2fq.go:44): full name -> sequence, the lines of a sequence joined, `\r`
// trimmed, a repeated name keeps the later sequence (PARITY.md PFILE; the rule of `locate -f`, with a map instead of its
// linear search: the table of a read set has millions of names)
std::vector<std::pair<std::string, std::string>> read_fasta_map(const std::string& path) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) {
        std::string why = strerror(errno);  // Go's syscall error text: lower-cased first letter
        if (!why.empty()) why[0] = (char)tolower((unsigned char)why[0]);
        throw OptError("open " + path + ": " + why);
    }
    std::string s;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
    fclose(f);
    std::vector<std::pair<std::string, std::string>> out;
    std::unordered_map<std::string, size_t> at;
    size_t cur = (size_t)-1;
    for (size_t i = 0; i < s.size();) {
        size_t j = s.find('\n', i);
        if (j == std::string::npos) j = s.size();
        size_t e = j;
        while (e > i && s[e - 1] == '\r') --e;
        if (e > i && s[i] == '>') {
            std::string name(s, i + 1, e - i - 1);
            auto it = at.find(name);
            if (it == at.end()) {
                cur = out.size();
                at.emplace(name, cur);
                out.emplace_back(std::move(name), "");
            } else {
                cur = it->second;
                out[cur].second.clear();
            }
        } else if (cur != (size_t)-1) {
            out[cur].second.append(s, i, e - i);
        }
        i = j + 1;
    }
    return out;
}

}  // namespace

void fa2fq_free(bsk_ctx* c) {
    if (!c->fa2fq) return;
    if (c->fa2fq->d_blob) hipFree(c->fa2fq->d_blob);
    if (c->fa2fq->d_comp) hipFree(c->fa2fq->d_comp);
    delete c->fa2fq;
    c->fa2fq = nullptr;
}

void validate_fa2fq_opts(bsk_ctx* c) {
    const Options& o = c->opts;
    c->alphabet = alphabet_from_seqtype(o.cs("SeqType"));
    check_id_regexp(c);
    const std::string& file = o.s("FastaFile");
    if (file.empty()) throw OptError("flag -f (--fasta-file) needed");
    std::unique_ptr<Fa2FqState> S(new Fa2FqState());
    S->recs = read_fasta_map(file);
    if (S->recs.empty()) throw OptError("no sequences found in fasta file: " + file);
    if (S->recs.size() >= FA2FQ_MINUS)
        throw OptError("libbsk: fa2fq: " + std::to_string(S->recs.size()) + " FASTA records; the HIP path indexes fewer than 2^31");
    c->info(std::to_string(S->recs.size()) + " sequences loaded", true);
    fa2fq_free(c);
    c->fa2fq = S.release();
}

namespace {

// the table on the device: keys | idx | name_off | seq_off | names | seqs (+ 16 bytes: the compares read 8 at a time)
int upload(bsk_ctx* c, hipStream_t st) {
    Fa2FqState& S = *c->fa2fq;
    if (S.d_blob) return BSK_OK;
    const size_t ne = S.recs.size();
    uint64_t cap = 1;
    while (cap < 2 * ne + 2) cap <<= 1;
    uint64_t names_n = 0, seqs_n = 0;
    for (auto& r : S.recs) { names_n += r.first.size(); seqs_n += r.second.size(); }
    auto up16 = [](uint64_t x) { return (x + 15) & ~15ull; };
    const uint64_t a_keys = 0, a_idx = a_keys + cap * 8, a_noff = up16(a_idx + cap * 4), a_soff = a_noff + (ne + 1) * 8,
                   a_names = a_soff + (ne + 1) * 8, a_seqs = up16(a_names + names_n), total = a_seqs + seqs_n + 16;
    std::vector<uint8_t> blob(total, 0);
    uint64_t* keys = reinterpret_cast<uint64_t*>(blob.data() + a_keys);
    uint32_t* idx = reinterpret_cast<uint32_t*>(blob.data() + a_idx);
    uint64_t* noff = reinterpret_cast<uint64_t*>(blob.data() + a_noff);
    uint64_t* soff = reinterpret_cast<uint64_t*>(blob.data() + a_soff);
    uint64_t np = 0, sp = 0;
    for (size_t e = 0; e < ne; ++e) {
        const auto& r = S.recs[e];
        noff[e] = np; soff[e] = sp;
        if (!r.first.empty()) memcpy(blob.data() + a_names + np, r.first.data(), r.first.size());
        if (!r.second.empty()) memcpy(blob.data() + a_seqs + sp, r.second.data(), r.second.size());
        np += r.first.size(); sp += r.second.size();
        const uint64_t h = fnv1a64_host(r.first);
        uint64_t s = h & (cap - 1);
        while (keys[s]) s = (s + 1) & (cap - 1);
        keys[s] = h; idx[s] = (uint32_t)e;
    }
    noff[ne] = np; soff[ne] = sp;
    // beside the shard and whatever the context holds: a table that does not fit is refused, never cut
    if (hipMalloc((void**)&S.d_blob, total) != hipSuccess) {
        (void)hipGetLastError();
        S.d_blob = nullptr;
        c->set_error("libbsk: fa2fq: the FASTA table (" + std::to_string(total) + " bytes for " + std::to_string(ne) +
                     " records) does not fit into device memory beside the shard");
        return BSK_ERR_UNSUPPORTED;
    }
    if (!S.d_comp) HIP_TRYX(c, hipMalloc((void**)&S.d_comp, 256 + 16));
    HIP_TRYX(c, hipMemcpyAsync(S.d_blob, blob.data(), total, hipMemcpyHostToDevice, st));
    HIP_TRYX(c, hipStreamSynchronize(st));
    std::vector<std::pair<std::string, std::string>>().swap(S.recs);  // (the device copy is the table from here on)
    uint8_t* b = S.d_blob;
    Fa2FqParams& P = S.P;
    memset(&P, 0, sizeof P);
    P.keys = reinterpret_cast<const uint64_t*>(b + a_keys);
    P.idx = reinterpret_cast<const uint32_t*>(b + a_idx);
    P.mask = cap - 1;
    P.name_off = reinterpret_cast<const uint64_t*>(b + a_noff);
    P.names = b + a_names;
    P.seq_off = reinterpret_cast<const uint64_t*>(b + a_soff);
    P.seqs = b + a_seqs;
    P.comp = S.d_comp;
    P.ctl = reinterpret_cast<unsigned long long*>(S.d_comp + 256);
    return BSK_OK;
}

}  // namespace

int fa2fq_run_device(bsk_ctx* c, const uint8_t* d_buf, size_t n, int format, hipStream_t st, bsk_out* out) {
    out->d_data = nullptr; out->len = 0; out->records = 0;
    int rc = build_index(c, d_buf, n, format, st);
    if (rc != BSK_OK) return rc;
    if (c->table.n == 0) return empty_result(c, out);
    if (format != BSK_FORMAT_FASTQ) { c->set_error("this command only works for FASTQ format"); return BSK_ERR_FORMAT; }
    rc = upload(c, st);
    if (rc != BSK_OK) return rc;
    Fa2FqState& S = *c->fa2fq;
    // the '-' strand is Seq.RevComInplace of the partition's alphabet, whatever it is (PARITY.md ALPHA; protein: reversed only)
    Alphabet ab = partition_alphabet(c, d_buf, n, format, st, &rc);
    if (rc != BSK_OK) return rc;
    struct { uint8_t comp[256]; uint64_t ctl[2]; } h;
    complement_table(ab, h.comp);
    h.ctl[0] = 0; h.ctl[1] = ~0ull;
    HIP_TRYX(c, hipMemcpyAsync(S.d_comp, &h, sizeof h, hipMemcpyHostToDevice, st));
    HIP_TRYX(c, hipStreamSynchronize(st));  // h lives on the host stack
    Fa2FqParams P = S.P;
    P.only_plus = c->opts.b("OnlyPositiveStrand");
    P.id_mode = id_mode_of(c);
    P.buf_end = d_buf + n;
    const uint64_t N = c->table.n;
    rc = ensure_record_scratch(c);
    if (rc != BSK_OK) return rc;
    Arena A;
    const uint64_t o_ent = A.take(N * 4), o_pos = A.take(N * 4), o_list = A.take(N * 4);
    rc = arena_reserve(c, &A);
    if (rc != BSK_OK) return rc;
    uint32_t* d_ent = A.at<uint32_t>(o_ent);
    uint32_t* d_pos = A.at<uint32_t>(o_pos);
    uint32_t* d_list = A.at<uint32_t>(o_list);
    {
        Timed t(c, "k_fa2fq_match", st);
        HIP_TRYX(c, launch_fa2fq_match(d_buf, c->table, P, d_ent, d_pos, c->d_out_len, d_list, st));
    }
    uint64_t total = 0, kept = 0;
    rc = finish_sizes(c, st, &total, &kept);
    if (rc != BSK_OK) return rc;
    HIP_TRYX(c, hipMemcpyAsync(h.ctl, P.ctl, sizeof h.ctl, hipMemcpyDeviceToHost, st));
    HIP_TRYX(c, hipStreamSynchronize(st));
    if (h.ctl[1] != ~0ull) {
        c->set_error("libbsk: fa2fq: the output of record " + std::to_string(h.ctl[1] + 1) +
                     " would reach 2^32 bytes (the HIP path writes records below 4 GiB)");
        return BSK_ERR_UNSUPPORTED;
    }
    rc = ensure_out(c, total);
    if (rc != BSK_OK) return rc;
    {
        Timed t(c, "k_fa2fq_emit", st);
        HIP_TRYX(c, launch_fa2fq_emit(d_buf, c->table, P, d_ent, d_pos, c->d_out_len, c->d_out_off, c->d_out, c->d_long_list,
                                      c->long_count, c->long_max, c->long_thresh, st));
    }
    out->d_data = c->d_out;
    out->len = total;
    out->records = kept;
    return BSK_OK;
}

}  // namespace bsk
