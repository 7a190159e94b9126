// Where `world` workers cut a BGZF file (PARITY.md BGZF "workers").  This header is the host rule:
// the candidate scan, the chain test and the record cut, over fetch(offset, len, dst).  Like bgzf_stream.hpp it needs nothing of
// the HIP runtime -- tests/host_c/bgzf_cuts_check.cpp builds it alone under the host's sanitizers -- and it restates nothing: the
// header parse is bgzf::parse_header, the decoder the host lane of bgzf_inflate_dev.hpp, the record rule find_fastq_cut /
// find_fasta_start (bsk_find_record_start).
//
// size: the file's bytes.  The block chain is the walk from offset 0, next = offset + BSIZE + 1.  For k = 1 .. world - 1:
//   lo_k = max(floor(size * k / world), B_{k-1}), B_0 = 0;  B_k = the first offset of the chain at or behind lo_k, or size;
//   V_k  = the virtual offset of the first record start at or behind the first text byte of B_k;
//   V_0  = the start of the text, V_world = size << 16; all normalised (never in an empty block, never at a block's end).
// The chain from 0 is not walked.  Every position of [max(0, lo_k - BGZF_CUT_BACK), lo_k] that parses as a block header is a
// candidate; it is kept if its BSIZE chain reaches a position at or behind lo_k through blocks that lie in the file and decode
// with the right CRC32 and ISIZE, and if the block there decodes as well (or the file ends there).  A true block start always
// passes, so the first candidate kept names a position of the chain unless a block's data holds a whole valid block -- which
// the worker's own walk finds out (the join check of bgzf_shard_load_device): a wrong candidate costs time or an explicit
// refusal, never bytes.  No candidate kept: the file is damaged there (BSK_ERR_FORMAT, the offsets named).
// The text of the chain's blocks in front of B_k is the look-behind of the record rule; the window behind it grows as the
// window of a plain file's cut does: the answer must be the same under a window four times as large and must not lie within
// 64 KiB of the window's end unless the text ends there.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../include/bsk.h"
#include "anchor.hpp"
#include "bgzf_inflate_dev.hpp"

namespace bsk {

constexpr uint64_t BGZF_CUT_BACK = 1ull << 20;    // compressed bytes in front of lo_k that are scanned for candidates
constexpr uint64_t BGZF_CUT_WINDOW = 1ull << 20;  // text bytes on either side of the cut that the record rule sees first

// bytes [off, off + len) of the file into dst; false: they cannot be read
using BgzfFetch = std::function<bool(uint64_t off, size_t len, uint8_t* dst)>;

class BgzfCutter {
public:
    BgzfCutter(BgzfFetch fetch, uint64_t size, int format) : fetch_(std::move(fetch)), size_(size), format_(format), S_(new bgzf::BgzfLds) {
        memset(S_->crc_mat, 0, sizeof S_->crc_mat);  // (one chunk per block on the host: never applied)
    }
    const std::string& error() const { return err_; }

    // voffs[0 .. world]
    int cut_points(int world, uint64_t* voffs) {
        if (world < 1 || !voffs) return fail(BSK_ERR_INVALID_ARG, "libbsk: bgzf: cut points need at least one worker");
        const uint64_t end = size_ << 16;
        int rc = text_start(&voffs[0]);
        if (rc != BSK_OK) return rc;
        uint64_t B = 0, lo_before = 0;
        for (int k = 1; k < world; ++k) {
            const uint64_t nominal = (uint64_t)((unsigned __int128)size_ * (unsigned)k / (unsigned)world);
            const uint64_t lo = std::max(nominal, B);
            if (lo >= size_) { voffs[k] = end; B = size_; continue; }
            if (k > 1 && lo == lo_before) { voffs[k] = voffs[k - 1]; continue; }  // (more workers than blocks: the same cut again)
            uint64_t V = 0;
            rc = cut(lo, &B, &V);
            if (rc != BSK_OK) return rc;
            lo_before = B;  // (lo_{k+1} == B_k names B_k again)
            voffs[k] = std::max(V, voffs[k - 1]);
        }
        voffs[world] = end;
        return BSK_OK;
    }

private:
    struct Blk { uint64_t coff; uint32_t csize, usize; };

    int fail(int rc, const std::string& m) { err_ = m; return rc; }

    // the file's bytes [off, off + len) through a window that is read ahead (chains run forward)
    const uint8_t* bytes(uint64_t off, size_t len) {
        if (off < win_off_ || off + len > win_off_ + win_.size()) {
            const uint64_t n = std::min<uint64_t>(size_ - off, std::max<uint64_t>(len, (uint64_t)4 << 20));
            win_.resize((size_t)n);
            win_off_ = off;
            if (n && !fetch_(off, (size_t)n, win_.data())) { win_.clear(); return nullptr; }
        }
        return win_.data() + (off - win_off_);
    }

    // 1: a whole block lies at off and decodes (*b; its text behind *text if given); 0: not so (*why); -1: the file cannot be read
    int block_at(uint64_t off, Blk* b, std::vector<uint8_t>* text, std::string* why) {
        const size_t len = (size_t)std::min<uint64_t>(size_ - off, 65536);
        const uint8_t* p = len ? bytes(off, len) : nullptr;
        if (len && !p) return -1;
        bgzf::BlockHeader h{0, 0};
        const int r = parse_header(p, len);
        if (r == 1) (void)bgzf::parse_header(p, len, &h);
        if (r == -1) { *why = "truncated: the file ends inside the block header"; return 0; }
        if (r != 1) { *why = "the bytes are not a block header"; return 0; }
        if (h.bsize < 12u + h.xlen + 8u) { *why = "BSIZE is smaller than the header and the trailer"; return 0; }
        if (h.bsize > len) { *why = "truncated: BSIZE reaches past the end of the file"; return 0; }
        const uint8_t* t = p + h.bsize - 8;
        const uint32_t crc = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
        const uint32_t isize = t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
        if (isize > bgzf::MAX_ISIZE) { *why = bgzf::error_text(bgzf::ERR_ISIZE); return 0; }
        out_.resize(bgzf::MAX_ISIZE + 16);
        bgzf::HostLane io{p, len, out_.data()};
        bgzf::Inflater<bgzf::HostLane> I(io, *S_);
        const int e = I.run(12u + h.xlen, h.bsize - 8u, isize, crc, 0);
        if (e != bgzf::OK) { *why = bgzf::error_text(e); return 0; }
        *b = Blk{off, h.bsize, isize};
        if (text) text->insert(text->end(), out_.begin(), out_.begin() + isize);
        return 1;
    }
    static int parse_header(const uint8_t* p, size_t len) {
        bgzf::BlockHeader h{0, 0};
        return len ? bgzf::parse_header(p, len, &h) : 0;
    }
    int unreadable() { return fail(BSK_ERR_INVALID_ARG, "libbsk: bgzf: reading the file failed"); }
    static std::string at(uint64_t off) { return "libbsk: bgzf: block at offset " + std::to_string(off); }

    // V_0: the first block that holds text, walked from offset 0 (which is a block start by definition)
    int text_start(uint64_t* v) {
        uint64_t no = 0;
        for (uint64_t off = 0; off < size_; ++no) {
            Blk b{};
            std::string why;
            const int r = block_at(off, &b, nullptr, &why);
            if (r < 0) return unreadable();
            if (r == 0) {
                if (off == 0) {
                    const int kind = parse_header(bytes(0, (size_t)std::min<uint64_t>(size_, 65536)), (size_t)std::min<uint64_t>(size_, 65536));
                    if (kind == 2) return fail(BSK_ERR_UNSUPPORTED, "libbsk: bgzf: the input is gzip but not BGZF: one gzip stream cannot be cut into independent blocks; recompress it with bgzip");
                    if (kind == 0) return fail(BSK_ERR_FORMAT, "libbsk: bgzf: the input is not gzip");
                }
                return fail(BSK_ERR_FORMAT, "libbsk: bgzf: block " + std::to_string(no) + " at offset " + std::to_string(off) + ": " + why);
            }
            if (b.usize) { *v = off << 16; return BSK_OK; }
            off += b.csize;
        }
        *v = size_ << 16;
        return BSK_OK;
    }

    // B: the first position at or behind lo that a candidate's chain reaches; V: the record start at or behind its text
    int cut(uint64_t lo, uint64_t* B_out, uint64_t* V_out) {
        const uint64_t s = lo > BGZF_CUT_BACK ? lo - BGZF_CUT_BACK : 0;
        std::vector<uint8_t> text;  // the chain's text in front of B, then the text from B on
        std::vector<Blk> fwd;       // the blocks from B on
        uint64_t B = 0, next = 0;   // next: the block behind the last one of fwd
        bool found = false;
        uint64_t broke_at = s;
        std::string broke_why = "no position there parses as a block header";
        std::vector<uint64_t> visited;
        for (uint64_t p = s; p <= lo && !found; ++p) {
            const size_t have = (size_t)std::min<uint64_t>(size_ - p, 4);
            const uint8_t* hp = bytes(p, have);
            if (!hp) return unreadable();
            if (have < 4 || hp[0] != 0x1f || hp[1] != 0x8b || hp[2] != 8 || !(hp[3] & 4)) continue;
            if (bad_.count(p)) continue;
            text.clear();
            visited.clear();
            uint64_t q = p;
            bool ok = true;
            while (ok && q < lo) {
                Blk b{};
                std::string why;
                visited.push_back(q);
                const int r = bad_.count(q) ? 0 : block_at(q, &b, &text, &why);
                if (r < 0) return unreadable();
                if (r == 0) {
                    if (!why.empty()) { broke_at = q; broke_why = why; }
                    ok = false;
                    break;
                }
                q += b.csize;
            }
            if (ok && q < size_) {  // the block at the position itself
                const size_t from = text.size();
                Blk b{};
                std::string why;
                visited.push_back(q);
                const int r = bad_.count(q) ? 0 : block_at(q, &b, &text, &why);
                if (r < 0) return unreadable();
                if (r == 0) {
                    if (!why.empty()) { broke_at = q; broke_why = why; }
                    ok = false;
                } else {
                    fwd.assign(1, b);
                    next = q + b.csize;
                    from_ = from;
                }
            } else if (ok) {
                from_ = text.size();
                fwd.clear();
                next = size_;
            }
            if (!ok) {  // (every position of a chain that breaks is on a chain that breaks)
                for (uint64_t v : visited) bad_.insert(v);
                continue;
            }
            B = q;
            found = true;
        }
        if (!found)
            return fail(BSK_ERR_FORMAT, "libbsk: bgzf: the file is damaged around offset " + std::to_string(lo) + ": no chain of whole blocks from a block header in [" +
                                            std::to_string(s) + ", " + std::to_string(lo) + "] reaches a block start in [" + std::to_string(lo) + ", " +
                                            std::to_string(lo + 65536) + "]; the last chain broke at offset " + std::to_string(broke_at) + ": " + broke_why);
        *B_out = B;
        if (B == size_) { *V_out = size_ << 16; return BSK_OK; }
        // ---- the record start: the window grows until the answer stands
        const uint64_t from = from_;
        uint64_t no = 1;  // (the number of the block at `next`, counted from B)
        auto extend = [&](uint64_t want) -> int {  // text up to from + want, or the end of the file
            while (next < size_ && text.size() < from + want) {
                Blk b{};
                std::string why;
                const int r = block_at(next, &b, &text, &why);
                if (r < 0) return unreadable();
                if (r == 0) return fail(BSK_ERR_FORMAT, at(next) + " (number " + std::to_string(no) + " from the cut at offset " + std::to_string(B) + "): " + why);
                fwd.push_back(b);
                next += b.csize;
                ++no;
            }
            return BSK_OK;
        };
        auto look = [&](uint64_t w, uint64_t* b_out, uint64_t* cut_out) -> int {
            const int rc = extend(w);
            if (rc != BSK_OK) return rc;
            const uint64_t a = from > w ? from - w : 0, b = std::min<uint64_t>(text.size(), from + w);
            const uint8_t* t = text.data() + a;
            const uint64_t n = b - a;
            const uint64_t c = n == 0 ? 0 : (format_ == BSK_FORMAT_FASTQ ? find_fastq_cut(t, n, from - a) : find_fasta_start(t, n, from - a));
            *b_out = b;
            *cut_out = std::min(c, n) + a;
            return BSK_OK;
        };
        uint64_t cutpos = 0;
        for (uint64_t w = BGZF_CUT_WINDOW;; w *= 4) {
            uint64_t b = 0, b4 = 0, c4 = 0;
            int rc = look(w, &b, &cutpos);
            if (rc != BSK_OK) return rc;
            const bool at_end = next >= size_ && b == text.size();
            if (at_end) break;
            if (cutpos + (64u << 10) > b) continue;
            rc = look(w * 4, &b4, &c4);
            if (rc != BSK_OK) return rc;
            if (c4 == cutpos) break;
        }
        // ---- its virtual offset, normalised
        uint64_t r = cutpos - from, V = size_ << 16;
        for (;;) {
            bool placed = false;
            uint64_t cum = 0;
            for (const Blk& b : fwd) {
                if (b.usize && r < cum + b.usize) { V = b.coff << 16 | (r - cum); placed = true; break; }
                cum += b.usize;
            }
            if (placed || next >= size_) break;
            const int rc = extend(text.size() - from + 1);  // (the cut is the end of the window's text: the next block that holds text)
            if (rc != BSK_OK) return rc;
        }
        *V_out = V;
        return BSK_OK;
    }

    BgzfFetch fetch_;
    uint64_t size_;
    int format_;
    std::unique_ptr<bgzf::BgzfLds> S_;
    std::string err_;
    std::vector<uint8_t> win_, out_;
    uint64_t win_off_ = 0;
    uint64_t from_ = 0;                 // cut(): where the text of B begins in the chain's text (set by the candidate that is kept)
    std::unordered_set<uint64_t> bad_;  // positions whose chain breaks
};

}  // namespace bsk
