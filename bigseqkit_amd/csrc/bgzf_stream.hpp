// A BGZF file as record-aligned pieces of its text (PARITY.md BGZF "pieces"): the file is never
// held whole, compressed or inflated.  This header is the definition -- which blocks are inflated, where a piece ends, what a
// virtual offset means -- written once over a small backend: where the compressed bytes land, who decodes a list of blocks,
// who moves the carried head, who finds the cut.  HostBackend (below) is the decoder of bgzf_inflate_dev.hpp with host
// buffers; the device's backend lives in ops_bgzf_stream.hip.  Nothing here needs the HIP runtime: tests/host_c/
// bgzf_stream_check.cpp builds this header alone under the host's sanitizers.
//
// Positions are BGZF virtual offsets: coffset << 16 | uoffset, coffset the file offset of a block and uoffset < ISIZE a byte
// of its text.  The reader hands out normalised ones: never the end of a block, never an empty block; the end of the text is
// file_size << 16.
//
// The pieces are a function of the text and the block ends, not of the chunk size and not of the backend.  For a piece that
// starts at text offset s:
//   1. whole blocks are inflated in file order up to E, the first block end with E - s >= piece + lookahead (blocks of
//      ISIZE 0 behind it belong to it), or the end of the text;
//   2. E the end of the text: the piece is the rest;
//   3. else the piece ends at c = the record start that bsk_find_record_start names on text[s, E) from `piece`;
//   4. no start before E: E moves on by whole blocks, the lookahead doubled, and 2. and 3. are asked again;
//   5. text[c, E) is the head of the next piece.
#pragma once
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/bsk.h"
#include "anchor.hpp"
#include "bgzf_inflate_dev.hpp"
#include "ops_bgzf.hpp"

namespace bsk {

// ---- the cut as the device finds it: the answer of the host rule, or "declined" -------------------------------------------
constexpr uint64_t CUT_DECLINED = ~0ull;

// a strict four-line record at p that the wrapped grammar (fastq_multiline_record_end) reads as the same record: bases on one
// line that is not empty and does not begin with '@'.  Returns the byte behind its quality line (n: the text ends there), 0: no
BSK_HD uint64_t fastq_plain_record_end(const uint8_t* buf, uint64_t n, uint64_t p) {
    if (!fastq_record_at(buf, n, p)) return 0;
    const uint64_t s0 = find_byte(buf, n, p, '\n') + 1, e1 = find_byte(buf, n, s0, '\n');
    if (e1 == s0 || buf[s0] == '@') return 0;
    const uint64_t q0 = find_byte(buf, n, e1 + 1, '\n') + 1, e3 = find_byte(buf, n, q0, '\n');
    return e3 < n ? e3 + 1 : n;
}

// The host rule on text[0, n) from `from` >= 1 is find_fasta_start / find_fastq_cut (bsk_find_record_start).  FASTA: the same
// function.  FASTQ: find_fastq_cut asks the wrapped grammar first, which looks at three records in a row and at the record in
// front; this function answers p only where that reading provably names p as well --
//   * no line between `from` and p begins with '@' (the wrapped rule tries nothing else, so it accepts nothing in front of p),
//   * p and the records behind it, up to three or the end of the text, are plain four-line records (fastq_multiline_record_at),
//   * the four lines in front of p are one plain record that ends at p, and none of its other lines begins with '@'
//     (fastq_multiline_prev_agrees walks back over exactly these lines and stops at that record)
// -- and declines everything else: wrapped text, a quality line that begins with '@' at the cut, a blank line, a window that
// begins too late.  n: no line in [from, n) begins with '@', so neither rule finds a start.
BSK_HD uint64_t stream_cut(const uint8_t* buf, uint64_t n, uint64_t from, int format) {
    if (from == 0 || from >= n) return CUT_DECLINED;
    if (format != BSK_FORMAT_FASTQ) return find_fasta_start(buf, n, from);
    uint64_t p = n;
    for (uint64_t j = find_byte(buf, n, from - 1, '\n'); j < n; j = find_byte(buf, n, j + 1, '\n')) {
        if (j + 1 < n && buf[j + 1] == '@') {
            if (!fastq_record_at(buf, n, j + 1)) return CUT_DECLINED;
            p = j + 1;
            break;
        }
        if (j >= from + ANCHOR_SEARCH_BYTES) return CUT_DECLINED;
    }
    if (p == n) return n;
    uint64_t q = p;
    for (int k = 0; k < 3; ++k) {
        const uint64_t e = fastq_plain_record_end(buf, n, q);
        if (e == 0) return CUT_DECLINED;
        q = e;
        while (q < n && buf[q] == '\n') ++q;
        if (q >= n) break;
    }
    // the record in front: quality, '+', bases, header -- four line starts back from p
    if (p < 2 || buf[p - 2] == '\n') return CUT_DECLINED;
    uint64_t s = p - 1;
    for (int line = 0; line < 4; ++line) {
        if (s == 0) return CUT_DECLINED;
        uint64_t b = s - 1;  // (s: the line feed that ends the line)
        while (b > 0 && buf[b - 1] != '\n') --b;
        if (b == 0 && line < 3) return CUT_DECLINED;
        if (line < 3) {
            if (buf[b] == '@') return CUT_DECLINED;
            s = b - 1;
        } else if (fastq_plain_record_end(buf, n, b) != p) {
            return CUT_DECLINED;
        }
    }
    return p;
}

// ---- the backend ------------------------------------------------------------------------------------------------------------
// Two compressed slots and two text buffers.  A slot holds FRONT bytes of room for the block that began in the chunk before,
// then the chunk.  A text buffer holds FRONT bytes of room in front of the piece (a piece that begins inside a block has the
// block's first bytes there), so a piece always begins at text(b) + FRONT, a multiple of 256 from the buffer's start.
struct BgzfStreamBackend {
    static constexpr size_t FRONT = 65536;
    std::string err;
    virtual ~BgzfStreamBackend() {}
    virtual int open(size_t chunk_bytes, size_t text_cap) = 0;
    virtual uint8_t* comp_host(int slot) = 0;                                         // the host's view of a slot (FRONT + chunk bytes)
    virtual int start_read(int slot, int fd, uint64_t file_off, size_t len) = 0;      // bytes of the file to comp_host(slot) + FRONT and on
    virtual int wait_read(int slot, size_t* got) = 0;
    virtual int push_front(int slot, size_t left) = 0;                                // comp_host(slot)[FRONT - left, FRONT) follows
    // the blocks d[0, nb) of `slot` (d.coff: offset in the slot, d.ooff: offset in the text buffer) inflated; *bad: ~0 or index << 8 | code
    virtual int inflate(int slot, size_t slot_bytes, const BgzfBlockDesc* d, size_t nb, int tbuf, uint64_t* bad) = 0;
    virtual size_t text_cap(int tbuf) const = 0;
    virtual int text_grow(int tbuf, size_t cap, size_t keep) = 0;                     // at least cap bytes, the first `keep` kept
    virtual const uint8_t* text(int tbuf) const = 0;
    virtual int reuse(int tbuf) = 0;                                                  // what reads the buffer now is waited for before it is written
    virtual int move(int from, size_t from_off, int to, size_t to_off, size_t n) = 0;
    // the record start of text(tbuf)[FRONT, FRONT + n) from `from` by the host rule (n: none)
    virtual int find_cut(int tbuf, uint64_t n, uint64_t from, int format, uint64_t* cut) = 0;
    virtual int sync() = 0;
};

// ---- the reader -------------------------------------------------------------------------------------------------------------
class BgzfPieceReader {
public:
    BgzfPieceReader(std::unique_ptr<BgzfStreamBackend> backend, int fd, uint64_t file_size, int format, size_t piece, size_t look, size_t chunk)
        : B(std::move(backend)), fd_(fd), fsize_(file_size), format_(format), piece_(piece ? piece : (size_t)1 << 30),
          look_(look ? look : (size_t)1 << 20), chunk_(chunk ? chunk : (size_t)256 << 20) {}
    int open() {
        // (a small file needs neither a full chunk nor room for a full piece: DEFLATE packs at most 1032 bytes into one)
        const uint64_t most_text = fsize_ < ((uint64_t)1 << 40) ? fsize_ * 1032 : ~0ull >> 2;
        const int rc = B->open((size_t)std::min<uint64_t>(chunk_, std::max<uint64_t>(fsize_, 1)),
                               FRONT + (size_t)std::min<uint64_t>((uint64_t)piece_ + look_, most_text) + 65536 + 16);
        if (rc != BSK_OK) return fail(rc, B->err);
        return seek(0);
    }
    const std::string& error() const { return err_; }
    uint64_t end_voff() const { return fsize_ << 16; }

    int seek(uint64_t voff) {
        const uint64_t coff = voff >> 16;
        if (coff > fsize_ || (coff == fsize_ && (voff & 0xFFFFu))) return fail(BSK_ERR_INVALID_ARG, "libbsk: bgzf: the virtual offset lies behind the end of the file");
        if (read_pending_) {  // (what was on its way belongs to another place)
            size_t got = 0;
            (void)B->wait_read(slot_ ^ 1, &got);
            read_pending_ = false;
        }
        failed_ = BSK_OK;
        blks_.clear();
        have_ = -(int64_t)(voff & 0xFFFFu);
        skip_ = (uint32_t)(voff & 0xFFFFu);
        head_off_ = FRONT;
        carry_moved_ = true;
        at_eof_ = coff == fsize_;
        c_at_ = c_end_ = FRONT;
        read_off_ = next_off_ = coff;
        const auto it = known_.find(coff);
        blk_known_ = coff == 0 || it != known_.end();
        blk_no_ = coff == 0 ? 0 : (blk_known_ ? it->second : 0);
        return BSK_OK;
    }

    // the next piece by the rule; *last: the text ends with it (further calls give empty last pieces)
    int next(const void** ptr, size_t* n, uint64_t* voff_lo, uint64_t* voff_hi, int* last) {
        if (failed_ != BSK_OK) return failed_;
        int rc = begin_piece();
        if (rc != BSK_OK) return rc;
        uint64_t look = look_, cut = 0;
        for (;;) {
            const uint64_t need = (uint64_t)piece_ + look;
            rc = fill([&](const Blk& h, int64_t queued) { return queued >= (int64_t)need && h.usize != 0; });
            if (rc != BSK_OK) return rc;
            if (at_eof_) { cut = (uint64_t)std::max<int64_t>(have_, 0); break; }
            rc = B->find_cut(tb_, (uint64_t)have_, piece_, format_, &cut);
            if (rc != BSK_OK) return fail(rc, B->err);
            if (cut < (uint64_t)have_) break;
            look *= 2;
        }
        return end_piece(cut, ptr, n, voff_lo, voff_hi, last);
    }

    // the bytes [voff_lo, voff_hi) again (both as next gave them)
    int piece(uint64_t voff_lo, uint64_t voff_hi, const void** ptr, size_t* n) {
        if (voff_hi < voff_lo || (voff_hi >> 16) > fsize_) return fail(BSK_ERR_INVALID_ARG, "libbsk: bgzf: bad virtual offsets of a piece");
        if (failed_ != BSK_OK || position() != voff_lo) {
            const int rc = seek(voff_lo);
            if (rc != BSK_OK) return rc;
        }
        int rc = begin_piece();
        if (rc != BSK_OK) return rc;
        const uint64_t chi = voff_hi >> 16, uhi = voff_hi & 0xFFFFu;
        rc = fill([&](const Blk& h, int64_t) { return h.coff > chi || (h.coff == chi && uhi == 0); });
        if (rc != BSK_OK) return rc;
        uint64_t cut = (uint64_t)std::max<int64_t>(have_, 0);
        if (chi < fsize_) {
            bool found = uhi == 0 && !at_eof_ && file_off(c_at_) == chi;  // (the piece ends where the next block begins)
            for (const Blk& b : blks_)
                if (b.coff == chi && uhi < b.usize && b.tstart + (int64_t)uhi >= 0) { cut = (uint64_t)(b.tstart + (int64_t)uhi); found = true; break; }
            if (!found) return fail(BSK_ERR_INVALID_ARG, "libbsk: bgzf: the end of the piece is not a position of the file's text");
        }
        uint64_t lo = 0, hi = 0;
        int last = 0;
        return end_piece(cut, ptr, n, &lo, &hi, &last);
    }

private:
    static constexpr size_t FRONT = BgzfStreamBackend::FRONT;
    struct Blk { uint64_t coff, no; int64_t tstart; uint32_t usize, csize; };  // (no: its number; tstart: where its text lies from the piece's start)

    int fail(int rc, const std::string& m) { err_ = m; failed_ = rc; return rc; }
    std::string where(uint64_t off) const { return where(blk_no_, off); }
    std::string where(uint64_t no, uint64_t off) const {
        if (blk_known_) return "libbsk: bgzf: block " + std::to_string(no) + " at offset " + std::to_string(off) + ": ";
        return "libbsk: bgzf: block at offset " + std::to_string(off) + " (number " + std::to_string(no) + " from the seek): ";
    }
    uint64_t file_off(size_t idx) const { return read_off_ + idx - FRONT; }  // (idx < FRONT: the bytes carried from the chunk before)

    // where the text at the head stands
    uint64_t position() const {
        for (const Blk& b : blks_)
            if (b.tstart + (int64_t)b.usize > 0) return b.coff << 16 | (uint64_t)(-std::min<int64_t>(b.tstart, 0));
        if (at_eof_) return end_voff();
        return (file_off(c_at_) << 16) | skip_;
    }

    // the other text buffer becomes the current one, the carried head at its front
    int begin_piece() {
        if (carry_moved_) {  // (behind a seek: nothing is carried, but the piece before stays valid as after any call)
            tb_ ^= 1;
            const int rc = B->reuse(tb_);
            if (rc != BSK_OK) return fail(rc, B->err);
            carry_moved_ = false;
            return BSK_OK;
        }
        const size_t carry = (size_t)std::max<int64_t>(have_, 0);
        int rc = B->reuse(tb_ ^ 1);
        if (rc == BSK_OK && B->text_cap(tb_ ^ 1) < FRONT + carry + 16) rc = B->text_grow(tb_ ^ 1, FRONT + carry + 16, 0);
        if (rc == BSK_OK && carry) rc = B->move(tb_, head_off_, tb_ ^ 1, FRONT, carry);
        if (rc != BSK_OK) return fail(rc, B->err);
        tb_ ^= 1;
        head_off_ = FRONT;
        return BSK_OK;
    }

    // the piece is text[0, cut) of the current buffer; what lies behind stays as the head of the next
    int end_piece(uint64_t cut, const void** ptr, size_t* n, uint64_t* voff_lo, uint64_t* voff_hi, int* last) {
        const int rc = B->sync();
        if (rc != BSK_OK) return fail(rc, B->err);
        *voff_lo = position();
        *ptr = B->text(tb_) + FRONT;
        *n = (size_t)cut;
        while (!blks_.empty() && blks_.front().tstart + (int64_t)blks_.front().usize <= (int64_t)cut) blks_.pop_front();
        for (Blk& b : blks_) b.tstart -= (int64_t)cut;
        have_ -= (int64_t)cut;
        head_off_ = FRONT + (size_t)cut;
        skip_ = 0;
        *voff_hi = position();
        *last = at_eof_ && have_ <= 0;
        if (blk_known_) known_[*voff_hi >> 16] = blks_.empty() ? blk_no_ : blks_.front().no;  // (a later seek to this boundary counts on)
        return BSK_OK;
    }

    // 1: the block at c_at_ lies whole in the slot (*h); 0: the file ends in front of it; < 0 - code: refused.  Moves to the next
    // chunk where the slot ends inside the block, after `flush`
    template <class Flush>
    int peek_block(Blk* h, Flush flush) {
        for (;;) {
            const size_t avail = c_end_ - c_at_;
            const uint64_t off = file_off(c_at_);
            const bool more = file_off(c_end_) < fsize_;
            if (avail == 0 && !more) return 0;
            bgzf::BlockHeader bh{0, 0};
            const uint8_t* p = B->comp_host(slot_) + c_at_;
            const int r = avail ? bgzf::parse_header(p, avail, &bh) : -1;
            bool whole = false;
            if (r == 1) {
                if (bh.bsize < 12u + bh.xlen + 8u) return -fail(BSK_ERR_FORMAT, where(off) + "BSIZE is smaller than the header and the trailer");
                whole = bh.bsize <= avail;
                if (!whole && !more) return -fail(BSK_ERR_FORMAT, where(off) + "truncated: BSIZE reaches past the end of the file");
            } else if (r == -1 || (more && avail < 18)) {
                if (!more || avail >= 65536) return -fail(BSK_ERR_FORMAT, where(off) + "truncated: the file ends inside the block header");
            } else {
                if (off == 0 && r == 2) return -fail(BSK_ERR_UNSUPPORTED, "libbsk: bgzf: the input is gzip but not BGZF: one gzip stream cannot be cut into independent blocks; recompress it with bgzip");
                if (off == 0) return -fail(BSK_ERR_FORMAT, "libbsk: bgzf: the input is not gzip");
                return -fail(BSK_ERR_FORMAT, where(off) + "the bytes after the last block are not a block header");
            }
            if (whole) {
                const uint8_t* t = p + bh.bsize - 8;
                const uint32_t isize = t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
                if (isize > bgzf::MAX_ISIZE) return -fail(BSK_ERR_FORMAT, where(off) + bgzf::error_text(bgzf::ERR_ISIZE));
                *h = Blk{off, blk_no_, 0, isize, bh.bsize};
                xlen_ = bh.xlen;
                crc_ = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
                return 1;
            }
            // the slot ends inside the block: it is the first block of the next chunk
            int rc = flush();
            if (rc != BSK_OK) return -rc;
            const int ns = slot_ ^ 1;
            if (!read_pending_) {
                rc = B->start_read(ns, fd_, next_off_, (size_t)std::min<uint64_t>(chunk_, fsize_ - next_off_));
                if (rc != BSK_OK) return -fail(rc, B->err);
            }
            size_t got = 0;
            rc = B->wait_read(ns, &got);
            read_pending_ = false;
            if (rc != BSK_OK) return -fail(rc, B->err);
            if (got == 0) return -fail(BSK_ERR_INVALID_ARG, "libbsk: bgzf: the file became shorter while it was read");
            if (avail) {
                memcpy(B->comp_host(ns) + FRONT - avail, p, avail);
                rc = B->push_front(ns, avail);
                if (rc != BSK_OK) return -fail(rc, B->err);
            }
            slot_ = ns;
            read_off_ = next_off_;
            next_off_ += got;
            c_at_ = FRONT - avail;
            c_end_ = FRONT + got;
            if (next_off_ < fsize_) {  // chunk k + 1 is read and crosses to the device while chunk k is inflated
                rc = B->start_read(slot_ ^ 1, fd_, next_off_, (size_t)std::min<uint64_t>(chunk_, fsize_ - next_off_));
                if (rc != BSK_OK) return -fail(rc, B->err);
                read_pending_ = true;
            }
        }
    }

    // blocks are inflated behind the text at hand until stop(next block, text at hand and queued) or the end of the file
    template <class Stop>
    int fill(Stop stop) {
        std::vector<BgzfBlockDesc> q;
        std::vector<Blk> qb;
        int64_t queued = have_;
        auto flush = [&]() -> int {
            if (q.empty()) return BSK_OK;
            uint64_t bad = ~0ull;
            const int rc = B->inflate(slot_, c_end_, q.data(), q.size(), tb_, &bad);
            if (rc != BSK_OK) return fail(rc, B->err);
            if (bad != ~0ull) {
                const size_t k = (size_t)(bad >> 8);
                return fail(BSK_ERR_FORMAT, where(qb[k].no, qb[k].coff) + bgzf::error_text((int)(bad & 255u)));
            }
            for (const Blk& b : qb)
                if (b.usize) blks_.push_back(b);
            have_ = queued;
            q.clear();
            qb.clear();
            return BSK_OK;
        };
        while (!at_eof_) {
            Blk h{};
            const int r = peek_block(&h, flush);
            if (r < 0) return -r;
            if (r == 0) { at_eof_ = true; break; }
            if (stop(h, queued)) break;
            if (skip_ && queued < 0 && skip_ >= h.usize) return fail(BSK_ERR_INVALID_ARG, "libbsk: bgzf: the virtual offset points behind the text of its block");
            const size_t room = FRONT + (size_t)(queued + (int64_t)h.usize) + 16;
            if (room > B->text_cap(tb_)) {  // (a record longer than a piece, or a piece asked for by its offsets)
                int rc = flush();
                if (rc != BSK_OK) return rc;
                rc = B->text_grow(tb_, std::max(room, 2 * B->text_cap(tb_)), FRONT + (size_t)std::max<int64_t>(have_, 0));
                if (rc != BSK_OK) return fail(rc, B->err);
            }
            h.tstart = queued;
            q.push_back(BgzfBlockDesc{(uint64_t)c_at_, (uint64_t)((int64_t)FRONT + queued), h.csize, xlen_, h.usize, crc_});
            qb.push_back(h);
            queued += h.usize;
            c_at_ += h.csize;
            ++blk_no_;
        }
        return flush();
    }

    std::unique_ptr<BgzfStreamBackend> B;
    int fd_;
    uint64_t fsize_;
    int format_;
    size_t piece_, look_, chunk_;
    std::string err_;
    int failed_ = BSK_OK;
    // the compressed window: slot_ holds the file's bytes [file_off(c_at_), file_off(c_end_)), the next block begins at c_at_
    int slot_ = 0;
    size_t c_at_ = FRONT, c_end_ = FRONT;
    uint64_t read_off_ = 0, next_off_ = 0;  // the file offset of comp_host(slot_)[FRONT], and of the chunk that follows
    bool read_pending_ = false;
    uint64_t blk_no_ = 0;  // the number of the block at c_at_, counted over the whole file where the walk began at a known block
    bool blk_known_ = true;
    std::map<uint64_t, uint64_t> known_;  // block start -> block number, at the boundaries of the pieces handed out
    uint32_t xlen_ = 0, crc_ = 0;
    // the text: buffer tb_ holds have_ bytes from head_off_ on (have_ < 0 behind a seek into a block: bytes still to skip)
    int tb_ = 0;
    size_t head_off_ = FRONT;
    int64_t have_ = 0;
    uint32_t skip_ = 0;
    bool carry_moved_ = true, at_eof_ = false;
    std::deque<Blk> blks_;  // the blocks with text at hand
};

// ---- the host's backend: plain buffers, pread, the decoder's host lane ------------------------------------------------------
struct BgzfHostBackend : BgzfStreamBackend {
    std::vector<uint8_t> comp[2], txt[2];
    size_t got[2] = {0, 0};
    int threads;
    explicit BgzfHostBackend(int threads_ = 8) : threads(threads_) {}
    int open(size_t chunk_bytes, size_t text_cap_) override {
        for (int k = 0; k < 2; ++k) {
            comp[k].resize(FRONT + chunk_bytes);
            txt[k].resize(text_cap_);
        }
        return BSK_OK;
    }
    uint8_t* comp_host(int slot) override { return comp[slot].data(); }
    int start_read(int slot, int fd, uint64_t file_off, size_t len) override {
        size_t at = 0;
        while (at < len) {
            const ssize_t k = pread(fd, comp[slot].data() + FRONT + at, len - at, (off_t)(file_off + at));
            if (k < 0) { err = "libbsk: bgzf: reading the file failed"; return BSK_ERR_INVALID_ARG; }
            if (k == 0) break;
            at += (size_t)k;
        }
        got[slot] = at;
        return BSK_OK;
    }
    int wait_read(int slot, size_t* g) override { *g = got[slot]; return BSK_OK; }
    int push_front(int, size_t) override { return BSK_OK; }
    int inflate(int slot, size_t slot_bytes, const BgzfBlockDesc* d, size_t nb, int tbuf, uint64_t* bad) override {
        std::atomic<uint64_t> next{0}, worst{~0ull};
        const uint8_t* c = comp[slot].data();
        uint8_t* out = txt[tbuf].data();
        auto work = [&]() {
            std::unique_ptr<bgzf::BgzfLds> S(new bgzf::BgzfLds);
            memset(S->crc_mat, 0, sizeof S->crc_mat);  // (one chunk per block on the host: never applied)
            for (;;) {
                const uint64_t i = next.fetch_add(1);
                if (i >= nb) break;
                bgzf::HostLane io{c + d[i].coff, slot_bytes - d[i].coff, out + d[i].ooff};
                bgzf::Inflater<bgzf::HostLane> I(io, *S);
                const int e = I.run(12u + d[i].xlen, d[i].csize - 8u, d[i].usize, d[i].crc, 0);
                if (e != bgzf::OK) {
                    const uint64_t mine = i << 8 | (uint64_t)e;
                    uint64_t seen = worst.load();
                    while (mine < seen && !worst.compare_exchange_weak(seen, mine)) {}
                }
            }
        };
        const int T = (int)std::min<uint64_t>((uint64_t)std::max(1, std::min(threads, 64)), std::max<uint64_t>(nb / 8, 1));
        std::vector<std::thread> pool;
        for (int t = 1; t < T; ++t) pool.emplace_back(work);
        work();
        for (auto& t : pool) t.join();
        *bad = worst.load();
        return BSK_OK;
    }
    size_t text_cap(int tbuf) const override { return txt[tbuf].size(); }
    int text_grow(int tbuf, size_t cap, size_t) override { txt[tbuf].resize(cap); return BSK_OK; }
    const uint8_t* text(int tbuf) const override { return txt[tbuf].data(); }
    int reuse(int) override { return BSK_OK; }
    int move(int from, size_t from_off, int to, size_t to_off, size_t n) override {
        memcpy(txt[to].data() + to_off, txt[from].data() + from_off, n);
        return BSK_OK;
    }
    int find_cut(int tbuf, uint64_t n, uint64_t from, int format, uint64_t* cut) override {
        const uint8_t* t = txt[tbuf].data() + FRONT;
        *cut = format == BSK_FORMAT_FASTQ ? find_fastq_cut(t, n, from) : find_fasta_start(t, n, from);
        return BSK_OK;
    }
    int sync() override { return BSK_OK; }
};

// ---- the device's backend (ops_bgzf_stream.hip) -------------------------------------------------------------------------------
// a reader over the open file `fd` (the caller's: it is read with pread and not closed): device >= 0, or -1 for the host's
// backend.  0 for piece, look, chunk: 1 GiB, 1 MiB, 256 MiB.  Null and *rc, err on a failure
BgzfPieceReader* bgzf_reader_open(int fd, int device, int format, size_t piece, size_t look, size_t chunk, int* rc, std::string& err);
// stream_cut on text[0, n): by k_bgzf_stream_cut on `device`, or (device < 0) on the host
int bgzf_stream_cut_run(const uint8_t* text, uint64_t n, uint64_t from, int format, int device, uint64_t* cut, std::string& err);
// k_bgzf_stream_cut on d_text[0, n) in device memory, the answer to *d_cut; `stream` is a hipStream_t, returns a hipError_t (the
// gzip reader of gzip_stream.hpp cuts its pieces with the same kernel)
int bgzf_launch_stream_cut(const uint8_t* d_text, uint64_t n, uint64_t from, int format, uint64_t* d_cut, void* stream);

}  // namespace bsk
