// A plain gzip file of any size as record-aligned pieces of its text (PARITY.md GZIP "segments"):
// the file is never held whole, compressed or inflated.  This header is the definition -- what a segment is, where the next one
// starts, where a piece ends, what is checked on which pass -- written once over a small backend that holds the buffers and
// runs the steps of gzip_spec_dev.hpp on a segment.  GzipHostBackend (below) runs them with one host lane; the device's backend
// lives in ops_gzip_stream.hip.  Nothing here needs the HIP runtime: tests/host_c/gzip_stream_check.cpp builds this header alone
// under the host's sanitizers.
//
// A RESUME POINT is a bit position of the file at which a non-final dynamic block starts (a landing of the chain), or offset
// 0, with what a decoder needs to go on from there: the text offset, the 32 KiB of text in front, the number of the open
// member, the text offset at which it began, its CRC and length so far.  A SEGMENT is S compressed bytes from the resume point,
// in a buffer that begins at `base`, the multiple of 4096 at or in front of it; the buffer is cut into chunks and read by find /
// size / chain / decode / windows / translate / crc as a whole file is, chunk 0 starting at the resume bit.  The segment ends in front of the chain
// chunk that runs into the end of the buffer, or that would bring its text above 8 S; that chunk's start is the next resume
// point.  If chunk 0 itself does not land inside the buffer -- a stream of stored or fixed blocks, one very long block -- S
// doubles and the segment is read again, up to 32 times the S the reader was opened with: then BSK_ERR_CAPACITY.
//
// Positions are TEXT OFFSETS.  The pieces are a function of the text alone, not of the segment size, the chunk size or the
// backend.  For a piece that starts at text offset s:
//   1. the window is text[s, min(s + piece + lookahead, end));
//   2. the window reaches the end of the text: the piece is the rest;
//   3. else the piece ends at c = the record start that bsk_find_record_start names on the window from `piece`;
//   4. no start in the window: the lookahead doubles, and 1. to 3. are asked again;
//   5. the text behind c is the head of the next piece.
// next() is the sequential pass: it checks CRC32 and ISIZE of every member, at the call that decodes its trailer.  piece(lo, hi)
// re-enters at the last resume point it has recorded at or in front of lo (one per segment start), decodes forward, and checks
// the DEFLATE stream only; consecutive pieces are read on without re-entry.
#pragma once
#include <unistd.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/bsk.h"
#include "bgzf_stream.hpp"
#include "gzip_spec_dev.hpp"

namespace bsk {

struct GzipResume {
    uint64_t bit = 0;             // in the file; 0: the first member's header
    uint64_t text = 0;            // the text offset there
    uint64_t member = 0;          // the number of the open member
    int64_t open_at = 0;          // the text offset at which it began
    uint32_t crc = 0;             // its CRC32 and length so far (crc_known: the pass that came here has computed them)
    uint64_t len = 0;
    bool crc_known = true;
    std::vector<uint8_t> window;  // the gz::WIN bytes of text in front; empty: zeros (offset 0)
};

// ---- the backend: two slots of compressed bytes, the buffers of one segment, two text buffers ------------------------------------
struct GzipStreamBackend {
    std::string err;
    uint64_t held = 0, peak = 0;  // bytes in the backend's buffers now, and at most
    virtual ~GzipStreamBackend() {}
    // two slots of comp_cap bytes, two text buffers of text_cap, and the buffers of a segment of comp_cap bytes in chunks of
    // chunk_bytes that holds seg_text bytes of text: what a file of dynamic blocks needs is allocated here, once
    virtual int open(size_t comp_cap, size_t text_cap, size_t seg_text, size_t chunk_bytes) = 0;
    virtual int comp_grow(size_t cap) = 0;                                          // both slots hold at least cap bytes
    virtual int start_read(int slot, int fd, uint64_t file_off, size_t len) = 0;
    virtual int wait_read(int slot, size_t* got) = 0;
    // find and size on slot[0, n): chunks of chunk_bytes (0: the backend's choice; *chunk_used), chunk 0 from the member header at
    // byte 0 (rel_bit gz::NONE) or from the bit rel_bit; cand and res as gz::walk_chain takes them
    virtual int size(int slot, uint64_t n, uint64_t chunk_bytes, uint64_t rel_bit, std::vector<uint64_t>& cand, std::vector<gz::ChunkResult>& res,
                     uint64_t* chunk_used) = 0;
    // the chain chunks of that segment decoded to symbols: `total` of them; mem[0, ..): the members that end in the segment,
    // member0 the number of the first; window: the gz::WIN bytes in front of the segment (it stays valid until finish)
    virtual int decode(const std::vector<gz::ChainChunk>& chain, uint64_t member0, uint64_t total, const uint8_t* window, std::vector<gz::MemberRec>& mem,
                       std::vector<gz::ChunkResult>& dres) = 0;
    // windows, translate -- the segment's text lies in the backend's staging buffer --, the CRCs of `pieces` (null: none),
    // *bad: ~0 or the least chain index with a marker in front of its member; the last `tail` bytes of the text to tail_dst
    virtual int finish(const std::vector<gz::ChainChunk>& chain, uint64_t total, const std::vector<gz::Piece>* pieces, std::vector<uint32_t>& pcrc,
                       uint64_t* bad, uint32_t tail, uint8_t* tail_dst) = 0;
    virtual int take(uint64_t from, int tbuf, size_t off, size_t n) = 0;            // staging[from, from + n) to text(tbuf) + off
    virtual size_t text_cap(int tbuf) const = 0;
    virtual int text_grow(int tbuf, size_t cap, size_t keep) = 0;
    virtual const uint8_t* text(int tbuf) const = 0;
    virtual int reuse(int tbuf) = 0;                                                // what reads the buffer now is waited for before it is written
    virtual int move(int from, size_t from_off, int to, size_t to_off, size_t n) = 0;
    virtual int find_cut(int tbuf, uint64_t n, uint64_t from, int format, uint64_t* cut) = 0;  // on text(tbuf)[0, n) (n: none)
    virtual int sync() = 0;
    void holds(int64_t delta) {
        held = (uint64_t)((int64_t)held + delta);
        peak = std::max(peak, held);
    }
};

// ---- the reader -------------------------------------------------------------------------------------------------------------
class GzipPieceReader {
public:
    static constexpr uint64_t GROW_LIMIT = 32, TEXT_PER_SEGMENT = 8;
    GzipPieceReader(std::unique_ptr<GzipStreamBackend> backend, int fd, uint64_t file_size, int format, size_t piece, size_t look, size_t segment, size_t chunk)
        : B(std::move(backend)), fd_(fd), fsize_(file_size), format_(format), piece_(piece ? piece : (size_t)1 << 30), look_(look ? look : (size_t)1 << 20),
          chunk_(chunk) {
        seg0_ = std::max<uint64_t>(2048, segment ? segment : (size_t)64 << 20);
        seg_len_ = seg0_;
        text_per_seg_ = std::max<uint64_t>(TEXT_PER_SEGMENT * seg0_, 65536);
    }
    int open() {
        const uint64_t most_text = fsize_ < ((uint64_t)1 << 40) ? fsize_ * 1032 : ~0ull >> 2;
        const int rc = B->open((size_t)std::min<uint64_t>(seg0_ + 4096, std::max<uint64_t>(fsize_, 4096)),
                               (size_t)(std::min<uint64_t>((uint64_t)piece_ + look_, most_text) + std::min(text_per_seg_, most_text) + 4096),
                               (size_t)std::min(text_per_seg_, most_text), chunk_);
        if (rc != BSK_OK) return fail(rc, B->err);
        reenter(0, true);
        return BSK_OK;
    }
    const std::string& error() const { return err_; }

    // the next piece by the rule; *last: the text ends with it (further calls give empty last pieces)
    int next(const void** ptr, size_t* n, uint64_t* text_lo, uint64_t* text_hi, int* last) {
        if (failed_ != BSK_OK) return failed_;
        if (!checking_) reenter(pos_, true);  // (pieces were asked for in between: the members' CRCs are taken up where they are known)
        int rc = begin_piece();
        if (rc != BSK_OK) return rc;
        uint64_t look = look_, cut = 0;
        for (;;) {
            const uint64_t need = (uint64_t)piece_ + look;
            while (!eof_ && have_ <= need)
                if ((rc = more_text(true)) != BSK_OK) return rc;
            if (have_ <= need) { cut = have_; break; }
            rc = B->find_cut(tb_, need, piece_, format_, &cut);
            if (rc != BSK_OK) return fail(rc, B->err);
            if (cut < need) break;
            look *= 2;
        }
        return end_piece(cut, ptr, n, text_lo, text_hi, last);
    }

    // the bytes [text_lo, text_hi) again
    int piece(uint64_t text_lo, uint64_t text_hi, const void** ptr, size_t* n) {
        if (text_hi < text_lo) return fail(BSK_ERR_INVALID_ARG, "libbsk: gzip: bad text offsets of a piece");
        if (failed_ != BSK_OK || pos_ != text_lo) reenter(text_lo, false);
        int rc = begin_piece();
        if (rc != BSK_OK) return rc;
        const uint64_t want = text_hi - text_lo;
        while (!eof_ && have_ < want)
            if ((rc = more_text(false)) != BSK_OK) return rc;
        if (have_ < want) return fail(BSK_ERR_INVALID_ARG, "libbsk: gzip: the end of the piece lies behind the end of the file's text");
        uint64_t lo = 0, hi = 0;
        int last = 0;
        return end_piece(want, ptr, n, &lo, &hi, &last);
    }

    // segments decoded, access points, buffer doublings, chain chunks dropped, members, text bytes so far, peak bytes of the
    // backend's buffers, chunk size used
    void info(uint64_t out[8]) const {
        out[0] = segments_; out[1] = points_.size(); out[2] = doublings_; out[3] = dropped_;
        out[4] = members_seen_; out[5] = text_seen_; out[6] = B->peak; out[7] = chunk_used_;
    }

private:
    int fail(int rc, const std::string& m) { err_ = m; failed_ = rc; return rc; }
    static int fail_code(int f) { return f == gz::FAIL_UNSUPPORTED ? BSK_ERR_UNSUPPORTED : BSK_ERR_FORMAT; }

    // the decoder goes back to the last recorded resume point at or in front of `lo`; the text in front of lo is dropped as it comes
    void reenter(uint64_t lo, bool with_crc) {
        GzipResume at;  // (offset 0: always known)
        for (auto it = points_.begin(); it != points_.end() && it->first <= lo; ++it)
            if (!with_crc || it->second.crc_known) at = it->second;
        cur_ = at;
        failed_ = BSK_OK;
        eof_ = fsize_ == 0;
        checking_ = with_crc;
        have_ = 0;
        pos_ = lo;
    }

    // the other text buffer becomes the current one, the carried head at its front
    int begin_piece() {
        const int to = tb_ ^ 1;
        int rc = B->reuse(to);
        if (rc == BSK_OK && B->text_cap(to) < have_ + 16) rc = B->text_grow(to, (size_t)have_ + 16, 0);
        if (rc == BSK_OK && have_) rc = B->move(tb_, head_off_, to, 0, (size_t)have_);
        if (rc != BSK_OK) return fail(rc, B->err);
        tb_ = to;
        head_off_ = 0;
        return BSK_OK;
    }
    int end_piece(uint64_t cut, const void** ptr, size_t* n, uint64_t* lo, uint64_t* hi, int* last) {
        const int rc = B->sync();
        if (rc != BSK_OK) return fail(rc, B->err);
        *ptr = B->text(tb_);
        *n = (size_t)cut;
        *lo = pos_;
        pos_ += cut;
        have_ -= cut;
        head_off_ = (size_t)cut;
        *hi = pos_;
        *last = eof_ && have_ == 0;
        return BSK_OK;
    }

    // the bytes [off, off + len) of the file in a slot: the one that was read ahead, or read now
    int fetch(uint64_t off, size_t len) {
        const int ns = slot_ ^ 1;
        size_t got = 0;
        int rc = BSK_OK;
        bool have = false;
        if (pending_) {
            rc = B->wait_read(ns, &got);
            pending_ = false;
            if (rc != BSK_OK) return fail(rc, B->err);
            have = pend_off_ == off && pend_len_ == len;
        }
        if (!have) {
            if ((rc = B->comp_grow((size_t)std::min<uint64_t>(seg_len_ + 4096, std::max<uint64_t>(fsize_, 4096)))) != BSK_OK || (rc = B->start_read(ns, fd_, off, len)) != BSK_OK || (rc = B->wait_read(ns, &got)) != BSK_OK) return fail(rc, B->err);
        }
        if (got != len) return fail(BSK_ERR_INVALID_ARG, "libbsk: gzip: the file became shorter while it was read");
        slot_ = ns;
        return BSK_OK;
    }

    // one more segment is decoded from cur_, its text behind the text at hand
    int more_text(bool verify) {
        if (!verify) checking_ = false;
        {
            auto it = points_.find(cur_.text);
            if (it == points_.end() || (!it->second.crc_known && checking_)) {
                GzipResume& p = points_[cur_.text];
                p = cur_;
                p.crc_known = checking_;
            }
        }
        std::vector<uint64_t> cand;
        std::vector<gz::ChunkResult> res;
        std::vector<gz::ChainChunk> chain;
        gz::SegmentEnds se;
        gz::Plan plan;
        uint64_t base = 0, n = 0;
        for (;;) {
            base = (cur_.bit >> 3) & ~4095ull;
            n = std::min<uint64_t>((cur_.bit >> 3) - base + seg_len_, fsize_ - base);
            int rc = fetch(base, (size_t)n);
            if (rc != BSK_OK) return rc;
            rc = B->size(slot_, n, chunk_, cur_.bit ? cur_.bit - base * 8u : gz::NONE, cand, res, &chunk_used_);
            if (rc != BSK_OK) return fail(rc, B->err);
            se = gz::SegmentEnds();
            se.open_at = cur_.open_at - (int64_t)cur_.text;
            se.members = cur_.member;
            se.file_off = base;
            se.more = base + n < fsize_;
            se.text_cap = text_per_seg_;
            chain.clear();
            std::string e;
            const int f = gz::walk_chain(cand, res, chunk_used_, chain, plan, e, &se);
            if (f) return fail(fail_code(f), e);
            if (!se.grow) break;
            if (seg_len_ >= GROW_LIMIT * seg0_)
                return fail(BSK_ERR_CAPACITY, "libbsk: gzip: no non-final dynamic block ends inside the " + std::to_string(n) + " bytes of the file from offset " + std::to_string(base) +
                                                  " (a stream of stored or fixed blocks, or one very long block): the reader's segment of " + std::to_string(seg0_) +
                                                  " bytes has doubled up to its limit of " + std::to_string(GROW_LIMIT * seg0_) + " bytes; open it with a larger segment (BSK_GZIP_SEGMENT_BYTES), or read the file whole");
            seg_len_ *= 2;
            ++doublings_;
        }
        uint64_t total = 0, next_bit = 0;
        for (const gz::ChainChunk& c : chain) total += c.text;
        const uint64_t nmem = plan.members - cur_.member;
        if (se.next != gz::NONE) {  // segment k + 1 is read, and crosses to the device, under the decode of segment k
            next_bit = base * 8u + cand[se.next];
            pend_off_ = (next_bit >> 3) & ~4095ull;
            pend_len_ = (size_t)std::min<uint64_t>((next_bit >> 3) - pend_off_ + seg_len_, fsize_ - pend_off_);  // (at most seg_len_ + 4095: the slots hold it)
            int rc = B->start_read(slot_ ^ 1, fd_, pend_off_, pend_len_);
            if (rc != BSK_OK) return fail(rc, B->err);
            pending_ = true;
            for (uint64_t k = 1; k < se.next; ++k) dropped_ += cand[k] != gz::NONE;
            dropped_ -= chain.size() - 1;
        } else {
            dropped_ += plan.off_chain;
        }
        static const std::vector<uint8_t> zeros(gz::WIN, 0);
        const uint8_t* window = cur_.window.empty() ? zeros.data() : cur_.window.data();
        std::vector<gz::MemberRec> mem(nmem + 1);
        std::vector<gz::ChunkResult> dres;
        int rc = B->decode(chain, cur_.member, total, window, mem, dres);
        if (rc != BSK_OK) return fail(rc, B->err);
        for (size_t i = 0; i < chain.size(); ++i) {
            const gz::ChainChunk& c = chain[i];
            std::string e;
            if (dres[i].err) return fail(fail_code(gz::chunk_failure(dres[i], c.member0, e, base)), e);
            if (dres[i].members != c.members || dres[i].text != c.text) return fail(BSK_ERR_FORMAT, "libbsk: gzip: the decode of chunk " + std::to_string(c.k) + " at offset " + std::to_string(base) + " does not repeat its size pass");
            for (uint32_t m = 0; m < c.members; ++m) mem[c.member0 - cur_.member + m].text_end += c.text_off;
        }
        mem[nmem] = gz::MemberRec{0, total, 0, 0};  // (the member that is open at the segment's end)
        std::vector<gz::Piece> pieces;
        std::vector<uint32_t> pcrc;
        if (checking_) gz::crc_pieces(mem, pieces);
        uint64_t bad = gz::NONE;
        const uint32_t tail = (uint32_t)std::min<uint64_t>(total, gz::WIN);
        std::vector<uint8_t> tailbuf(gz::WIN);
        rc = B->finish(chain, total, checking_ ? &pieces : nullptr, pcrc, &bad, tail, tailbuf.data());
        if (rc != BSK_OK) return fail(rc, B->err);
        if (bad != gz::NONE) {
            const gz::ChainChunk& c = chain[(size_t)bad];
            return fail(BSK_ERR_FORMAT, gz::where(c.member0, base + cand[c.k] / 8u) + gz::error_text(bgzf::ERR_DISTANCE) + " (in chunk " + std::to_string(c.k) + " of the segment at offset " + std::to_string(base) + ")");
        }
        gz::OpenMember om{cur_.member, base, cur_.crc, cur_.len};
        if (checking_) {
            std::string e;
            const int f = gz::check_members(mem, pieces, pcrc, e, &om);
            if (f) return fail(fail_code(f), e);
        }
        // the text of the segment that lies behind the text at hand
        const uint64_t from = pos_ + have_ - cur_.text;
        if (from < total) {
            const uint64_t take = total - from, room = head_off_ + have_ + take + 16;
            if (room > B->text_cap(tb_)) {
                rc = B->text_grow(tb_, (size_t)std::max<uint64_t>(room, 2 * (uint64_t)B->text_cap(tb_)), head_off_ + (size_t)have_);
                if (rc != BSK_OK) return fail(rc, B->err);
            }
            rc = B->take(from, tb_, head_off_ + (size_t)have_, (size_t)take);
            if (rc != BSK_OK) return fail(rc, B->err);
            have_ += take;
        }
        // where the next segment starts
        std::vector<uint8_t> w(gz::WIN);
        memcpy(w.data(), window + tail, gz::WIN - tail);
        memcpy(w.data() + (gz::WIN - tail), tailbuf.data(), tail);
        cur_.window.swap(w);
        cur_.open_at = (int64_t)cur_.text + se.open_at;
        cur_.text += total;
        cur_.member = plan.members;
        cur_.crc = om.crc;
        cur_.len = om.len;
        cur_.crc_known = checking_;
        cur_.bit = next_bit;
        ++segments_;
        members_seen_ = std::max(members_seen_, plan.members);
        text_seen_ = std::max(text_seen_, cur_.text);
        if (se.next == gz::NONE) eof_ = true;
        return BSK_OK;
    }

    std::unique_ptr<GzipStreamBackend> B;
    int fd_;
    uint64_t fsize_;
    int format_;
    size_t piece_, look_, chunk_;
    uint64_t seg0_ = 0, seg_len_ = 0, text_per_seg_ = 0;
    std::string err_;
    int failed_ = BSK_OK;
    GzipResume cur_;                          // where the next segment starts
    std::map<uint64_t, GzipResume> points_;   // the access points: one per segment start, by text offset
    bool eof_ = false, checking_ = true;
    int slot_ = 0;
    bool pending_ = false;                    // slot_ ^ 1 is being read: the file's bytes [pend_off_, pend_off_ + pend_len_)
    uint64_t pend_off_ = 0;
    size_t pend_len_ = 0;
    // the text: buffer tb_ holds have_ bytes from head_off_ on, the first of them at text offset pos_
    int tb_ = 0;
    size_t head_off_ = 0;
    uint64_t have_ = 0, pos_ = 0;
    uint64_t segments_ = 0, doublings_ = 0, dropped_ = 0, members_seen_ = 0, text_seen_ = 0, chunk_used_ = 0;
};

// ---- the host's backend: plain buffers, pread, the method's host lane ----------------------------------------------------------
struct GzipHostBackend : GzipStreamBackend {
    std::vector<uint8_t> comp[2], txt[2], stage, W;
    std::vector<uint16_t> sym;
    size_t got[2] = {0, 0};
    std::unique_ptr<gz::GzDecodeLds> lds{new gz::GzDecodeLds};
    // the segment at hand
    int slot = 0;
    uint64_t n = 0;
    bool resumed = false;
    gz::Geometry G{};
    std::vector<uint64_t> cands;
    const uint8_t* window = nullptr;

    template <class V> void resize(V& v, size_t k) {
        holds((int64_t)(k * sizeof(v[0])) - (int64_t)(v.size() * sizeof(v[0])));
        v.resize(k);
    }
    template <class V> void at_least(V& v, size_t k) { if (v.size() < k) resize(v, k); }
    static uint64_t chunk_of(uint64_t chunk_bytes, uint64_t n) { return std::max<uint64_t>(chunk_bytes ? chunk_bytes : n / 16, 1024); }
    int open(size_t comp_cap, size_t text_cap_, size_t seg_text, size_t chunk_bytes) override {
        for (int k = 0; k < 2; ++k) {
            resize(comp[k], comp_cap);
            resize(txt[k], text_cap_);
        }
        resize(sym, seg_text + 8);
        resize(stage, seg_text + 1);
        resize(W, (size_t)gz::geometry(comp_cap, chunk_of(chunk_bytes, comp_cap), nullptr).nchunks * gz::WIN);
        return BSK_OK;
    }
    int comp_grow(size_t cap) override {
        for (int k = 0; k < 2; ++k) at_least(comp[k], cap);
        return BSK_OK;
    }
    int start_read(int s, int fd, uint64_t file_off, size_t len) override {
        size_t at = 0;
        while (at < len) {
            const ssize_t k = pread(fd, comp[s].data() + at, len - at, (off_t)(file_off + at));
            if (k < 0) { err = "libbsk: gzip: reading the file failed"; return BSK_ERR_INVALID_ARG; }
            if (k == 0) break;
            at += (size_t)k;
        }
        got[s] = at;
        return BSK_OK;
    }
    int wait_read(int s, size_t* g) override { *g = got[s]; return BSK_OK; }
    template <bool EMIT, bool RESUME>
    gz::ChunkResult walk(const gz::Parked& park, uint32_t shift) {
        gz::HostLane io{comp[slot].data(), n};
        lds->T.park = park;
        gz::Walker<gz::HostLane, EMIT, RESUME> Wk(io, lds->T, EMIT ? lds->ring : nullptr);
        return Wk.run(shift);
    }
    int size(int slot_, uint64_t n_, uint64_t chunk_bytes, uint64_t rel_bit, std::vector<uint64_t>& cand, std::vector<gz::ChunkResult>& res, uint64_t* chunk_used) override {
        slot = slot_;
        n = n_;
        resumed = rel_bit != gz::NONE;
        G = gz::geometry(n, chunk_of(chunk_bytes, n), nullptr);
        *chunk_used = G.chunk_bytes;
        cands.assign(G.nchunks, gz::NONE);
        for (uint64_t k = 1; k < G.nchunks; ++k) {
            cands[k] = gz::find_host(comp[slot].data(), n, G.chunk_bytes, k);
            if (resumed && cands[k] <= rel_bit) cands[k] = gz::NONE;  // (chunk 0 starts at the resume bit: nothing in front of it is a start)
        }
        if (resumed) cands[0] = rel_bit;
        G.cand = cands.data();
        res.assign(G.nchunks, gz::ChunkResult{gz::NONE, 0, gz::NONE, 0, 0, 0});
        for (uint64_t k = 0; k < G.nchunks; ++k) {
            if (k && cands[k] == gz::NONE) continue;
            const gz::Parked park{G, k, 0, (k || resumed) ? gz::NONE : 0, nullptr, nullptr, 0};
            res[k] = resumed ? walk<false, true>(park, 0) : walk<false, false>(park, 0);
        }
        cand = cands;
        return BSK_OK;
    }
    int decode(const std::vector<gz::ChainChunk>& chain, uint64_t member0, uint64_t total, const uint8_t* window_, std::vector<gz::MemberRec>& mem,
               std::vector<gz::ChunkResult>& dres) override {
        window = window_;
        at_least(sym, (size_t)total + 8);
        dres.clear();
        for (const gz::ChainChunk& c : chain) {
            const gz::Parked park{G, c.k, c.text, (c.k || resumed) ? gz::NONE : 0, mem.data() + (c.member0 - member0), sym.data() + c.text_off, c.members};
            const uint32_t shift = (uint32_t)(c.text_off & 7u);
            dres.push_back(resumed ? walk<true, true>(park, shift) : walk<true, false>(park, shift));
        }
        return BSK_OK;
    }
    int finish(const std::vector<gz::ChainChunk>& chain, uint64_t total, const std::vector<gz::Piece>* pieces, std::vector<uint32_t>& pcrc, uint64_t* bad,
               uint32_t tail, uint8_t* tail_dst) override {
        at_least(W, chain.size() * (size_t)gz::WIN);
        at_least(stage, (size_t)total + 1);
        gz::windows_host(chain, sym.data(), W.data(), window);
        *bad = gz::NONE;
        for (size_t j = 0; j < chain.size() && *bad == gz::NONE; ++j) {
            const gz::ChainChunk& c = chain[j];
            for (uint64_t q = c.text_off; q < c.text_off + c.text; ++q) {
                const uint16_t s = sym[q];
                if (s < 0x8000u) { stage[q] = (uint8_t)s; continue; }
                if ((s & 0x7FFFu) < c.marker_lo) { *bad = j; break; }
                stage[q] = W[j * (size_t)gz::WIN + (s & 0x7FFFu)];
            }
        }
        if (*bad != gz::NONE) return BSK_OK;
        if (pieces) {
            uint32_t tab[256];
            for (uint32_t i = 0; i < 256; ++i) tab[i] = bgzf::crc_table_entry(i);
            pcrc.resize(pieces->size());
            for (size_t i = 0; i < pieces->size(); ++i) {
                uint32_t c = 0xFFFFFFFFu;
                for (uint32_t q = 0; q < (*pieces)[i].len; ++q) c = tab[(c ^ stage[(*pieces)[i].off + q]) & 255u] ^ (c >> 8);
                pcrc[i] = ~c;
            }
        }
        if (tail) memcpy(tail_dst, stage.data() + (total - tail), tail);
        return BSK_OK;
    }
    int take(uint64_t from, int tbuf, size_t off, size_t k) override {
        memcpy(txt[tbuf].data() + off, stage.data() + from, k);
        return BSK_OK;
    }
    size_t text_cap(int tbuf) const override { return txt[tbuf].size(); }
    int text_grow(int tbuf, size_t cap, size_t) override { resize(txt[tbuf], cap); return BSK_OK; }
    const uint8_t* text(int tbuf) const override { return txt[tbuf].data(); }
    int reuse(int) override { return BSK_OK; }
    int move(int from, size_t from_off, int to, size_t to_off, size_t k) override {
        memmove(txt[to].data() + to_off, txt[from].data() + from_off, k);
        return BSK_OK;
    }
    int find_cut(int tbuf, uint64_t k, uint64_t from, int format, uint64_t* cut) override {
        const uint8_t* t = txt[tbuf].data();
        *cut = format == BSK_FORMAT_FASTQ ? find_fastq_cut(t, k, from) : find_fasta_start(t, k, from);
        return BSK_OK;
    }
    int sync() override { return BSK_OK; }
};

// ---- the device's backend (ops_gzip_stream.hip) -------------------------------------------------------------------------------
// a reader over the open file `fd` (the caller's: it is read with pread and not closed): device >= 0, or -1 for the host's
// backend.  0 for piece, look, segment: 1 GiB, 1 MiB, 64 MiB; chunk 0: the rule of gzip_inflate_device applied to a segment (on
// the host: a sixteenth of it).  Null and *rc, err on a failure
GzipPieceReader* gzip_reader_open(int fd, int device, int format, size_t piece, size_t look, size_t segment, size_t chunk, int* rc, std::string& err);

}  // namespace bsk
