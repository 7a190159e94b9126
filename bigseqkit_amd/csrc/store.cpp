// ============================================================================
// store.cpp -- FileStore / StoreFASTXN behind the C ABI, and the pipelined host path of the record operators.
//
// Reference: NewFileStore (/root/reference/bigseqkit-lib/helper.go:378-460) writes the elements of every partition,
// joined by '\n', into ONE file in partition order -- an MPI token travels from executor to executor so that partition
// k + 1 starts where k ended; StoreFASTXN (bigseqkit/helper.go:193-195) is SaveAsTextFile: one file per partition.
// Here the order comes from a scan of sizes instead of a token: a part that arrives before its predecessors is kept
// in host memory until they are written (single file), or simply owns its file (directory of parts).
//
// bsk_run_to_store is the file -> file path for a partition that sits in HOST memory (a file read into a pinned
// buffer): record-aligned chunks of 256 MiB go through two device buffers,
//     H2D(chunk i+1)  ||  kernels(chunk i)  ||  D2H(output of chunk i-1) + write,
// on three streams, so that the PCIe copies in both directions hide behind each other and behind the kernels
// (north_star: "async hipMemcpy double-buffers host file reads against kernel execution").  Operators whose result
// depends on the whole partition (rmdup, sort, rename, range, grep -C / --delete-matched) run on the whole shard and
// only their output is drained in chunks.
//
// The drain (round 3).  What one file takes was measured before anything was built (scripts/experiments/write_rates.cpp,
// profiles/r03_write_rates.txt, the GPU box's 256-thread host): ONE file accepts 6.0 GB/s in /dev/shm and 10.6 GB/s under
// /tmp whatever the number of writer threads -- a buffered write holds the inode lock for the whole copy (2 .. 16 threads on
// disjoint pieces of one file: 5.1 .. 3.6 GB/s) -- a shared mapping filled by 1 .. 16 threads 3.5 .. 3.9 GB/s (page faults
// of one address space), a preallocated file 7.6 / 12.2 GB/s; a file PER THREAD scales: 35 GB/s with 8, 108 GB/s with 32.
// So the drain of one part stays one stream of pwrite()s (three pinned buffers: two D2H copies in flight behind the piece
// being written, no lock held while writing), and the way to more than ~10 GB/s is the reference's own default layout, a
// directory of part files (StoreFASTXN) written by several contexts at once: scripts/bench_file_to_file.py --parts.
// ============================================================================
#include <fcntl.h>
#include <hip/hip_runtime_api.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <cstring>
#include <functional>
#include <future>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/bsk.h"
#include "anchor.hpp"
#include "ctx.hpp"
#include "ops_host.hpp"
#include "ops_host_internal.hpp"
#include "ops_bgzf_write.hpp"
#include "ops_segcopy.hpp"

using namespace bsk;

struct bsk_store {
    std::string path;
    bool merge = true;
    int fd = -1;               // single file
    std::mutex mu;
    uint64_t next = 0;         // the part whose bytes go to the file directly
    uint64_t offset = 0;       // end of what has been written
    struct Pending { std::vector<uint8_t> bytes; bool done = false; int fd = -1; uint64_t off = 0; };
    std::map<uint64_t, Pending> parts;  // parts that are not `next` yet (single file) / open part files (directory)
    uint64_t total = 0;
    std::string err;
    bool bgzf = false;         // bsk_store_set_bgzf: what is put is text, what is written is BGZF (every put piece whole blocks)
    bool bgzf_eof = true;      // ... and a file ends with the EOF block (off: the file is a piece of one, bsk_store_set_bgzf(s, 2))
    bool touched = false;      // something was put: the mode stays
};

namespace {

int store_fail(bsk_store* s, const std::string& m) {
    if (s) s->err = m;
    return BSK_ERR_INVALID_ARG;
}

// the file of a part in directory mode
std::string part_name(const bsk_store* s, uint64_t part) {
    char nm[64];
    snprintf(nm, sizeof nm, s->bgzf ? "/part%05llu.gz" : "/part%05llu", (unsigned long long)part);
    return s->path + nm;
}

bool write_all(int fd, const uint8_t* p, size_t n, uint64_t at) {
    while (n) {
        const ssize_t w = pwrite(fd, p, n, (off_t)at);
        if (w < 0) { if (errno == EINTR) continue; return false; }
        p += w; n -= (size_t)w; at += (uint64_t)w;
    }
    return true;
}

// a part file is complete: in BGZF mode the EOF block ends it
bool end_part_file(bsk_store* s, int fd, uint64_t off) {
    if (!s->bgzf || !s->bgzf_eof) return true;
    uint8_t e[28];
    bgzf_eof_block(e);
    s->total += sizeof e;
    return write_all(fd, e, sizeof e, off);
}

// bytes of part `part`; last: the part is complete
int store_append(bsk_store* s, uint64_t part, const uint8_t* data, size_t n, bool last) {
    std::lock_guard<std::mutex> g(s->mu);
    if (!s->merge) {  // a file per partition (SaveAsTextFile)
        auto& P = s->parts[part];
        if (P.fd < 0) {
            const std::string nm = part_name(s, part);
            P.fd = open(nm.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0644);
            if (P.fd < 0) return store_fail(s, "libbsk: cannot create " + nm + ": " + strerror(errno));
            P.bytes.clear();
            P.off = 0;
        }
        if (!write_all(P.fd, data, n, P.off)) return store_fail(s, "libbsk: write failed: " + std::string(strerror(errno)));
        P.off += n;
        s->total += n;
        if (last) {
            if (!end_part_file(s, P.fd, P.off)) return store_fail(s, "libbsk: write failed: " + std::string(strerror(errno)));
            close(P.fd);
            s->parts.erase(part);
        }
        return BSK_OK;
    }
    if (part < s->next) return store_fail(s, "libbsk: part " + std::to_string(part) + " was already completed");
    if (part != s->next) {  // not its turn: keep the bytes
        auto& P = s->parts[part];
        P.bytes.insert(P.bytes.end(), data, data + n);
        if (last) P.done = true;
        return BSK_OK;
    }
    if (!write_all(s->fd, data, n, s->offset)) return store_fail(s, "libbsk: write failed: " + std::string(strerror(errno)));
    s->offset += n;
    s->total += n;
    if (!last) return BSK_OK;
    // the next parts that are already here
    for (;;) {
        ++s->next;
        auto it = s->parts.find(s->next);
        if (it == s->parts.end()) break;
        auto& P = it->second;
        if (!P.bytes.empty()) {
            if (!write_all(s->fd, P.bytes.data(), P.bytes.size(), s->offset)) return store_fail(s, "libbsk: write failed: " + std::string(strerror(errno)));
            s->offset += P.bytes.size();
            s->total += P.bytes.size();
        }
        const bool done = P.done;
        s->parts.erase(it);
        if (!done) break;  // that part is still being produced: it now writes directly
    }
    return BSK_OK;
}

// Pinned staging of the drain, per context (allocated by the thread that owns the context, before any writer thread runs)
constexpr size_t DRAIN_PIECE = (size_t)32 << 20;
constexpr int DRAIN_NBUF = 3;
struct Drainer {
    uint8_t* pin[DRAIN_NBUF] = {nullptr, nullptr, nullptr};
    hipEvent_t ev[DRAIN_NBUF] = {nullptr, nullptr, nullptr};
    uint8_t* dev[DRAIN_NBUF] = {nullptr, nullptr, nullptr};  // round 6: a result that is a list of slices is gathered piece by piece into these
};

int drainer_prepare(bsk_ctx* c) {
    if (c->drainer) return BSK_OK;
    Drainer* d = new Drainer;
    for (int b = 0; b < DRAIN_NBUF; ++b) {
        if (hipHostMalloc((void**)&d->pin[b], DRAIN_PIECE, hipHostMallocDefault) != hipSuccess ||
            hipEventCreateWithFlags(&d->ev[b], hipEventDisableTiming) != hipSuccess) {
            for (int k = 0; k <= b; ++k) { if (d->pin[k]) hipHostFree(d->pin[k]); if (d->ev[k]) hipEventDestroy(d->ev[k]); }
            delete d;
            c->set_error("libbsk: pinned staging buffers of the output drain could not be allocated");
            return BSK_ERR_HIP;
        }
    }
    c->drainer = d;
    return BSK_OK;
}

// where the next n bytes of `part` go.  direct: fd + file offset reserved (the part's turn, or its own file);
// else the bytes are kept in host memory until the part's turn (store_append)
struct Target { bool direct = false; int fd = -1; uint64_t base = 0; };
int reserve_target(bsk_store* s, uint64_t part, size_t n, Target* t) {
    std::lock_guard<std::mutex> g(s->mu);
    if (!s->merge) {
        auto& P = s->parts[part];
        if (P.fd < 0) {
            const std::string nm = part_name(s, part);
            P.fd = open(nm.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0644);
            if (P.fd < 0) return store_fail(s, "libbsk: cannot create " + nm + ": " + strerror(errno));
            P.off = 0;
        }
        t->direct = true; t->fd = P.fd; t->base = P.off;
        P.off += n;
        s->total += n;
        return BSK_OK;
    }
    if (part < s->next) return store_fail(s, "libbsk: part " + std::to_string(part) + " was already completed");
    if (part != s->next) { t->direct = false; return BSK_OK; }
    t->direct = true; t->fd = s->fd; t->base = s->offset;
    s->offset += n;
    s->total += n;
    return BSK_OK;
}

// the part is complete: the next parts that are already here follow (single file) / the part file is closed (directory)
int finish_part(bsk_store* s, uint64_t part) {
    std::lock_guard<std::mutex> g(s->mu);
    if (!s->merge) {
        auto it = s->parts.find(part);
        if (it != s->parts.end()) {
            if (it->second.fd >= 0) {
                if (!end_part_file(s, it->second.fd, it->second.off)) return store_fail(s, "libbsk: write failed: " + std::string(strerror(errno)));
                close(it->second.fd);
            }
            s->parts.erase(it);
        }
        return BSK_OK;
    }
    if (part != s->next) return BSK_OK;  // (kept in memory: store_append marked it done)
    for (;;) {
        ++s->next;
        auto it = s->parts.find(s->next);
        if (it == s->parts.end()) break;
        auto& P = it->second;
        if (!P.bytes.empty()) {
            if (!write_all(s->fd, P.bytes.data(), P.bytes.size(), s->offset)) return store_fail(s, "libbsk: write failed: " + std::string(strerror(errno)));
            s->offset += P.bytes.size();
            s->total += P.bytes.size();
        }
        const bool done = P.done;
        s->parts.erase(it);
        if (!done) break;  // that part is still being produced: it now writes directly
    }
    return BSK_OK;
}

}  // namespace

namespace bsk {
// The text of a result -- n bytes at d, or the list of slices `seg` (d null) -- as BGZF, in bounded pieces: a piece is
// BGZF_PIECE bytes of text (whole blocks, so a piece boundary is a block boundary), gathered if need be, compressed on the
// context's device without an EOF block and handed to sink(d_comp, n_comp) before the next one is made.
int bgzf_pieces(bsk_ctx* c, const uint8_t* d, const bsk_ctx::PendingOut* seg, size_t n, std::string* err,
                const std::function<int(const void*, size_t)>& sink) {
    // whole blocks of text AND whole tiles of the gather (launch_seg_copy_range starts a piece on a tile): 65 280 = 2^8 * 255
    // and 4 096 meet every 1 044 480 bytes; 64 of those are 64 MiB less 256 KiB
    constexpr uint64_t BGZF_UNIT = 1044480, BGZF_PIECE_DEFAULT = 64 * BGZF_UNIT;
    static_assert(BGZF_UNIT % SEG_TILE == 0 && BGZF_UNIT % 65280 == 0, "a piece boundary is a block boundary and a tile boundary");
    // BSK_BGZF_PIECE_BYTES moves the line (tests: a result of a few MB in several pieces); rounded up to the unit
    uint64_t BGZF_PIECE = BGZF_PIECE_DEFAULT;
    if (const char* e = getenv("BSK_BGZF_PIECE_BYTES")) BGZF_PIECE = std::max<uint64_t>(1, (strtoull(e, nullptr, 10) + BGZF_UNIT - 1) / BGZF_UNIT) * BGZF_UNIT;
    uint8_t* d_piece = nullptr;
    if (seg && hipMalloc((void**)&d_piece, (size_t)std::min<uint64_t>(BGZF_PIECE, ((uint64_t)n + 4095) & ~4095ull)) != hipSuccess) {
        *err = "libbsk: bgzf: no device memory for a piece of the result";
        return BSK_ERR_HIP;
    }
    int rc = BSK_OK;
    for (uint64_t at = 0; at < n && rc == BSK_OK; at += BGZF_PIECE) {
        const uint64_t to = std::min<uint64_t>(n, at + BGZF_PIECE);
        const uint8_t* from = d ? d + at : d_piece;
        if (seg) {
            hipError_t e = launch_seg_copy_range(seg->seg_src, seg->seg_off, seg->nseg, seg->first4k, d_piece, at, to, seg->total, seg->lo, seg->hi, nullptr);
            if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
            if (e != hipSuccess) { *err = std::string("libbsk: gathering the slices of the result failed: ") + hipGetErrorString(e); rc = BSK_ERR_HIP; break; }
        }
        void* d_comp = nullptr;
        size_t n_comp = 0;
        rc = bgzf_deflate_device(from, (size_t)(to - at), c->device, 0, false, &d_comp, &n_comp, *err);
        if (rc == BSK_OK) rc = sink(d_comp, n_comp);
        if (d_comp) hipFree(d_comp);
    }
    if (d_piece) hipFree(d_piece);
    return rc;
}
}  // namespace bsk

namespace {

// device bytes -> store.  Returns a status and, on failure, the message in *err (the caller owns the context's error
// text: this function also runs on the writer thread of bsk_run_to_store, next to the thread that computes).
int drain_to_store(bsk_ctx* c, bsk_store* s, uint64_t part, const uint8_t* d, size_t n, bool last, hipStream_t d2h, std::string* err,
                   const bsk_ctx::PendingOut* seg = nullptr /* the n bytes are this list of slices (d is null) */) {
    auto hipfail = [&](hipError_t e, const char* what) { *err = std::string(what) + ": " + hipGetErrorString(e); return BSK_ERR_HIP; };
#define DR_TRY(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) return hipfail(e__, #expr); } while (0)
    DR_TRY(hipSetDevice(c->device));
    Drainer* D = (Drainer*)c->drainer;
    if (!D) { *err = "libbsk: drain without staging buffers"; return BSK_ERR_INVALID_ARG; }
    int rc = BSK_OK;
    if (n && s->bgzf) {
        // the text is compressed on the device in front of the D2H copy, piece by piece, and appended as the bytes of a part are
        std::vector<uint8_t> host;
        rc = bgzf_pieces(c, d, seg, n, err, [&](const void* d_comp, size_t n_comp) {
            host.resize(n_comp);
            if (n_comp && hipMemcpy(host.data(), d_comp, n_comp, hipMemcpyDeviceToHost) != hipSuccess) { *err = "libbsk: bgzf: the D2H copy of a compressed piece failed"; return BSK_ERR_HIP; }
            const int r = store_append(s, part, host.data(), n_comp, false);
            if (r != BSK_OK) *err = s->err;
            return r;
        });
        if (rc != BSK_OK) return rc;
    } else if (n) {
        Target t;
        rc = reserve_target(s, part, n, &t);
        if (rc != BSK_OK) { *err = s->err; return rc; }
        const size_t npieces = (n + DRAIN_PIECE - 1) / DRAIN_PIECE;
        auto piece_len = [&](size_t k) { return std::min(DRAIN_PIECE, n - k * DRAIN_PIECE); };
        if (seg)
            for (int b = 0; b < DRAIN_NBUF; ++b)
                if (!D->dev[b]) DR_TRY(hipMalloc((void**)&D->dev[b], DRAIN_PIECE));
        auto issue = [&](size_t k) -> hipError_t {
            const int b = (int)(k % DRAIN_NBUF);
            const uint8_t* from = d ? d + k * DRAIN_PIECE : D->dev[b];
            hipError_t e = hipSuccess;
            if (seg)  // the piece of the text out of its slices (the buffer is free: the D2H copy that read it was waited for before its piece was written)
                e = launch_seg_copy_range(seg->seg_src, seg->seg_off, seg->nseg, seg->first4k, D->dev[b], k * DRAIN_PIECE,
                                          k * DRAIN_PIECE + piece_len(k), seg->total, seg->lo, seg->hi, d2h);
            if (e == hipSuccess) e = hipMemcpyAsync(D->pin[b], from, piece_len(k), hipMemcpyDeviceToHost, d2h);
            return e == hipSuccess ? hipEventRecord(D->ev[b], d2h) : e;
        };
        // two copies in flight ahead of the piece being written (a buffer is free again once its piece has been written)
        for (size_t k = 0; k < std::min<size_t>(npieces, DRAIN_NBUF - 1); ++k) {
            const hipError_t e = issue(k);
            if (e != hipSuccess) return hipfail(e, "hipMemcpyAsync (drain)");
        }
        for (size_t k = 0; k < npieces && rc == BSK_OK; ++k) {
            const int b = (int)(k % DRAIN_NBUF);
            if (k + DRAIN_NBUF - 1 < npieces) {
                const hipError_t e = issue(k + DRAIN_NBUF - 1);
                if (e != hipSuccess) { rc = hipfail(e, "hipMemcpyAsync (drain)"); break; }
            }
            const hipError_t e = hipEventSynchronize(D->ev[b]);
            if (e != hipSuccess) { rc = hipfail(e, "hipEventSynchronize (drain)"); break; }
            const size_t len = piece_len(k);
            if (t.direct) {  // (the range is reserved: no lock is held while the bytes go out)
                if (!write_all(t.fd, D->pin[b], len, t.base + k * DRAIN_PIECE)) { *err = "libbsk: write failed: " + std::string(strerror(errno)); rc = BSK_ERR_INVALID_ARG; }
            } else {
                rc = store_append(s, part, D->pin[b], len, false);
                if (rc != BSK_OK) *err = s->err;
            }
        }
        if (rc != BSK_OK) { hipStreamSynchronize(d2h); return rc; }
    }
    if (last) {
        // a part that waits in memory is marked complete by an empty append; one whose turn it is hands over to its successors
        bool in_turn;
        { std::lock_guard<std::mutex> g(s->mu); in_turn = !s->merge || part == s->next; }
        rc = in_turn ? finish_part(s, part) : store_append(s, part, nullptr, 0, true);
        if (rc != BSK_OK) *err = s->err;
    }
    return rc;
#undef DR_TRY
}

}  // namespace

namespace bsk {
void store_drainer_free(bsk_ctx* c) {
    Drainer* d = (Drainer*)c->drainer;
    if (!d) return;
    for (int b = 0; b < DRAIN_NBUF; ++b) { if (d->pin[b]) hipHostFree(d->pin[b]); if (d->ev[b]) hipEventDestroy(d->ev[b]); if (d->dev[b]) hipFree(d->dev[b]); }
    delete d;
    c->drainer = nullptr;
}
}  // namespace bsk

extern "C" {

int bsk_store_open(const char* path, int merge, bsk_store** out) {
    if (!path || !out) return BSK_ERR_INVALID_ARG;
    bsk_store* s = new bsk_store;
    s->path = path;
    s->merge = merge != 0;
    if (s->merge) {
        s->fd = open(path, O_RDWR | O_CREAT | O_TRUNC, 0644);
        if (s->fd < 0) { delete s; return BSK_ERR_INVALID_ARG; }
    } else {
        struct stat sb;
        if (!(stat(path, &sb) == 0 && S_ISDIR(sb.st_mode)) && mkdir(path, 0755) != 0) { delete s; return BSK_ERR_INVALID_ARG; }
    }
    *out = s;
    return BSK_OK;
}

int bsk_store_set_bgzf(bsk_store* s, int on) {
    if (!s) return BSK_ERR_INVALID_ARG;
    if (s->touched) return store_fail(s, "libbsk: bsk_store_set_bgzf comes before the first put");
    s->bgzf = on != 0;
    s->bgzf_eof = on != 2;
    return BSK_OK;
}

const char* bsk_store_error(const bsk_store* s) { return s ? s->err.c_str() : ""; }

int bsk_store_put_host(bsk_store* s, uint64_t part, const void* data, size_t n) {
    if (!s || (n && !data)) return BSK_ERR_INVALID_ARG;
    s->touched = true;
    if (s->bgzf && n) {
        std::vector<uint8_t> comp(bgzf_deflate_bound(n, 0));
        size_t got = 0;
        std::string err;
        const int rc = bgzf_deflate_host(data, n, 0, false, comp.data(), comp.size(), &got, 0, err);
        if (rc != BSK_OK) { s->err = err; return rc; }
        return store_append(s, part, comp.data(), got, true);
    }
    return store_append(s, part, (const uint8_t*)data, n, true);
}

int bsk_store_put(bsk_store* s, bsk_ctx* c, uint64_t part, const bsk_out* o) {
    if (!s || !c || !o) return BSK_ERR_INVALID_ARG;
    s->touched = true;
    if (c->device < 0) { c->set_error("libbsk: context was created without a device"); return BSK_ERR_NO_DEVICE; }
    bsk_call_scope scope(c);
    if (!scope.owns) { c->set_error(BSK_BUSY_TEXT); return BSK_ERR_INVALID_ARG; }
    HIP_TRYX(c, hipSetDevice(c->device));
    HIP_TRYX(c, hipDeviceSynchronize());
    if (!c->copy_stream[1]) HIP_TRYX(c, hipStreamCreateWithFlags(&c->copy_stream[1], hipStreamNonBlocking));
    int rc = drainer_prepare(c);
    if (rc != BSK_OK) return rc;
    std::string err;
    if (o->n_segments && o->len) {
        // round 6: the result is a list of slices (include/bsk.h): every 32 MiB piece of the text is gathered out of them into
        // a staging buffer of the device and leaves from there -- the one block is never made
        const bsk_ctx::PendingOut& P = c->pend_out;
        if (P.kind == 0 || o->d_seg_src != P.seg_src || o->d_seg_off != P.seg_off || o->n_segments != P.nseg || o->len != P.total) {
            c->set_error("libbsk: this result is not the one the context holds as slices (a later run replaced it)");
            return BSK_ERR_INVALID_ARG;
        }
        rc = pending_first4k(c, nullptr);
        if (rc != BSK_OK) return rc;
        HIP_TRYX(c, hipDeviceSynchronize());
        rc = drain_to_store(c, s, part, nullptr, o->len, true, c->copy_stream[1], &err, &P);
    } else {
        rc = drain_to_store(c, s, part, (const uint8_t*)o->d_data, o->len, true, c->copy_stream[1], &err);
    }
    if (rc != BSK_OK) c->set_error(err);
    return rc;
}

int bsk_out_to_host_bgzf(bsk_ctx* c, const bsk_out* o, int eof, void* dst, size_t cap, size_t* n_comp) {
    if (!c || !o || !n_comp || (cap && !dst)) { if (c) c->set_error("libbsk: null argument"); return BSK_ERR_INVALID_ARG; }
    *n_comp = 0;
    if (c->device < 0) { c->set_error("libbsk: context was created without a device"); return BSK_ERR_NO_DEVICE; }
    bsk_call_scope scope(c);
    if (!scope.owns) { c->set_error(BSK_BUSY_TEXT); return BSK_ERR_INVALID_ARG; }
    HIP_TRYX(c, hipSetDevice(c->device));
    HIP_TRYX(c, hipDeviceSynchronize());
    const bsk_ctx::PendingOut* seg = nullptr;
    if (o->n_segments && o->len) {
        const bsk_ctx::PendingOut& P = c->pend_out;
        if (P.kind == 0 || o->d_seg_src != P.seg_src || o->d_seg_off != P.seg_off || o->n_segments != P.nseg || o->len != P.total) {
            c->set_error("libbsk: this result is not the one the context holds as slices (a later run replaced it)");
            return BSK_ERR_INVALID_ARG;
        }
        const int rc = pending_first4k(c, nullptr);
        if (rc != BSK_OK) return rc;
        HIP_TRYX(c, hipDeviceSynchronize());
        seg = &P;
    }
    std::string err;
    size_t at = 0;
    auto put = [&](const void* src, size_t n, bool on_device) {
        if (n > cap - at) { err = "libbsk: bgzf: the output buffer holds " + std::to_string(cap) + " bytes, the file needs more (bsk_bgzf_deflate_bound)"; return BSK_ERR_CAPACITY; }
        if (on_device) { if (n && hipMemcpy((uint8_t*)dst + at, src, n, hipMemcpyDeviceToHost) != hipSuccess) { err = "libbsk: bgzf: the D2H copy of a compressed piece failed"; return BSK_ERR_HIP; } }
        else memcpy((uint8_t*)dst + at, src, n);
        at += n;
        return BSK_OK;
    };
    int rc = bgzf_pieces(c, seg ? nullptr : (const uint8_t*)o->d_data, seg, o->len, &err, [&](const void* d_comp, size_t n) { return put(d_comp, n, true); });
    if (rc == BSK_OK && eof) {
        uint8_t e[28];
        bgzf_eof_block(e);
        rc = put(e, sizeof e, false);
    }
    if (rc != BSK_OK) { c->set_error(err); return rc; }
    *n_comp = at;
    return BSK_OK;
}

int bsk_store_close(bsk_store* s, uint64_t* total_bytes) {
    if (!s) return BSK_ERR_INVALID_ARG;
    int rc = BSK_OK;
    {
        std::lock_guard<std::mutex> g(s->mu);
        if (s->merge) {
            // parts that never became `next` (a gap in the part numbers): written in part order all the same
            for (auto& kv : s->parts) {
                if (!kv.second.bytes.empty()) {
                    if (!write_all(s->fd, kv.second.bytes.data(), kv.second.bytes.size(), s->offset)) rc = BSK_ERR_INVALID_ARG;
                    s->offset += kv.second.bytes.size();
                    s->total += kv.second.bytes.size();
                }
            }
            if (s->bgzf && s->fd >= 0 && !end_part_file(s, s->fd, s->offset)) rc = BSK_ERR_INVALID_ARG;
            if (s->fd >= 0) close(s->fd);
        } else {
            for (auto& kv : s->parts)
                if (kv.second.fd >= 0) {
                    if (!end_part_file(s, kv.second.fd, kv.second.off)) rc = BSK_ERR_INVALID_ARG;
                    close(kv.second.fd);
                }
        }
        if (total_bytes) *total_bytes = s->total;
    }
    delete s;
    return rc;
}

int bsk_run_to_store(bsk_ctx* c, const void* host_shard, size_t n, int format, int64_t pid, bsk_store* s, uint64_t part,
                     uint64_t* out_bytes, uint64_t* out_records) {
    if (!c || !s) return BSK_ERR_INVALID_ARG;
    s->touched = true;
    if (c->device < 0) { c->set_error("libbsk: context was created without a device"); return BSK_ERR_NO_DEVICE; }
    if (format != BSK_FORMAT_FASTA && format != BSK_FORMAT_FASTQ) { c->set_error("libbsk: bad format"); return BSK_ERR_INVALID_ARG; }
    if (n && !host_shard) { c->set_error("libbsk: null shard"); return BSK_ERR_INVALID_ARG; }
    const RecordOp r = record_op(c);
    if (r.store == RecordOp::NoStore) { c->set_error("libbsk: bsk_run_to_store: operator without a single-shard record output"); return BSK_ERR_INVALID_ARG; }
    if (out_bytes) *out_bytes = 0;      // (also on the early ways out: ADVICE r03)
    if (out_records) *out_records = 0;
    bsk_call_scope scope(c);
    if (!scope.owns) { c->set_error(BSK_BUSY_TEXT); return BSK_ERR_INVALID_ARG; }
    // replace: {nr} counts the records of this call from 1, across its chunks; with pin_alphabet set the caller says that
    // several calls carry ONE partition (the CLI's pieces of a worker's shard), and the count goes on from the last call
    if (!c->tune.is("pin_alphabet", "1")) c->nr_base = 0;
    // sample: the record index goes on across the chunks likewise, from bsk_sample_set_first_record's value (0 by default)
    if (!c->tune.is("pin_alphabet", "1")) c->sample_next = c->sample_first;
    // head-genome: prefix, n_1 and "cut reached" go on across the chunks likewise; a call is a file of its own otherwise
    if (c->op == Op::HeadGenome && !c->tune.is("pin_alphabet", "1")) head_genome_reset(c);
    // (the chunks' outputs are drained from the two output buffers while the next chunk computes: one block each, whatever
    // the switch "out" says)
    struct Contig { bsk_ctx* c; bool was; ~Contig() { c->force_contiguous = was; } } contig{c, c->force_contiguous};
    c->force_contiguous = true;
    c->pend_out.kind = 0;
    HIP_TRYX(c, hipSetDevice(c->device));
    for (int b = 0; b < 2; ++b)
        if (!c->copy_stream[b]) HIP_TRYX(c, hipStreamCreateWithFlags(&c->copy_stream[b], hipStreamNonBlocking));
    if (!c->own_stream) HIP_TRYX(c, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    hipStream_t st = c->own_stream, h2d = c->copy_stream[0], d2h = c->copy_stream[1];
    int rc = drainer_prepare(c);  // (pinned buffers and events exist before the writer thread does)
    if (rc != BSK_OK) return rc;
    // everything the call borrows from the context or creates goes back on EVERY way out: the spare output buffer (the
    // two are swapped per chunk -- left swapped, the next call would drain one chunk while computing the next in the
    // same memory), the events, the alphabet pinned for the chunks, the writer thread
    struct Scope {
        bsk_ctx* c;
        uint8_t* alt_out;
        uint64_t alt_cap;
        bool swapped = false;
        hipEvent_t in_done[2] = {nullptr, nullptr}, in_free[2] = {nullptr, nullptr};
        std::future<std::pair<int, std::string>> writer;
        Alphabet saved_alphabet;
        bool alphabet_pinned = false;
        ~Scope() {
            if (writer.valid()) writer.get();
            if (swapped) { std::swap(c->d_out, alt_out); std::swap(c->out_cap, alt_cap); }
            c->d_out_alt = alt_out;
            c->out_alt_cap = alt_cap;
            if (alphabet_pinned) { c->alphabet = saved_alphabet; c->alphabet_guessed = false; }
            for (int b = 0; b < 2; ++b) { if (in_done[b]) hipEventDestroy(in_done[b]); if (in_free[b]) hipEventDestroy(in_free[b]); }
        }
    } S{c, c->d_out_alt, c->out_alt_cap};
    S.saved_alphabet = c->alphabet;
    for (int b = 0; b < 2; ++b) {
        HIP_TRYX(c, hipEventCreateWithFlags(&S.in_done[b], hipEventDisableTiming));
        HIP_TRYX(c, hipEventCreateWithFlags(&S.in_free[b], hipEventDisableTiming));
    }
    const char* env = c->tune.get("stage_bytes");
    const size_t want = env && strtoull(env, nullptr, 10) ? (size_t)strtoull(env, nullptr, 10) : ((size_t)256 << 20);
    // records wrapped over several lines: the cut points below assume 4-line records, so the shard goes as one piece
    const bool chunkable = r.store == RecordOp::Chunks &&
                           !(format == BSK_FORMAT_FASTQ && fastq_head_multiline((const uint8_t*)host_shard, std::min<size_t>(n, 256 * 1024)));
    const uint8_t* h = (const uint8_t*)host_shard;
    const std::vector<size_t> cuts = record_cuts(h, n, format, chunkable ? want : n);
    const size_t nchunks = cuts.size() - 1;
    uint64_t bytes = 0, records = 0;
    auto stage_in = [&](size_t i) -> int {  // H2D of chunk i into input buffer i & 1
        const int b = (int)(i & 1);
        const size_t len = cuts[i + 1] - cuts[i];
        const int rcs = stage_reserve(c, b, len, len / 16, 4096, /*drain=*/true, st);
        if (rcs != BSK_OK) return rcs;
        if (i >= 2) HIP_TRYX(c, hipStreamWaitEvent(h2d, S.in_free[b], 0));
        HIP_TRYX(c, hipMemcpyAsync(c->d_stage[b], h + cuts[i], len, hipMemcpyHostToDevice, h2d));
        HIP_TRYX(c, hipEventRecord(S.in_done[b], h2d));
        return BSK_OK;
    };
    if (nchunks == 0) return store_append(s, part, nullptr, 0, true);
    rc = stage_in(0);
    // the output of chunk i is drained (D2H + write, on a writer thread) while chunk i+1 computes: two output buffers,
    // swapped with the context's; the drain of chunk i must be over before chunk i+2 reuses its buffer, and before the
    // drain of chunk i+1 starts (the bytes of a part are appended in order)
    for (size_t i = 0; i < nchunks && rc == BSK_OK; ++i) {
        const int b = (int)(i & 1);
        if (i + 1 < nchunks) { rc = stage_in(i + 1); if (rc != BSK_OK) break; }
        HIP_TRYX(c, hipStreamWaitEvent(st, S.in_done[b], 0));
        HIP_TRYX(c, hipMemsetAsync(c->d_status, 0, 8 * sizeof(uint64_t), st));
        c->cur_pid = (pid == 0 && i == 0) ? 0 : (pid == 0 ? 1 : pid);  // locate: the header row belongs to the first chunk of partition 0
        // SeqType auto: the reference guesses the alphabet ONCE per partition, from its first record (helper.go:286-291);
        // a chunk that guessed from its own first record could search other strands or validate other letters than a
        // run over the whole shard.  The guess of chunk 0 is pinned for the rest of the call.
        // (switch "pin_alphabet": the caller feeds ONE partition through several calls -- the command line's pieces of a shard
        // that does not fit the GPU -- and the guess of the first call's first record stays for all of them)
        const bool pin_for_good = c->tune.is("pin_alphabet", "1");
        if (i == 0 && (nchunks > 1 || pin_for_good) && c->alphabet == AB_NONE && c->op != Op::Duplicate) {
            HIP_TRYX(c, hipStreamSynchronize(st));  // (chunk 0 is on the device: its head is read back)
            int arc = BSK_OK;
            const Alphabet ab = partition_alphabet(c, c->d_stage[b], cuts[1] - cuts[0], format, st, &arc);
            if (arc != BSK_OK) { rc = arc; break; }
            c->alphabet = ab;
            c->alphabet_guessed = true;
            S.alphabet_pinned = !pin_for_good;
        }
        std::swap(c->d_out, S.alt_out);
        std::swap(c->out_cap, S.alt_cap);
        S.swapped = !S.swapped;
        bsk_out o;
        memset(&o, 0, sizeof o);
        ++c->call_gen;  // (the staging buffers come round again with other text: nothing sampled from chunk i - 2 may survive)
        // a chunk whose head is wrapped runs on its rewrite (only then: the cuts assume 4-line records further down)
        rc = run_multiline(c, [&](const uint8_t* t, const uint64_t* e) { return r.fn(c, t, e[0], format, st, &o); }, c->d_stage[b],
                           {cuts[i + 1] - cuts[i]}, format, st, /*head_only=*/true);
        if (rc != BSK_OK) break;
        HIP_TRYX(c, hipStreamSynchronize(st));  // the output is complete (the run functions end with launches in flight)
        HIP_TRYX(c, hipEventRecord(S.in_free[b], st));
        if (S.writer.valid()) {
            auto w = S.writer.get();
            if (w.first != BSK_OK) { c->set_error(w.second); rc = w.first; break; }
        }
        const uint8_t* od = (const uint8_t*)o.d_data;
        const size_t ol = o.len;
        const bool last = i + 1 == nchunks;
        S.writer = std::async(std::launch::async, [=]() {
            std::string err;
            const int wrc = drain_to_store(c, s, part, od, ol, last, d2h, &err);
            return std::make_pair(wrc, err);
        });
        bytes += o.len;
        records += o.records;
    }
    if (S.writer.valid()) {
        auto w = S.writer.get();
        if (rc == BSK_OK && w.first != BSK_OK) { c->set_error(w.second); rc = w.first; }
    }
    if (out_bytes) *out_bytes = bytes;
    if (out_records) *out_records = records;
    return rc;
}

}  // extern "C"
