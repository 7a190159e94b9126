// The piece reader of a plain gzip file on the host, alone under the host's sanitizers: this program includes gzip_stream.hpp
// (the reader, its host backend, the speculative method, the record-start rules) and nothing of the library.
//     gzip_stream_check <file> <format 0|1> <piece> <lookahead> <segment> <chunk> <text out>
// It reads the file piece by piece, writes the joined text to <text out> and prints one line "piece <text_lo> <text_hi> <n>"
// per piece; then it asks for every piece again by its offsets, from the last to the first and once more in order, and
// compares the bytes; then it runs the sequential pass again behind them.  The last line is "ok <pieces> <bytes> <segments>
// <doublings>", "refused <code> <message>" or "differs ...".  Exit 0 unless the reader contradicted itself (1) or the call was
// wrong (2).  tests/test_gzip_stream_cpu.py builds it with -fsanitize=address,undefined.
#include <fcntl.h>
#include <sys/stat.h>

#include <cstdio>

#include "../../bigseqkit_amd/csrc/gzip_stream.hpp"

using namespace bsk;

int main(int argc, char** argv) {
    if (argc != 8) { fprintf(stderr, "usage: gzip_stream_check <file> <format> <piece> <lookahead> <segment> <chunk> <text out>\n"); return 2; }
    const int fd = open(argv[1], O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    auto num = [&](int k) { return (size_t)strtoull(argv[k], nullptr, 10); };
    GzipPieceReader R(std::unique_ptr<GzipStreamBackend>(new GzipHostBackend()), fd, (uint64_t)sb.st_size, atoi(argv[2]), num(3), num(4), num(5), num(6));
    if (R.open() != BSK_OK) { printf("refused open %s\n", R.error().c_str()); return 0; }
    struct P { uint64_t lo, hi; std::vector<uint8_t> bytes; };
    std::vector<P> pieces;
    FILE* out = fopen(argv[7], "wb");
    if (!out) { fprintf(stderr, "cannot write %s\n", argv[7]); return 2; }
    size_t total = 0;
    for (;;) {
        const void* p = nullptr;
        size_t n = 0;
        uint64_t lo = 0, hi = 0;
        int last = 0;
        const int rc = R.next(&p, &n, &lo, &hi, &last);
        if (rc != BSK_OK) { printf("refused %d %s\n", rc, R.error().c_str()); fclose(out); return 0; }
        printf("piece %llu %llu %zu\n", (unsigned long long)lo, (unsigned long long)hi, n);
        // (a copy of exactly n bytes: a byte read past the piece is the sanitizer's to find)
        pieces.push_back(P{lo, hi, std::vector<uint8_t>((const uint8_t*)p, (const uint8_t*)p + n)});
        fwrite(p, 1, n, out);
        total += n;
        if (last) break;
    }
    fclose(out);
    for (int pass = 0; pass < 2; ++pass)
        for (size_t k = 0; k < pieces.size(); ++k) {
            const P& w = pieces[pass == 0 ? pieces.size() - 1 - k : k];
            const void* p = nullptr;
            size_t n = 0;
            if (R.piece(w.lo, w.hi, &p, &n) != BSK_OK) { printf("differs: piece %llu refused: %s\n", (unsigned long long)w.lo, R.error().c_str()); return 1; }
            if (n != w.bytes.size() || (n && memcmp(p, w.bytes.data(), n))) { printf("differs: piece %llu has other bytes\n", (unsigned long long)w.lo); return 1; }
        }
    {   // the sequential pass behind the pieces: an empty last piece, the members' checks taken up where they are known
        const void* p = nullptr;
        size_t n = 0;
        uint64_t lo = 0, hi = 0;
        int last = 0;
        if (R.next(&p, &n, &lo, &hi, &last) != BSK_OK || n != 0 || !last || lo != total) { printf("differs: the pass behind the last piece gave %zu bytes at %llu\n", n, (unsigned long long)lo); return 1; }
    }
    uint64_t info[8];
    R.info(info);
    printf("ok %zu %zu %llu %llu\n", pieces.size(), total, (unsigned long long)info[0], (unsigned long long)info[2]);
    return 0;
}
