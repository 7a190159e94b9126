// The speculative gzip reader alone under the host's sanitizers: this program includes gzip_spec_dev.hpp and nothing of the
// library.
//     gzip_host_check <file> <expected> <chunk_bytes>   the file must inflate to the bytes of <expected>, in one piece and in
//                                                       chunks: prints "ok <bytes> <chunks on the chain>"
//     gzip_host_check <file> - <chunk_bytes>            the file must be REFUSED both ways: prints "refused <kind>: <text>"
// Besides, the finder's predicate is held against the decoder itself: at every bit of the first 1 KiB of the file, and of the
// 1 KiB around the file's middle, header_ok says yes exactly where the three bits read BFINAL 0, BTYPE 2 and
// HuffCore::tables(2) returns OK.  Exit 0 when the file did what the caller said it would, 1 when not, 2 on a usage error.
// tests/test_gzip_cpu.py builds it with -fsanitize=address,undefined and runs it over the corpus and the malformed inputs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../bigseqkit_amd/csrc/gzip_spec_dev.hpp"

using namespace bsk;

static bool slurp(const char* path, std::vector<uint8_t>& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + k);
    fclose(f);
    return true;
}

// what the decoder says of a dynamic non-final block at bit `pos`
static bool decoder_takes(const std::vector<uint8_t>& comp, gz::GzTables& T, uint64_t pos) {
    gz::HostLane io{comp.data(), comp.size()};
    gz::Walker<gz::HostLane, false> W(io, T, nullptr);
    W.in_end = comp.size();
    W.seek(pos >> 3);
    if (!W.drop((uint32_t)(pos & 7u))) return false;
    W.need32();
    const uint32_t head = W.peek(3);
    if (!W.drop(3) || head != 4u) return false;
    return W.tables(2u) == bgzf::OK;
}

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: gzip_host_check <file> <expected | -> <chunk_bytes>\n"); return 2; }
    std::vector<uint8_t> comp, want;
    if (!slurp(argv[1], comp)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    const bool refuse = !strcmp(argv[2], "-");
    if (!refuse && !slurp(argv[2], want)) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    const uint64_t chunk = strtoull(argv[3], nullptr, 10);
    // (the bytes in a buffer of exactly their size: a byte read past it is the sanitizer's to find)
    std::vector<uint8_t> exact(comp.begin(), comp.end());
    {
        std::unique_ptr<gz::GzTables> T(new gz::GzTables);
        const gz::HostLane io{exact.data(), exact.size()};
        auto word = [&](uint64_t w) { return io.word(w); };
        const uint64_t total = 8ull * exact.size(), span = 8192;
        const uint64_t from[2] = {0, total / 2 > span / 2 ? total / 2 - span / 2 : 0};
        for (int part = 0; part < 2; ++part)
            for (uint64_t pos = from[part]; pos < from[part] + span && pos < total; ++pos)
                if (gz::header_ok(word, total, pos) != decoder_takes(exact, *T, pos)) {
                    printf("the finder and the decoder differ at bit %llu\n", (unsigned long long)pos);
                    return 1;
                }
    }
    std::string err[2];
    std::vector<uint8_t> text[2];
    gz::Plan plan[2];
    int rc[2];
    for (int i = 0; i < 2; ++i) rc[i] = gz::inflate_host(exact.data(), exact.size(), i ? chunk : 0, text[i], plan[i], err[i]);
    if (refuse) {
        if (rc[0] == gz::FAIL_NONE || rc[1] == gz::FAIL_NONE) { printf("accepted %zu %zu\n", text[0].size(), text[1].size()); return 1; }
        if (rc[0] != rc[1]) { printf("refused differently: %s / %s\n", err[0].c_str(), err[1].c_str()); return 1; }
        printf("refused %d: %s\n", rc[1], err[1].c_str());
        return 0;
    }
    for (int i = 0; i < 2; ++i) {
        if (rc[i] != gz::FAIL_NONE) { printf("refused %d: %s\n", rc[i], err[i].c_str()); return 1; }
        if (text[i] != want) { printf("differs %zu %zu\n", text[i].size(), want.size()); return 1; }
    }
    printf("ok %zu %llu\n", want.size(), (unsigned long long)plan[1].on_chain);
    return 0;
}
