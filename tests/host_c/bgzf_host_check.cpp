// The BGZF decoder alone under the host's sanitizers: this program includes bgzf_inflate_dev.hpp and nothing of the library.
//     bgzf_host_check <file> <expected>       the file must inflate to the bytes of <expected>: prints "ok <bytes>"
//     bgzf_host_check <file> -                the file must be REFUSED: prints "refused <block> <code>"
// It walks the chain of blocks itself (parse_header), decodes every block with the host's lane and exits 0 when the file did
// what the caller said it would, 1 when not, 2 on a usage error.  tests/test_bgzf_cpu.py builds it with
// -fsanitize=address,undefined and runs it over the corpus and over every malformed input.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../bigseqkit_amd/csrc/bgzf_inflate_dev.hpp"

using namespace bsk::bgzf;

static bool slurp(const char* path, std::vector<uint8_t>& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + k);
    fclose(f);
    return true;
}

static uint32_t le32(const uint8_t* p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// 0 and the text, or the failing block and its code (a code of 100 + r: the header at that offset is not a block header)
static int inflate_file(const std::vector<uint8_t>& comp, std::vector<uint8_t>& text, uint64_t* bad_block) {
    std::unique_ptr<BgzfLds> S(new BgzfLds);
    memset(S->crc_mat, 0, sizeof S->crc_mat);
    uint64_t k = 0;
    for (uint64_t off = 0; off < comp.size(); ++k) {
        *bad_block = k;
        BlockHeader h{0, 0};
        const int r = parse_header(comp.data() + off, comp.size() - off, &h);
        if (r != 1) return 100 + r;
        if (h.bsize < 12u + h.xlen + 8u || off + h.bsize > comp.size()) return ERR_TRUNCATED;
        const uint8_t* t = comp.data() + off + h.bsize - 8;
        const uint32_t isize = le32(t + 4);
        if (isize > MAX_ISIZE) return ERR_ISIZE;
        // (the output of a block is a buffer of its own of exactly ISIZE bytes: a byte written past it is the sanitizer's to find)
        std::vector<uint8_t> out(isize);
        std::vector<uint8_t> block(comp.begin() + (long)off, comp.begin() + (long)(off + h.bsize));  // ... and so is a byte read past the block
        HostLane io{block.data(), block.size(), out.data()};
        Inflater<HostLane> I(io, *S);
        const int e = I.run(12u + h.xlen, h.bsize - 8u, isize, le32(t), 0);
        if (e != OK) return e;
        text.insert(text.end(), out.begin(), out.end());
        off += h.bsize;
    }
    return OK;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: bgzf_host_check <file> <expected | ->\n"); return 2; }
    std::vector<uint8_t> comp, want, text;
    if (!slurp(argv[1], comp)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    const bool refuse = !strcmp(argv[2], "-");
    if (!refuse && !slurp(argv[2], want)) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    // the chunked CRC, as the kernel folds it, on the whole file's bytes (any bytes will do)
    {
        const uint32_t n = (uint32_t)(comp.size() < 65536 ? comp.size() : 65536);
        uint32_t mat[32], tab[256];
        crc_advance_matrix(mat, 1024);
        for (uint32_t i = 0; i < 256; ++i) tab[i] = crc_table_entry(i);
        auto crc_of = [&](uint32_t a, uint32_t b) { uint32_t c = ~0u; for (uint32_t q = a; q < b; ++q) c = tab[(c ^ comp[q]) & 255u] ^ (c >> 8); return ~c; };
        const uint32_t folded = crc_fold(mat, (n + 1023) / 1024, [&](uint32_t k) { const uint32_t ce = n - k * 1024; return crc_of(ce > 1024 ? ce - 1024 : 0, ce); });
        if (folded != (n ? crc_of(0, n) : 0u)) { printf("crc fold differs\n"); return 1; }
    }
    uint64_t bad = 0;
    const int e = inflate_file(comp, text, &bad);
    if (refuse) {
        if (e == OK) { printf("accepted %zu\n", text.size()); return 1; }
        printf("refused %llu %d\n", (unsigned long long)bad, e);
        return 0;
    }
    if (e != OK) { printf("refused %llu %d\n", (unsigned long long)bad, e); return 1; }
    if (text != want) { printf("differs %zu %zu\n", text.size(), want.size()); return 1; }
    printf("ok %zu\n", text.size());
    return 0;
}
