// The BGZF encoder alone (bgzf_deflate_dev.hpp with one host lane) and the decoder alone (bgzf_inflate_dev.hpp), nothing of the
// library: every file named on the command line is cut into blocks, encoded, decoded back and compared.  Built by
// tests/test_bgzf_write_cpu.py with the host's address and undefined-behaviour sanitizers.
//   bgzf_deflate_check [-b block_bytes] [-o compressed_out] file...
// prints "ok <text bytes> <compressed bytes> <blocks>" per file; exit 1 on the first difference.  -o keeps the last file's
// BGZF image (the members and the EOF block), which the test compares with the library's bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../bigseqkit_amd/csrc/bgzf_deflate_dev.hpp"

using namespace bsk::bgzf;

static bool read_file(const char* path, std::vector<uint8_t>& data) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + got);
    fclose(f);
    return true;
}

int main(int argc, char** argv) {
    uint32_t bt = BLOCK_TEXT;
    const char* keep = nullptr;
    int a = 1;
    for (; a + 1 < argc && argv[a][0] == '-'; a += 2) {
        if (!strcmp(argv[a], "-b")) bt = (uint32_t)strtoul(argv[a + 1], nullptr, 10);
        else if (!strcmp(argv[a], "-o")) keep = argv[a + 1];
        else break;
    }
    if (bt == 0 || bt > BLOCK_TEXT || a >= argc) {
        fprintf(stderr, "usage: bgzf_deflate_check [-b block_bytes <= 65280] [-o out] file...\n");
        return 2;
    }
    std::unique_ptr<DeflateLds> S(new DeflateLds);
    std::unique_ptr<BgzfLds> I(new BgzfLds);
    memset(S->crc_mat, 0, sizeof S->crc_mat);   // (one chunk per block on the host: never applied)
    memset(I->crc_mat, 0, sizeof I->crc_mat);
    std::vector<uint32_t> toks(bt + 1u);
    std::vector<uint8_t> slot(slot_bytes(bt)), back(bt), image;
    for (; a < argc; ++a) {
        std::vector<uint8_t> text;
        if (!read_file(argv[a], text)) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        image.clear();
        size_t blocks = 0;
        for (size_t off = 0; off < text.size(); off += bt, ++blocks) {
            const uint32_t n = (uint32_t)(text.size() - off < bt ? text.size() - off : bt);
            HostDeflateLane io{text.data() + off, toks.data(), slot.data()};
            Deflater<HostDeflateLane> D(io, *S);
            D.init();
            const uint32_t size = D.run(n);
            if (size > n + MEMBER_EXTRA || size > 65536u) { printf("block %zu of %s: %u bytes for %u of text\n", blocks, argv[a], size, n); return 1; }
            BlockHeader h{0, 0};
            if (parse_header(slot.data(), size, &h) != 1 || h.bsize != size || h.xlen != 6u) { printf("block %zu of %s: bad header\n", blocks, argv[a]); return 1; }
            const uint8_t* t = slot.data() + size - 8;
            const uint32_t crc = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
            const uint32_t isize = t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
            if (isize != n) { printf("block %zu of %s: ISIZE %u for %u\n", blocks, argv[a], isize, n); return 1; }
            HostLane in{slot.data(), size, back.data()};
            Inflater<HostLane> R(in, *I);
            const int rc = R.run(18u, size - 8u, isize, crc, 0);
            if (rc != OK) { printf("block %zu of %s: the decoder says %s\n", blocks, argv[a], error_text(rc)); return 1; }
            if (memcmp(back.data(), text.data() + off, n) != 0) { printf("block %zu of %s: decoded bytes differ\n", blocks, argv[a]); return 1; }
            image.insert(image.end(), slot.begin(), slot.begin() + size);
        }
        for (uint32_t i = 0; i < EOF_BYTES; ++i) image.push_back(eof_byte(i));
        printf("ok %zu %zu %zu\n", text.size(), image.size(), blocks);
    }
    if (keep) {
        FILE* f = fopen(keep, "wb");
        if (!f || fwrite(image.data(), 1, image.size(), f) != image.size()) { fprintf(stderr, "cannot write %s\n", keep); return 2; }
        fclose(f);
    }
    return 0;
}
