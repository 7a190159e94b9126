// The cut points of a BGZF file for several workers on the host, alone under the host's sanitizers: this program includes
// bgzf_cuts.hpp (the candidate scan, the chain test, the record cut, the decoder's host lane) and nothing of the library.
//     bgzf_cuts_check <file> <format 0|1> <world>
// It prints "ok <voff 0> ... <voff world>" or "refused <code> <message>".  Exit 0 unless the call was wrong (2).
// tests/test_bgzf_devices_cpu.py builds it with -fsanitize=address,undefined.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>

#include "../../bigseqkit_amd/csrc/bgzf_cuts.hpp"

using namespace bsk;

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: bgzf_cuts_check <file> <format> <world>\n"); return 2; }
    const int fd = open(argv[1], O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    const int world = atoi(argv[3]);
    if (world < 1) { fprintf(stderr, "bad world\n"); return 2; }
    BgzfCutter cutter([fd](uint64_t off, size_t len, uint8_t* dst) {
        size_t at = 0;
        while (at < len) {
            const ssize_t k = pread(fd, dst + at, len - at, (off_t)(off + at));
            if (k <= 0) return false;
            at += (size_t)k;
        }
        return true;
    }, (uint64_t)sb.st_size, atoi(argv[2]));
    std::vector<uint64_t> voffs((size_t)world + 1, 0);
    const int rc = cutter.cut_points(world, voffs.data());
    if (rc != BSK_OK) { printf("refused %d %s\n", rc, cutter.error().c_str()); return 0; }
    printf("ok");
    for (uint64_t v : voffs) printf(" %llu", (unsigned long long)v);
    printf("\n");
    close(fd);
    return 0;
}
