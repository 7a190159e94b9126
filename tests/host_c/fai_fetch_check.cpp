// The indexed fetch of `faidx -d` on the host, alone under the host's sanitizers: this program includes fai_fetch.hpp (the
// planner, the batch steps, the one-lane tile of fai_fetch_dev.hpp) and nothing of the library.
//     fai_fetch_check <sequence file> <index file> <LineWidth> <budget> <text out> [<name> <s> <e> <minus 0|1> <suffix>]...
// The queries are given resolved (what validate_faidx_opts leaves in the context; "-" is an empty suffix).  It plans, reads
// every batch's spans into a buffer of exactly the planned size, runs the tiles and writes the joined text to <text out>.
// The last line is "ok <hits> <batches> <bytes read>" or "refused <code> <message>".  Exit 0 unless the call was wrong (2).
// The complement table is the plain one of ACGTN.  tests/test_faidx_fetch_cpu.py builds it with -fsanitize=address,undefined.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../../bigseqkit_amd/csrc/fai_fetch.hpp"

using namespace bsk;

static std::string slurp(const char* path) {
    std::string s;
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    char buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, k);
    fclose(f);
    return s;
}

int main(int argc, char** argv) {
    if (argc < 6 || (argc - 6) % 5 != 0) { fprintf(stderr, "usage: see the head of fai_fetch_check.cpp\n"); return 2; }
    const std::string index = slurp(argv[2]);
    const int fd = open(argv[1], O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    fai::Options o;
    o.line_width = (uint32_t)atoi(argv[3]);
    o.budget = strtoull(argv[4], nullptr, 10);
    for (int k = 6; k < argc; k += 5) {
        const std::string suffix = argv[k + 4];
        o.queries.push_back(fai::Query{argv[k], suffix == "-" ? std::string() : suffix, atoll(argv[k + 1]), atoll(argv[k + 2]), atoi(argv[k + 3]) != 0});
    }
    fai::Plan plan;
    std::string err;
    int rc = fai::parse_rows(index, (uint64_t)sb.st_size, -1, false, &plan, &err);
    if (rc == 0) rc = fai::make_plan(o, &plan, &err);
    if (rc != 0) { printf("refused %d %s\n", rc, err.c_str()); return 0; }
    uint8_t comp[256];
    for (int i = 0; i < 256; ++i) comp[i] = (uint8_t)i;
    const char *from = "ACGTNacgtn", *to = "TGCANtgcan";
    for (int i = 0; from[i]; ++i) comp[(uint8_t)from[i]] = (uint8_t)to[i];
    FILE* out = fopen(argv[5], "wb");
    if (!out) { fprintf(stderr, "cannot create %s\n", argv[5]); return 2; }
    uint64_t read_bytes = 0;
    for (size_t b = 0; b < plan.batches.size(); ++b) {
        const fai::Batch& B = plan.batches[b];
        const fai::Layout L = fai::layout(B);
        std::unique_ptr<uint8_t[]> buf(new uint8_t[L.bytes]);  // (exactly the planned bytes: a read beside them is a report)
        memset(buf.get(), 0, L.bytes);
        for (size_t k = 0; k < B.spans.size(); ++k) {
            const uint64_t n = B.spans[k].hi - B.spans[k].lo;
            if (pread(fd, buf.get() + L.slot[k], n, (off_t)B.spans[k].lo) != (ssize_t)n) { fprintf(stderr, "short read\n"); return 2; }
            read_bytes += n;
        }
        fai::Tables T;
        rc = fai::prepare(plan, b, L, buf.get(), &T, &err);
        if (rc != 0) { printf("refused %d %s\n", rc, err.c_str()); fclose(out); return 0; }
        std::unique_ptr<uint8_t[]> text(new uint8_t[T.out_bytes ? T.out_bytes : 1]);
        const uint64_t word = fai::run_host(T, buf.get(), plan.line_width, comp, text.get());
        if (word != fai::FETCH_NO_FAULT) {
            printf("refused %d %s\n", fai::ERR_FORMAT, fai::fault_text(plan, b, T, word).c_str());
            fclose(out);
            return 0;
        }
        fwrite(text.get(), 1, T.out_bytes, out);
    }
    fclose(out);
    close(fd);
    printf("ok %zu %zu %llu\n", plan.hits.size(), plan.batches.size(), (unsigned long long)read_bytes);
    return 0;
}
