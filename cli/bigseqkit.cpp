// bigseqkit -- seqkit-compatible command line for the seven hot-path commands, on libbsk.so.
//
// Mirrors the cobra CLI of the reference (flag names, shorthands and defaults):
//   persistent flags   /root/reference/bigseqkit-cli/helper.go:161-173
//   seq / stats / grep / locate / subseq / translate / rmdup flag tables
//                      bigseqkit-cli/{seq.go:54-73, stats.go:61-65, grep.go:81-96, locate.go:61-74,
//                                     subseq.go:56-67, translate.go:86-94, rmdup.go:45-51}
//   input sniffing     bigseqkit-cli/helper.go:63-78   (extension, then first byte)
//   output naming      bigseqkit-cli/helper.go:105-127 (<file>-out, --merge: one file, else a directory of parts)
// Where the reference builds an IgnisHPC dataflow (ignisDriver, helper.go:87-132) this program
// builds the option JSON of the command (same schema as bigseqkit.OptionsToString) and drives the
// C ABI of include/bsk.h: one bsk_create, one bsk_<op>_run per input file (partition), bsk_destroy.
// Extras of this CLI: --device N, --dry-run (print the operator name and option JSON, no GPU needed),
// and "-o -" for standard output.
#include <execinfo.h>
#include <fcntl.h>
#include <signal.h>
#include <unistd.h>
#include <sys/mman.h>
#include <sys/sendfile.h>
#include <sys/stat.h>

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <atomic>
#include <future>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include <chrono>

#include "../include/bsk.h"
#include "../bigseqkit_amd/csrc/json.hpp"

namespace {

enum Kind { BOOL, INT, FLOAT, STR, SLICE };
struct Flag {
    const char* name;  // long name
    char shorthand;    // 0 = none
    Kind kind;
    const char* field;  // JSON field ("" = CLI-only), prefixed with "Config." for KitConfig
    const char* def;    // textual default
};

const Flag kPersistent[] = {
    {"seq-type", 't', STR, "Config.SeqType", "auto"},
    {"line-width", 'w', INT, "Config.LineWidth", "60"},
    {"id-regexp", 0, STR, "Config.IDRegexp", "^(\\S+)\\s?"},
    {"id-ncbi", 0, BOOL, "Config.IDNCBI", "false"},
    {"out-file", 'o', STR, "", ""},
    {"quiet", 0, BOOL, "Config.Quiet", "false"},
    {"alphabet-guess-seq-length", 0, INT, "Config.AlphabetGuessSeqLength", "10000"},
    {"infile-list", 0, STR, "", ""},
    {"merge", 0, BOOL, "", "false"},
    {"partitions", 0, INT, "", "0"},
    {"order", 0, BOOL, "", "false"},
    {"device", 0, INT, "", "0"},
    {"dry-run", 0, BOOL, "", "false"},
    {"plan", 0, BOOL, "", "false"},      // one JSON object: operator, options, files, output place (python -m bigseqkit_amd.run)
    {"devices", 0, STR, "", ""},         // "0,1,2,3" / "0-7": one worker THREAD per GPU in this process, collectives over librccl
                                         // (run_devices below); a device named twice shares its GPU (tests)
};

struct Command {
    const char* use;
    const char* op;  // operator name for bsk_create
    std::vector<Flag> flags;
    const char* help = nullptr;  // the reference's Long text and flag lines, printed by -h / --help (commands that carry one)
};

const Command kCommands[] = {
    {"seq", "SeqTransform",
     {{"reverse", 'r', BOOL, "Reverse", "false"}, {"complement", 'p', BOOL, "Complement", "false"},
      {"name", 'n', BOOL, "Name", "false"}, {"seq", 's', BOOL, "Seq", "false"}, {"qual", 'q', BOOL, "Qual", "false"},
      {"only-id", 'i', BOOL, "OnlyId", "false"}, {"remove-gaps", 'g', BOOL, "RemoveGaps", "false"},
      {"gap-letters", 'G', STR, "GapLetters", "- \t."}, {"lower-case", 'l', BOOL, "LowerCase", "false"},
      {"upper-case", 'u', BOOL, "UpperCase", "false"}, {"dna2rna", 0, BOOL, "Dna2rna", "false"},
      {"rna2dna", 0, BOOL, "Rna2dna", "false"}, {"color", 'k', BOOL, "", "false"},
      {"validate-seq", 'v', BOOL, "ValidateSeq", "false"}, {"validate-seq-length", 'V', INT, "ValidateSeqLength", "10000"},
      {"min-len", 'm', INT, "MinLen", "-1"}, {"max-len", 'M', INT, "MaxLen", "-1"},
      {"qual-ascii-base", 'b', INT, "QualAsciiBase", "33"}, {"min-qual", 'Q', FLOAT, "MinQual", "-1"},
      {"max-qual", 'R', FLOAT, "MaxQual", "-1"}}},
    {"stats", "Stats",
     {{"tabular", 'T', BOOL, "Tabular", "false"}, {"gap-letters", 'G', STR, "GapLetters", "- ."},
      {"all", 'a', BOOL, "All", "false"}, {"skip-err", 'e', BOOL, "SkipErr", "false"},
      {"fq-encoding", 'E', STR, "FqEncoding", "sanger"}}},
    {"grep", "Grep",
     {{"pattern", 'p', SLICE, "Pattern", ""}, {"pattern-file", 'f', STR, "PatternFile", ""},
      {"use-regexp", 'r', BOOL, "UseRegexp", "false"}, {"delete-matched", 0, BOOL, "DeleteMatched", "false"},
      {"invert-match", 'v', BOOL, "InvertMatch", "false"}, {"by-name", 'n', BOOL, "ByName", "false"},
      {"by-seq", 's', BOOL, "BySeq", "false"}, {"only-positive-strand", 'P', BOOL, "OnlyPositiveStrand", "false"},
      {"max-mismatch", 'm', INT, "MaxMismatch", "0"}, {"ignore-case", 'i', BOOL, "IgnoreCase", "false"},
      {"degenerate", 'd', BOOL, "Degenerate", "false"}, {"region", 'R', STR, "Region", ""},
      {"circular", 'c', BOOL, "Circular", "false"}, {"immediate-output", 'I', BOOL, "", "false"},
      {"count", 'C', BOOL, "Count", "false"}}},
    {"locate", "Locate",
     {{"pattern", 'p', SLICE, "Pattern", ""}, {"pattern-file", 'f', STR, "PatternFile", ""},
      {"degenerate", 'd', BOOL, "Degenerate", "false"}, {"use-regexp", 'r', BOOL, "UseRegexp", "false"},
      {"use-fmi", 'F', BOOL, "UseFmi", "false"}, {"ignore-case", 'i', BOOL, "IgnoreCase", "false"},
      {"only-positive-strand", 'P', BOOL, "OnlyPositiveStrand", "false"},
      {"validate-seq-length", 'V', INT, "ValidateSeqLength", "10000"}, {"non-greedy", 'G', BOOL, "NonGreedy", "false"},
      {"gtf", 0, BOOL, "Gtf", "false"}, {"bed", 0, BOOL, "Bed", "false"}, {"max-mismatch", 'm', INT, "MaxMismatch", "0"},
      {"hide-matched", 'M', BOOL, "HideMatched", "false"}, {"circular", 'c', BOOL, "Circular", "false"}}},
    {"subseq", "SubseqTransform",
     {{"chr", 0, SLICE, "Chr", ""}, {"region", 'r', STR, "Region", ""}, {"gtf", 0, STR, "Gtf", ""},
      {"feature", 0, SLICE, "Feature", ""}, {"up-stream", 'u', INT, "UpStream", "0"},
      {"down-stream", 'd', INT, "DownStream", "0"}, {"only-flank", 'f', BOOL, "OnlyFlank", "false"},
      {"bed", 0, STR, "Bed", ""}, {"gtf-tag", 0, STR, "GtfTag", "gene_id"}}},
    {"translate", "Translate",
     {{"transl-table", 'T', INT, "TranslTable", "1"}, {"frame", 'f', SLICE, "Frame", "1"},
      {"trim", 0, BOOL, "Trim", "false"}, {"clean", 0, BOOL, "Clean", "false"},
      {"allow-unknown-codon", 'x', BOOL, "AllowUnknownCodon", "false"}, {"init-codon-as-M", 'M', BOOL, "InitCodonAsM", "false"},
      {"list-transl-table", 'l', INT, "ListTranslTable", "-1"},
      {"list-transl-table-with-amb-codons", 'L', INT, "ListTranslTableWithAmbCodons", "-1"},
      {"append-frame", 'F', BOOL, "AppendFrame", "false"}}},
    {"fq2fa", "Fq2Fa", {}},                                                          // cli/fq2fa.go:27
    {"range", "Range", {{"range", 'r', STR, "Range", ""}}},                            // cli/range.go:48
    {"head", "Head", {{"number", 'n', INT, "N", "10"}}},                               // cli/head.go:40
    {"duplicate", "Duplicate", {{"times", 'n', INT, "Times", "1"}}},                   // cli/duplicate.go:28-40 (alias dup)
    {"concat", "Concat", {{"full", 'f', BOOL, "Full", "false"}, {"separator", 's', STR, "Separator", "|"}}},   // cli/concat.go:51-52
    {"common", "Common",                                                               // cli/common.go:52-56
     {{"by-name", 'n', BOOL, "ByName", "false"}, {"by-seq", 's', BOOL, "BySeq", "false"},
      {"ignore-case", 'i', BOOL, "IgnoreCase", "false"}, {"only-positive-strand", 'P', BOOL, "OnlyPositiveStrand", "false"}}},
    {"pair", "Pair",                                                                   // cli/pair.go (flags of its init())
     {{"read1", '1', STR, "", ""}, {"read2", '2', STR, "", ""}, {"out-dir", 'O', STR, "", ""}, {"force", 'f', BOOL, "", "false"},
      {"save-unpaired", 'u', BOOL, "SaveUnpaired", "false"}}},
    {"rename", "Rename", {{"by-name", 'n', BOOL, "ByName", "false"}}},                  // cli/rename.go
    {"replace", "Replace",                                                             // cli/replace.go:70-83
     {{"pattern", 'p', STR, "Pattern", ""}, {"replacement", 'r', STR, "Replacement", ""},
      {"nr-width", 0, INT, "NrWidth", "1"}, {"by-seq", 's', BOOL, "BySeq", "false"},
      {"ignore-case", 'i', BOOL, "IgnoreCase", "false"}, {"kv-file", 'k', STR, "KvFile", ""},
      {"keep-untouch", 'U', BOOL, "KeepUntouch", "false"}, {"keep-key", 'K', BOOL, "KeepKey", "false"},
      {"key-capt-idx", 'I', INT, "KeyCaptIdx", "1"}, {"key-miss-repl", 'm', STR, "KeyMissRepl", ""}}},
    {"fa2fq", "Fa2Fq",                                                                 // cli/fa2fq.go:28-49
     {{"fasta-file", 'f', STR, "FastaFile", ""}, {"only-positive-strand", 'P', BOOL, "OnlyPositiveStrand", "false"}},
     "retrieve corresponding FASTQ records by a FASTA file\n"
     "Attention:\n"
     "  1. We assume the FASTA file comes from the FASTQ file,\n"
     "     so they share sequence IDs, and sequences in FASTA\n"
     "     should be subseq of sequences in FASTQ file.\n"
     "\n"
     "Usage:\n"
     "  bigseqkit fa2fq [flags]\n"
     "\n"
     "Flags:\n"
     "  -f, --fasta-file string      FASTA file)\n"
     "  -h, --help                   help for fa2fq\n"
     "  -P, --only-positive-strand   only search on positive strand\n"},
    {"faidx", "Faidx",                                                                 // cli/faidx.go:68-72
     {{"use-regexp", 'r', BOOL, "UseRegexp", "false"}, {"ignore-case", 'i', BOOL, "IgnoreCase", "false"},
      {"full-head", 'f', BOOL, "FullHead", "false"}, {"region-file", 'l', STR, "RegionFile", ""},
      {"index-file", 'd', STR, "", ""}}},
    {"sort", "Sort",                                                                   // cli/sort.go:50-61
     {{"natural-order", 'N', BOOL, "InNaturalOrder", "false"}, {"by-name", 'n', BOOL, "ByName", "false"},
      {"by-seq", 's', BOOL, "BySeq", "false"}, {"by-length", 'l', BOOL, "ByLength", "false"},
      {"by-bases", 'b', BOOL, "ByBases", "false"}, {"gap-letters", 'G', STR, "GapLetters", "- \t."},
      {"reverse", 'r', BOOL, "Reverse", "false"}, {"ignore-case", 'i', BOOL, "IgnoreCase", "false"},
      {"two-pass", '2', BOOL, "", "false"}, {"keep-temp", 'k', BOOL, "", "false"},
      {"seq-prefix-length", 'L', INT, "SeqPrefixLength", "10000"}}},
    {"sample", "Sample",                                                               // cli/sample.go:43-46
     {{"rand-seed", 's', INT, "Seed", "11"}, {"number", 'n', INT, "Number", "0"}, {"proportion", 'p', FLOAT, "Proportion", "0"},
      {"two-pass", '2', BOOL, "", "false"}}},
    {"shuffle", "Shuffle",                                                             // cli/shuffle.go:44-46
     {{"rand-seed", 's', INT, "Seed", "23"}, {"two-pass", '2', BOOL, "", "false"}, {"keep-temp", 'k', BOOL, "", "false"}}},
    {"head-genome", "HeadGenome", {{"mini-common-words", 'm', INT, "MiniCommonWords", "1"}},          // cli/head_genome.go:25-53
     "print sequences of the first genome with common prefixes in name\n"
     "For a FASTA file containing multiple contigs of strains (see example below),\n"
     "these's no list of IDs available for retrieving sequences of a certain strain,\n"
     "while descriptions of each strain share the same prefix.\n"
     "This command is used to restrieve sequences of the first strain,\n"
     "i.e., \"Vibrio cholerae strain M29\".\n"
     ">NZ_JFGR01000001.1 Vibrio cholerae strain M29 Contig_1, whole genome shotgun sequence\n"
     ">NZ_JFGR01000002.1 Vibrio cholerae strain M29 Contig_2, whole genome shotgun sequence\n"
     ">NZ_JFGR01000003.1 Vibrio cholerae strain M29 Contig_3, whole genome shotgun sequence\n"
     ">NZ_JSTP01000001.1 Vibrio cholerae strain 2012HC-12 NODE_79, whole genome shotgun sequence\n"
     ">NZ_JSTP01000002.1 Vibrio cholerae strain 2012HC-12 NODE_78, whole genome shotgun sequence\n"
     "Attention:\n"
     "  1. Sequences in file should be well organized.\n"
     "\n"
     "Usage:\n"
     "  bigseqkit head-genome [flags]\n"
     "\n"
     "Flags:\n"
     "  -h, --help                    help for head-genome\n"
     "  -m, --mini-common-words int   minimal shared prefix words (default 1)\n"},
    {"rmdup", "RmDup",
     {{"by-name", 'n', BOOL, "ByName", "false"}, {"by-seq", 's', BOOL, "BySeq", "false"},
      {"ignore-case", 'i', BOOL, "IgnoreCase", "false"}, {"dup-seqs-file", 'd', STR, "DupSeqsFile", ""},
      {"dup-num-file", 'D', STR, "DupNumFile", ""}, {"only-positive-strand", 'P', BOOL, "OnlyPositiveStrand", "false"}}},
};

// The process ends here, without atexit handlers / static destructors: everything the command wrote is flushed and closed
// by then, and the teardown of the HIP runtime at exit() is not ours to wait for -- it took one CLI run in ~200 down with
// SIGSEGV after the output was complete (tests/test_cli.py on the MI355X box, round 3).
[[noreturn]] void leave(int rc) {
    std::cout.flush();
    std::cerr.flush();
    fflush(nullptr);
    _exit(rc);
}

[[noreturn]] void die(const std::string& m) {
    std::cerr << "Error: " << m << "\n";
    leave(1);
}

std::string jquote(const std::string& s) {
    std::string o = "\"";
    char b[8];
    for (unsigned char c : s) {
        if (c == '"') o += "\\\"";
        else if (c == '\\') o += "\\\\";
        else if (c == '\n') o += "\\n";
        else if (c == '\t') o += "\\t";
        else if (c < 0x20 || c == '<' || c == '>' || c == '&') { snprintf(b, sizeof b, "\\u%04x", c); o += b; }
        else o.push_back((char)c);
    }
    return o + "\"";
}

// pflag StringSlice: comma separated, double quotes protect commas
std::vector<std::string> split_csv(const std::string& v) {
    std::vector<std::string> out;
    std::string cur;
    bool q = false;
    for (size_t i = 0; i < v.size(); ++i) {
        char c = v[i];
        if (c == '"') {
            if (q && i + 1 < v.size() && v[i + 1] == '"') { cur.push_back('"'); ++i; }
            else q = !q;
        } else if (c == ',' && !q) { out.push_back(cur); cur.clear(); }
        else cur.push_back(c);
    }
    out.push_back(cur);
    return out;
}

struct Values {
    std::map<std::string, std::string> scalar;            // flag name -> text
    std::map<std::string, std::vector<std::string>> slice;  // flag name -> values (only when given)
};

const Flag* find_flag(const Command& c, const std::string& name, char sh) {
    for (auto& f : c.flags)
        if ((!name.empty() && name == f.name) || (sh && sh == f.shorthand)) return &f;
    for (auto& f : kPersistent)
        if ((!name.empty() && name == f.name) || (sh && sh == f.shorthand)) return &f;
    return nullptr;
}

bool file_exists(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0; }
bool is_dir(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode); }

bool has_suffix(std::string s, const std::vector<const char*>& es) {
    for (auto& c : s) c = (char)tolower((unsigned char)c);
    for (auto e : es) {
        size_t n = strlen(e);
        if (s.size() >= n && s.compare(s.size() - n, n, e) == 0) return true;
    }
    return false;
}

std::string read_file(const std::string& path) {
    // (one read() loop into the string: the stream-buffer copy this replaced moved a file of 8 GB twice)
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) die("open " + path + ": no such file or directory");
    struct stat sb;
    std::string text;
    if (fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode)) {
        text.resize((size_t)sb.st_size);
        size_t done = 0;
        while (done < text.size()) {
            const ssize_t got = read(fd, &text[done], std::min<size_t>(text.size() - done, (size_t)256 << 20));
            if (got < 0 && errno == EINTR) continue;
            if (got <= 0) break;
            done += (size_t)got;
        }
        text.resize(done);
    } else {  // a pipe, a character device: until it ends
        char buf[1 << 16];
        for (;;) {
            const ssize_t got = read(fd, buf, sizeof buf);
            if (got < 0 && errno == EINTR) continue;
            if (got <= 0) break;
            text.append(buf, (size_t)got);
        }
    }
    close(fd);
    return text;
}

// bigseqkit-cli/helper.go:63-78; `data` is the TEXT of the file -- of a compressed file (PARITY.md BGZF) what it inflates to --
// and the suffix rule looks under a trailing .gz / .bgz
int sniff_format(const std::string& file_, const std::string& data) {
    std::string file = file_;
    for (const char* z : {".gz", ".bgz"})
        if (has_suffix(file, {z})) { file.resize(file.size() - strlen(z)); break; }
    if (has_suffix(file, {".fa", ".fna", ".ffn", ".faa", ".frn"})) return BSK_FORMAT_FASTA;
    if (has_suffix(file, {".fq", ".fastq"})) return BSK_FORMAT_FASTQ;
    if (!data.empty() && data[0] == '>') return BSK_FORMAT_FASTA;
    if (!data.empty() && data[0] == '@') return BSK_FORMAT_FASTQ;
    die(" <file> must be fasta or fastq");
}

// ---- compressed input (PARITY.md BGZF, GZIP): BGZF is inflated, on the device where the part lives there; any other gzip is
// refused unless BSK_GZIP=1 asks for it: then it is read wherever a BGZF file is read whole (bsk_gzip_load on the device, the same
// method on the host for the commands that keep host strings).  The paths that read a file in pieces refuse it -- unless
// BSK_GZIP_STREAM=1 is set as well: then `stats` on a file that is not read whole and the bucket paths read it through the
// segment reader (bsk_gzip_reader_*), which re-enters the stream at the block starts it has recorded; its positions are text
// offsets.  Without that switch every exit status and every byte of stderr is as before.
// The paths for inputs that are not loaded whole read a BGZF file in pieces (bsk_bgzf_reader_*) only when asked to:
// BSK_BGZF_STREAM=1.  Every pass over the input inflates the file again -- a bucket command reads it 2 + B times and more --, which
// a user should choose knowingly; without the switch these paths refuse a compressed file as before, and the message names it.
// --devices reads a BGZF file only under BSK_BGZF_DEVICES=1: the file is cut at block starts found near size * k / world and at
// the record starts behind them (bsk_bgzf_cut_points), every worker inflates its own blocks (bsk_bgzf_shard_load), and a cut
// that fell on bytes that only look like a block is refused by the worker whose chain steps over it, before anything is written

// One input file of an invocation, looked at once (classify_inputs): the record goes to whoever opens the file.  kind is what
// bsk_bgzf_probe says of its first bytes; a pipe is plain here: it is looked at once it has been read
enum InputKind { kPlain = 0, kBgzf = 1, kGzip = 2 };
struct Input {
    std::string path;
    int kind = kPlain;
    bool regular = false, missing = false;
    size_t size = 0;
};
std::vector<Input> classify_inputs(const std::vector<std::string>& files) {
    std::vector<Input> ins;
    for (auto& path : files) {
        Input in;
        in.path = path;
        const int fd = open(path.c_str(), O_RDONLY);
        in.missing = fd < 0;  // (said by admit, or by whoever opens the file)
        struct stat sb;
        if (fd >= 0 && fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode)) {
            in.regular = true;
            in.size = (size_t)sb.st_size;
            std::string head((size_t)12 + 65535, '\0');
            const ssize_t got = pread(fd, &head[0], head.size(), 0);
            if (got > 0) in.kind = bsk_bgzf_probe(head.data(), (size_t)got);
        }
        if (fd >= 0) close(fd);
        ins.push_back(std::move(in));
    }
    return ins;
}

// files of at least this many bytes do not go to the GPU as one shard: `stats` streams them from the host, the other
// commands say what to do.  BSK_HOST_PIPELINE_FROM moves the line (tests: 0)
static size_t whole_file_limit() {
    size_t lim = (size_t)200 << 30;  // (288 GB of HBM: the shard, the stats vector and nothing else)
    if (const char* e = getenv("BSK_HOST_PIPELINE_FROM")) lim = (size_t)strtoull(e, nullptr, 10);
    return lim;
}
static bool stats_streams(const std::string& use, size_t size) { return use == "stats" && size > 0 && size >= whole_file_limit(); }

// THE admission rule: which kind of input a route takes under which switch, and what a refusal says.
//   Any       every invocation on one device, before a device is touched
//   HostText  the text of a file or a pipe on the host, inflated there (inflate_host_text)
//   Device    a file that goes to the GPU whole (read_parts), or -- `stats` on a file that does not fit -- is streamed
//   Buckets   the bucket paths (run_buckets), which read a file in pieces
//   Devices   --devices, which cuts a file by its bytes -- and a BGZF file by its blocks, when BSK_BGZF_DEVICES=1 asks for it
// Returns whether a BGZF file may be read in pieces (BSK_BGZF_STREAM=1), and in *gzip_pieces whether a plain gzip file may
// (BSK_GZIP=1 BSK_GZIP_STREAM=1: read here and nowhere else); the refusals of plain gzip come first, over all files
enum class Route { Any, HostText, Device, Buckets, Devices };
bool admit(const std::vector<Input>& ins, Route route, const std::string& use = "", bool* gzip_pieces = nullptr) {
    static const char* const kPlainGzip = " is gzip but not BGZF: one gzip stream cannot be cut into independent blocks, so it is not read; "
                                          "recompress it with bgzip (gzip -dc FILE | bgzip > FILE.gz) or decompress it first, or set BSK_GZIP=1 "
                                          "to have it inflated whole, in speculative chunks, where the file and its text fit one GPU";
    static const char* const kStreamHint = ", or set BSK_BGZF_STREAM=1 to read it in record-aligned pieces, inflated once per pass";
    auto switch_on = [](const char* name) { const char* e = getenv(name); return e && *e && strcmp(e, "0") != 0; };
    const bool gzip = switch_on("BSK_GZIP"), pieces = switch_on("BSK_BGZF_STREAM"), segments = gzip && switch_on("BSK_GZIP_STREAM");
    const bool shards = switch_on("BSK_BGZF_DEVICES");  // (a BGZF file under --devices: block-aligned cuts, a shard per worker)
    if (gzip_pieces) *gzip_pieces = segments;
    // the routes that read a file by its bytes or in pieces: what they do, and what to do about a BGZF file instead
    std::string gzip_where, bgzf_where, instead;
    if (route == Route::Device) {
        gzip_where = "'stats' streams";
        bgzf_where = "'stats' streams a file that does not fit one GPU";
        instead = std::string("decompress it first (bgzip -d), or cut it into files that fit") + kStreamHint;
    } else if (route == Route::Buckets) {
        gzip_where = bgzf_where = "the buckets of '" + use + "' read";
        instead = std::string("decompress it first (bgzip -d), or unset the budget if the file and its text fit one GPU") + kStreamHint;
    } else if (route == Route::Devices) {
        gzip_where = bgzf_where = "--devices cuts";
        instead = "run it on one device (--device N), or decompress it first (bgzip -d)";
    }
    auto by_bytes = [&](const Input& in) { return route == Route::Buckets || route == Route::Devices || (route == Route::Device && stats_streams(use, in.size)); };
    for (auto& in : ins) {
        if (in.missing && (route != Route::Any || !gzip)) die("open " + in.path + ": no such file or directory");
        if (in.kind != kGzip) continue;
        if (!gzip) die(in.path + kPlainGzip);  // (read by no path without the switch)
        if (by_bytes(in) && segments && route == Route::Devices)
            die(in.path + " is gzip but not BGZF, and --devices cuts a file by its bytes: where a worker starts in a gzip stream is known only after a pass over "
                "the stream in front of it, so BSK_GZIP_STREAM=1 reads it in pieces on one device only; run it on one device (--device N), or decompress it first (gzip -d)");
        if (by_bytes(in) && !segments)
            die(in.path + " is gzip but not BGZF, and " + gzip_where + " a file in pieces: a gzip stream has no virtual offsets to re-enter at, so BSK_GZIP=1 "
                "reads it only where a file is read whole; decompress it first (gzip -d), or recompress it with bgzip (gzip -dc FILE | bgzip > FILE.gz)");
    }
    for (auto& in : ins)
        if (in.kind == kBgzf && by_bytes(in) && !(route == Route::Devices ? shards : pieces))
            die(in.path + " is BGZF-compressed, and " + bgzf_where + " a file by its bytes, which a compressed file does not allow yet; " + instead);
    return pieces;
}

// the double call of an inflate entry point: call(nullptr, 0, &n) says how many bytes the text has, call(buf, n, &n) brings them
template <class Call>
bool size_then_fill(std::string& out, Call call) {
    size_t n = 0;
    if (call(nullptr, 0, &n) != BSK_OK) return false;
    out.assign(n, '\0');
    return n == 0 || call(&out[0], n, &n) == BSK_OK;
}

// The first byte of a BGZF file's text (0: it has none): the blocks are walked by their BSIZE, and the first one that holds text is
// inflated on the host -- what sniff_format asks of a file that is not read whole
char bgzf_first_text_byte(const std::string& path) {
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) die("open " + path + ": no such file or directory");
    std::string blk((size_t)12 + 65535 + 65536, '\0');
    char first = 0;
    for (off_t off = 0;;) {
        const ssize_t got = pread(fd, &blk[0], blk.size(), off);
        if (got < 18) break;
        const uint8_t* b = (const uint8_t*)blk.data();
        const size_t xlen = b[10] | (size_t)b[11] << 8;
        size_t bsize = 0;
        for (size_t at = 12; at + 4 <= 12 + xlen && at + 6 <= (size_t)got;) {
            const size_t slen = b[at + 2] | (size_t)b[at + 3] << 8;
            if (b[at] == 'B' && b[at + 1] == 'C' && slen == 2) { bsize = (b[at + 4] | (size_t)b[at + 5] << 8) + 1; break; }
            at += 4 + slen;
        }
        if (bsize == 0 || bsize > (size_t)got) break;  // (not a whole block: the reader will say what is wrong with the file)
        std::string text;
        if (!size_then_fill(text, [&](char* buf, size_t cap, size_t* n) { return bsk_bgzf_inflate_host(b, bsize, buf, cap, n, 1); })) break;
        if (!text.empty()) {
            first = text[0];
            break;
        }
        off += (off_t)bsize;
    }
    close(fd);
    return first;
}

// the sizes of the BGZF piece reader (bsk_bgzf_reader_open; 0: its defaults).  The tests pin them
struct BgzfSizes { size_t piece, look, chunk; };
BgzfSizes bgzf_sizes() {
    auto env = [](const char* name) { const char* e = getenv(name); return e ? (size_t)strtoull(e, nullptr, 10) : (size_t)0; };
    return {env("BSK_STREAM_PIECE_BYTES"), env("BSK_BGZF_LOOKAHEAD_BYTES"), env("BSK_BGZF_CHUNK_BYTES")};
}

// the sizes of the gzip segment reader (bsk_gzip_reader_open; 0: its defaults)
struct GzipSizes { size_t piece, look, segment, chunk; };
GzipSizes gzip_sizes() {
    auto env = [](const char* name) { const char* e = getenv(name); return e ? (size_t)strtoull(e, nullptr, 10) : (size_t)0; };
    return {env("BSK_STREAM_PIECE_BYTES"), env("BSK_GZIP_LOOKAHEAD_BYTES"), env("BSK_GZIP_SEGMENT_BYTES"), env("BSK_GZIP_CHUNK_BYTES")};
}

// The first byte of a gzip file's text (0: it has none): the reader on the host, in small segments, asked for one byte -- what
// sniff_format asks of a file that is not read whole
char gzip_first_text_byte(const std::string& path) {
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) die("open " + path + ": no such file or directory");
    bsk_gzip_reader* rd = nullptr;
    if (bsk_gzip_reader_open(fd, -1, BSK_FORMAT_FASTA, 1, 1, (size_t)64 << 10, (size_t)16 << 10, &rd) != BSK_OK) die(path + ": " + bsk_global_error());
    const void* p = nullptr;
    size_t n = 0;
    char first = 0;
    if (bsk_gzip_reader_piece(rd, 0, 1, &p, &n) == BSK_OK && n == 1) first = *(const char*)p;  // (an empty text, or a bad file: the pass over it says so)
    bsk_gzip_reader_close(rd);
    close(fd);
    return first;
}

// `text` as read from a file or a pipe: inflated in place when it is compressed -- BGZF on host threads with the decoder of the
// device, plain gzip by the speculative method with one host lane, in one piece
void inflate_host_text(const std::string& path, std::string& text) {
    Input in;
    in.path = path;
    in.kind = bsk_bgzf_probe(text.data(), text.size());
    if (in.kind == kPlain) return;
    admit({in}, Route::HostText);
    std::string out;
    const bool ok = size_then_fill(out, [&](char* buf, size_t cap, size_t* n) {
        return in.kind == kGzip ? bsk_gzip_inflate_host(text.data(), text.size(), buf, cap, n, 0) : bsk_bgzf_inflate_host(text.data(), text.size(), buf, cap, n, 0);
    });
    if (!ok) die(path + ": " + bsk_global_error());
    text.swap(out);
}

// ---- compressed output (PARITY.md BGZFW).  THE rule: an -o name that ends in .gz / .bgz makes every file written under it BGZF
// ("-" and the default <input>-out do not end so: plain).  It is decided here and nowhere else; the writers below share it.
bool name_is_bgzf(const std::string& out_name) { return has_suffix(out_name, {".gz", ".bgz"}); }
const char* part_suffix(bool bgzf) { return bgzf ? ".gz" : ""; }
std::string eof_block() {
    std::string e(28, '\0');
    size_t n = 0;
    if (bsk_bgzf_deflate_host(nullptr, 0, 0, 1, &e[0], e.size(), &n, 1) != BSK_OK || n != e.size()) die(bsk_global_error());
    return e;
}
// the result of a run joins `text`: as it is, or -- pack -- as BGZF without an EOF block, compressed on the context's device so
// that only the compressed bytes cross to the host (a share or a piece ends on a block: the pieces and one EOF block are a file)
void append_result(bsk_ctx* c, const bsk_out& out, std::string& text, bool pack) {
    if (!out.len) return;
    const size_t at = text.size();
    if (!pack) {
        text.resize(at + out.len);
        if (bsk_out_to_host(c, &out, &text[at], out.len) != BSK_OK) die(bsk_last_error(c));
        return;
    }
    const size_t cap = bsk_bgzf_deflate_bound(out.len, 0);
    size_t got = 0;
    text.resize(at + cap);
    if (bsk_out_to_host_bgzf(c, &out, 0, &text[at], cap, &got) != BSK_OK) die(bsk_last_error(c));
    text.resize(at + got);
}
// host text as BGZF without an EOF block, on host threads (the bytes the device writes): the rare paths that hold the text on
// the host -- part files cut at record starts, the commands that join their inputs there
std::string deflate_host_text(const char* p, size_t n) {
    std::string comp(bsk_bgzf_deflate_bound(n, 0), '\0');
    size_t got = 0;
    if (bsk_bgzf_deflate_host(p, n, 0, 0, &comp[0], comp.size(), &got, 0) != BSK_OK) die(bsk_global_error());
    comp.resize(got);
    return comp;
}
// one file of the output: [p, p + n) is text, or -- packed -- BGZF already; a BGZF file ends with the EOF block
void write_out_file(const std::string& path, bool bgzf, bool packed, const char* p, size_t n) {
    std::ofstream f(path, std::ios::binary);
    if (!f) die("cannot create " + path);
    if (bgzf && !packed) {
        const std::string comp = deflate_host_text(p, n);
        f.write(comp.data(), (std::streamsize)comp.size());
    } else {
        f.write(p, (std::streamsize)n);
    }
    if (bgzf) f.write(eof_block().data(), 28);
    f.close();  // (die() ends the process without destructors: nothing may still sit in a stream buffer by then)
    if (!f) die("write " + path + " failed");
}

void usage() {
    std::cout << "bigseqkit -- MI355X-native seqkit-compatible commands (libbsk)\n\nUsage:\n  bigseqkit <command> [flags] files...\n\nCommands:\n";
    for (auto& c : kCommands) std::cout << "  " << c.use << "\n";
    std::cout << "\nGlobal flags: -t/--seq-type -w/--line-width --id-regexp --id-ncbi -o/--out-file --quiet\n"
                 "  --alphabet-guess-seq-length --infile-list --merge --partitions --order --device --dry-run\n"
                 "faidx FILE REGION... -d IDX: with IDX present the regions are fetched through it and FILE is not loaded (plain, or BGZF\n"
                 "  with its block table FILE.gzi, built where absent; the bytes are checked against the index); with IDX absent the run is the whole-file run and writes the index rows to IDX.\n"
                 "An -o name that ends in .gz or .bgz is written as BGZF (what bgzip writes), compressed on the GPU; any other name is plain text.\n";
}

// one parsed command line: `args[0]` is the command, the rest flags and input files
struct Invocation {
    const Command* cmd = nullptr;
    Values val;
    std::vector<std::string> files;
    std::string js;  // option JSON of the operator
    std::string pget(const char* name) const {
        auto it = val.scalar.find(name);
        if (it != val.scalar.end()) return it->second;
        for (auto& f : kPersistent)
            if (!strcmp(f.name, name)) return f.def;
        if (cmd)
            for (auto& f : cmd->flags)
                if (!strcmp(f.name, name)) return f.def;
        return "";
    }
};

Invocation parse_invocation(const std::vector<std::string>& args) {
    Invocation inv;
    const int argc = (int)args.size();
    auto argv = [&](int i) -> const std::string& { return args[(size_t)i]; };
    for (auto& c : kCommands)
        if (args[0] == c.use || (args[0] == "dup" && !strcmp(c.use, "duplicate"))) inv.cmd = &c;
    if (!inv.cmd) die(std::string("unknown command \"") + args[0] + "\" for \"bigseqkit\"");
    const Command* cmd = inv.cmd;
    Values& val = inv.val;
    std::vector<std::string>& files = inv.files;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv(i);
        if (a == "--") { for (int k = i + 1; k < argc; ++k) files.push_back(argv(k)); break; }
        if (a.size() < 2 || a[0] != '-' || a == "-") { files.push_back(a); continue; }
        if (cmd->help && (a == "-h" || a == "--help")) { std::cout << cmd->help; exit(0); }
        std::vector<std::pair<const Flag*, std::string>> parsed;  // flag, inline value ("\x01" = none)
        if (a[1] == '-') {
            std::string name = a.substr(2), v = "\x01";
            size_t eq = name.find('=');
            if (eq != std::string::npos) { v = name.substr(eq + 1); name = name.substr(0, eq); }
            const Flag* f = find_flag(*cmd, name, 0);
            if (!f) die("unknown flag: --" + name);
            parsed.push_back({f, v});
        } else {
            for (size_t k = 1; k < a.size(); ++k) {
                const Flag* f = find_flag(*cmd, "", a[k]);
                if (!f) die(std::string("unknown shorthand flag: '") + a[k] + "' in " + a);
                if (f->kind != BOOL && k + 1 < a.size()) {  // -p=ACGT or -pACGT
                    std::string v = a.substr(k + 1);
                    if (!v.empty() && v[0] == '=') v.erase(0, 1);
                    parsed.push_back({f, v});
                    break;
                }
                parsed.push_back({f, "\x01"});
            }
        }
        for (auto& pr : parsed) {
            const Flag* f = pr.first;
            std::string v = pr.second;
            if (f->kind == BOOL) {
                if (v == "\x01") v = "true";
                if (v != "true" && v != "false") die(std::string("invalid argument \"") + v + "\" for \"--" + f->name + "\" flag");
                val.scalar[f->name] = v;
                continue;
            }
            if (v == "\x01") {
                if (i + 1 >= argc) die(std::string("flag needs an argument: --") + f->name);
                v = argv(++i);
            }
            if (f->kind == SLICE) {
                auto parts = split_csv(v);
                auto& dst = val.slice[f->name];
                dst.insert(dst.end(), parts.begin(), parts.end());
            } else {
                if (f->kind == INT) {
                    char* e = nullptr;
                    strtol(v.c_str(), &e, 10);
                    if (v.empty() || *e) die(std::string("invalid argument \"") + v + "\" for \"--" + f->name + "\" flag");
                }
                if (f->kind == FLOAT) {
                    char* e = nullptr;
                    strtod(v.c_str(), &e);
                    if (v.empty() || *e) die(std::string("invalid argument \"") + v + "\" for \"--" + f->name + "\" flag");
                }
                val.scalar[f->name] = v;
            }
        }
    }
    auto get = [&](const char* name, const Flag* table, size_t n) -> std::string {
        auto it = val.scalar.find(name);
        if (it != val.scalar.end()) return it->second;
        for (size_t k = 0; k < n; ++k)
            if (!strcmp(table[k].name, name)) return table[k].def;
        return "";
    };
    auto pget = [&](const char* name) { return get(name, kPersistent, sizeof(kPersistent) / sizeof(Flag)); };

    // getFlagPositiveInt / getFlagNonNegativeInt (bigseqkit-cli/helper.go:248-265), message as written
    for (const char* nm : {"line-width", "max-mismatch", "up-stream", "down-stream", "validate-seq-length", "alphabet-guess-seq-length",
                           "qual-ascii-base", "transl-table", "mini-common-words"}) {
        const Flag* f = find_flag(*cmd, nm, 0);
        if (!f) continue;
        auto it = val.scalar.find(nm);
        long v = strtol((it != val.scalar.end() ? it->second : std::string(f->def)).c_str(), nullptr, 10);
        const bool positive = !strcmp(nm, "qual-ascii-base") || !strcmp(nm, "transl-table") || !strcmp(nm, "mini-common-words");
        if (positive ? v <= 0 : v < 0) die(std::string("value of flag --") + nm + " should be greater than 0");
        if (!strcmp(nm, "validate-seq-length") && v > 0 && v < 1000)
            die("value of flag --validate-seq-length too small, should >= 1000");
    }
    // getIDRegexp (helper.go:297-309)
    if (val.scalar.count("id-ncbi") && val.scalar["id-ncbi"] == "true") val.scalar["id-regexp"] = "\\|([^\\|]+)\\| ";
    // bigseqkit-cli/helper.go:332-338
    {
        long g = strtol(pget("alphabet-guess-seq-length").c_str(), nullptr, 10);
        if (g > 0 && g < 1000) die("value of flag --alphabet-guess-seq-length too small, should >= 1000");
    }

    // ---- option JSON (schema of bigseqkit.OptionsToString).  Like the reference's parseSeqKit*Options,
    // every field carries the flag's value, i.e. the CLI default when the flag was not given.
    auto emit_field = [&](std::string& js, const Flag& f, const char* field) {
        js += jquote(field);
        js += ":";
        if (f.kind == SLICE) {
            auto it = val.slice.find(f.name);
            std::vector<std::string> v = it != val.slice.end() ? it->second : (*f.def ? split_csv(f.def) : std::vector<std::string>());
            js += "[";
            for (size_t k = 0; k < v.size(); ++k) js += (k ? "," : "") + jquote(v[k]);
            js += "]";
            return;
        }
        auto it = val.scalar.find(f.name);
        const std::string v = it != val.scalar.end() ? it->second : std::string(f.def);
        if (f.kind == STR) js += jquote(v);
        else js += v;
    };
    std::string& js = inv.js;
    js = "{\"Config\":{";
    bool first = true;
    for (auto& f : kPersistent) {
        if (strncmp(f.field, "Config.", 7)) continue;
        if (!first) js += ",";
        first = false;
        emit_field(js, f, f.field + 7);
    }
    js += "}";
    for (auto& f : cmd->flags) {
        if (!*f.field) continue;
        js += ",";
        emit_field(js, f, f.field);
    }
    js += "}";

    // input files (+ --infile-list, one per line)
    {
        std::string lst = pget("infile-list");
        if (!lst.empty()) {
            std::istringstream ss(read_file(lst));
            std::string line;
            while (std::getline(ss, line))
                if (!line.empty()) files.push_back(line);
        }
    }
    return inv;
}

// ---------------------------------------------------------------------------
// execution: inputs are PARTS (the reference's dataframe partitions): the text of a file on the host, or the
// device-resident output of an upstream command of a `pipe` job (it never leaves HBM)
// ---------------------------------------------------------------------------
struct Part {
    int fmt = BSK_FORMAT_FASTA;
    std::string host;        // file text (when dptr == nullptr)
    void* dptr = nullptr;    // device text of `n` bytes
    size_t n = 0;
    bsk_ctx* owner = nullptr;  // context whose output buffer dptr is (destroyed with the part)
    bool owned_alloc = false;  // dptr came from bsk_device_alloc
    // a file that does not fit the GPU (round 6; the reference takes any file size through its partitions,
    // bigseqkit/helper.go:148-178): its read-only mapping -- `stats` streams it through the library's double-buffered
    // host-shard path (bsk_stats_run with on_device = 0: record-aligned 256 MiB chunks, H2D of chunk i + 1 under the kernels of i)
    const void* map = nullptr;
    size_t map_n = 0;
    // ... and a BGZF file of that size: the open file, which `stats` reads through the piece reader (bsk_bgzf_reader_*: the text
    // arrives in record-aligned pieces on the device, the file is never held whole)
    int bgzf_fd = -1;
    // ... and a plain gzip file of that size (BSK_GZIP_STREAM=1): the segment reader (bsk_gzip_reader_*), in the same way
    int gzip_fd = -1;
    const void* ptr() const { return dptr ? dptr : (map ? map : (const void*)host.data()); }
    size_t size() const { return dptr ? n : (map ? map_n : host.size()); }
    int on_device() const { return dptr ? 1 : 0; }
};

void release(std::vector<Part>& parts) {
    for (auto& p : parts) {
        if (p.owner) bsk_destroy(p.owner);
        else if (p.owned_alloc && p.dptr) bsk_device_free(p.dptr);
        if (p.map) munmap(const_cast<void*>(p.map), p.map_n);
        if (p.bgzf_fd >= 0) close(p.bgzf_fd);
        if (p.gzip_fd >= 0) close(p.gzip_fd);
        p.owner = nullptr; p.dptr = nullptr; p.map = nullptr; p.bgzf_fd = p.gzip_fd = -1;
    }
    parts.clear();
}

struct Output {
    std::vector<Part> parts;  // FASTA / FASTQ records (device-resident when keep_on_device)
    std::string text;         // everything else: stats table, grep -C count, locate rows, or the host copy of the records
    bool is_text = false;     // `text` is the result (not record text)
    int fmt = -1;             // format of the record text in `text` (-1: line oriented)
    bool stored = false;      // the result has been written already, share by share (run_buckets, concat): store() is not called
    bool packed = false;      // `text` is BGZF without its EOF block (append_result with pack): store() writes it as it comes
};

bool g_pipe_job = false;  // the jobs of a `pipe` run: their results stay text, `pipe` itself stores (and compresses) the last one
bool out_is_bgzf(const Invocation& inv) { return name_is_bgzf(inv.pget("out-file")); }
// the result goes to ONE compressed file: it can leave the device compressed.  (Several part files are cut from the host text at
// record starts, as ever, and each is compressed on host threads: rare.)
bool packs_on_device(const Invocation& inv) {
    return !g_pipe_job && out_is_bgzf(inv) && (inv.pget("merge") == "true" || strtol(inv.pget("partitions").c_str(), nullptr, 10) <= 1);
}

bool g_faidx_query = false;  // `faidx` with regions: records out, not index rows

int run_op(const std::string& use, bsk_ctx* ctx, const Part& in, int64_t pid, uint64_t first_record, bsk_out* out) {
    const void* p = in.ptr();
    const size_t n = in.size();
    const int dev = in.on_device();
    if (use == "seq") return bsk_seq_run(ctx, p, n, dev, in.fmt, pid, nullptr, out);
    if (use == "grep") return bsk_grep_run(ctx, p, n, dev, in.fmt, pid, nullptr, out);
    if (use == "locate") return bsk_locate_run(ctx, p, n, dev, in.fmt, pid, nullptr, out);
    if (use == "subseq") return bsk_subseq_run(ctx, p, n, dev, in.fmt, pid, nullptr, out);
    if (use == "translate") return bsk_translate_run(ctx, p, n, dev, in.fmt, pid, nullptr, out);
    if (use == "fq2fa") return bsk_fq2fa_run(ctx, p, n, dev, in.fmt, pid, nullptr, out);
    if (use == "rename") return bsk_rename_run(ctx, p, n, dev, in.fmt, pid, nullptr, out);
    if (use == "replace") return bsk_replace_run(ctx, p, n, dev, in.fmt, pid, nullptr, out);
    if (use == "fa2fq") return bsk_fa2fq_run(ctx, p, n, dev, in.fmt, pid, nullptr, out);
    if (use == "sort") return bsk_sort_run(ctx, p, n, dev, in.fmt, pid, nullptr, out);
    if (use == "faidx" && g_faidx_query) return bsk_faidx_query_run(ctx, p, n, dev, in.fmt, pid, nullptr, out);
    if (use == "faidx") return bsk_faidx_run(ctx, p, n, dev, in.fmt, pid, first_record /* = byte offset here */, nullptr, out);
    if (use == "duplicate") return bsk_duplicate_run(ctx, p, n, dev, in.fmt, pid, nullptr, out);
    if (use == "range" || use == "head") return bsk_range_run(ctx, p, n, dev, in.fmt, pid, first_record, nullptr, out);
    if (use == "sample") return bsk_sample_run(ctx, p, n, dev, in.fmt, pid, first_record, nullptr, out);
    if (use == "shuffle") return bsk_shuffle_run(ctx, p, n, dev, in.fmt, pid, nullptr, out);
    if (use == "head-genome") {  // every input is a run of its own (cli/head_genome.go:11-15)
        bsk_head_genome_reset(ctx);
        return bsk_head_genome_run(ctx, p, n, dev, in.fmt, pid, nullptr, out);
    }
    return bsk_rmdup_run(ctx, p, n, dev, in.fmt, pid, nullptr, out);
}

// keep_on_device: the caller is an inner node of a pipe job; record outputs stay in HBM (one context per part)
Output execute(const Invocation& inv, std::vector<Part>& inputs, bool keep_on_device) {
    const std::string use = inv.cmd->use;
    const std::string& js = inv.js;
    const int device = (int)strtol(inv.pget("device").c_str(), nullptr, 10);
    Output res;
    // rmdup is global over the union of its inputs (bigseqkit/rmdup.go:97 groups the whole dataframe): one shard
    // (shuffle: the files of the command line are unioned, cli/shuffle.go:11-15, and the order is over all of them)
    if ((use == "rmdup" || use == "rename" || use == "sort" || use == "shuffle") && inputs.size() > 1) {
        size_t total = 0;
        for (auto& p : inputs) {
            if (p.fmt != inputs[0].fmt) die(use + ": inputs of different formats");
            total += p.size();
        }
        Part all;
        all.fmt = inputs[0].fmt;
        all.dptr = bsk_device_alloc(total + inputs.size() + 1);  // room for a newline after every part
        if (!all.dptr) die(bsk_global_error());
        all.owned_alloc = true;
        size_t at = 0;
        for (auto& p : inputs) {
            if (!p.size()) continue;
            if (bsk_device_copy((char*)all.dptr + at, p.ptr(), p.size(), p.on_device() ? BSK_COPY_D2D : BSK_COPY_H2D) != BSK_OK)
                die(bsk_global_error());
            at += p.size();
            // a file that does not end in a newline must not run into the next file's first header
            char last = 0;
            if (bsk_device_copy(&last, (char*)all.dptr + at - 1, 1, BSK_COPY_D2H) != BSK_OK) die(bsk_global_error());
            if (last != '\n') {
                const char nl = '\n';
                if (bsk_device_copy((char*)all.dptr + at, &nl, 1, BSK_COPY_H2D) != BSK_OK) die(bsk_global_error());
                ++at;
            }
        }
        all.n = at;
        release(inputs);
        inputs.push_back(all);
    }
    if (use == "stats") {
        std::string head, body;
        for (size_t fi = 0; fi < inputs.size(); ++fi) {
            const Part& in = inputs[fi];
            bsk_ctx* sc = nullptr;  // one Stats per input (cli/stats.go:16-21)
            if (bsk_create("Stats", js.c_str(), device, &sc) != BSK_OK) die(bsk_global_error());
            if (in.bgzf_fd >= 0) {  // every piece of the reader is a device shard of its own, the pids ascending
                const BgzfSizes z = bgzf_sizes();
                bsk_bgzf_reader* rd = nullptr;
                if (bsk_bgzf_reader_open(in.bgzf_fd, device, in.fmt, z.piece, z.look, z.chunk, &rd) != BSK_OK) die(bsk_global_error());
                int last = 0;
                for (int64_t pid = 0; !last; ++pid) {
                    const void* p = nullptr;
                    size_t n = 0;
                    uint64_t lo = 0, hi = 0;
                    if (bsk_bgzf_reader_next(rd, &p, &n, &lo, &hi, &last) != BSK_OK) die(bsk_global_error());
                    if (n && bsk_stats_run(sc, p, n, 1, in.fmt, pid, nullptr, nullptr) != BSK_OK) die(bsk_last_error(sc));
                }
                bsk_bgzf_reader_close(rd);  // (waits for the kernels that still read the last pieces)
            } else if (in.gzip_fd >= 0) {  // the same over the segment reader: the pass checks every member's CRC32 and ISIZE
                const GzipSizes z = gzip_sizes();
                bsk_gzip_reader* rd = nullptr;
                if (bsk_gzip_reader_open(in.gzip_fd, device, in.fmt, z.piece, z.look, z.segment, z.chunk, &rd) != BSK_OK) die(bsk_global_error());
                int last = 0;
                for (int64_t pid = 0; !last; ++pid) {
                    const void* p = nullptr;
                    size_t n = 0;
                    uint64_t lo = 0, hi = 0;
                    if (bsk_gzip_reader_next(rd, &p, &n, &lo, &hi, &last) != BSK_OK) die(bsk_global_error());
                    if (n && bsk_stats_run(sc, p, n, 1, in.fmt, pid, nullptr, nullptr) != BSK_OK) die(bsk_last_error(sc));
                }
                bsk_gzip_reader_close(rd);
            } else if (bsk_stats_run(sc, in.ptr(), in.size(), in.on_device(), in.fmt, 0, nullptr, nullptr) != BSK_OK) die(bsk_last_error(sc));
            std::vector<int64_t> keys(1 << 20), vals(1 << 20);
            size_t n = 0;
            if (bsk_stats_collect(sc, nullptr, keys.data(), vals.data(), keys.size(), &n) != BSK_OK) die(bsk_last_error(sc));
            bsk_statinfo info;
            bsk_stats_finalize(sc, keys.data(), vals.data(), n, &info);
            std::vector<char> buf(1 << 16);
            std::string name = "input" + std::to_string(fi);
            if (bsk_stats_string(sc, name.c_str(), "N/A", &info, buf.data(), buf.size()) != BSK_OK) die(bsk_last_error(sc));
            std::string table = buf.data();
            size_t nl = table.find('\n');
            head = table.substr(0, nl + 1);
            body += table.substr(nl + 1) + "\n";  // Join(lines[1:]) + "\n": a blank line per input, as written
            bsk_destroy(sc);
        }
        res.is_text = true;
        res.text = head + body;
        return res;
    }
    const bool grep_count = use == "grep" && inv.pget("count") == "true";
    const bool rows_out = use == "locate" || (use == "faidx" && !g_faidx_query);  // line-oriented text, not records
    const bool records_out = !(rows_out || grep_count);
    uint64_t grep_total = 0;
    bsk_ctx* ctx = nullptr;
    auto fresh = [&]() {
        bsk_ctx* c = nullptr;
        if (bsk_create(inv.cmd->op, js.c_str(), device, &c) != BSK_OK) die(bsk_global_error());
        return c;
    };
    if (!(keep_on_device && records_out)) {
        ctx = fresh();
        // the result goes to the host right after the run, while the input is still there: the operators that can leave their
        // text as ordered slices (rmdup, seq -n, subseq -r: include/bsk.h bsk_out.d_seg_*) do, and bsk_out_to_host gathers them
        bsk_ctx_set(ctx, "out", "slices");
    }
    // range / head: the record index runs over the union of the inputs (cli/helper.go unions the files into one
    // dataframe); negative positions need the total (bigseqkit/range.go:69-80)
    std::vector<uint64_t> first(inputs.size(), 0);
    uint64_t n_records = 0;
    bool range_needs = false;
    if (use == "range" || use == "head") {
        bsk_ctx* probe = fresh();
        int needs = 0;
        bsk_range_needs_count(probe, &needs);
        range_needs = needs != 0;
        if (range_needs || inputs.size() > 1)
            for (size_t fi = 0; fi < inputs.size(); ++fi) {
                uint64_t k = 0;
                if (bsk_index_build(probe, inputs[fi].ptr(), inputs[fi].size(), inputs[fi].on_device(), inputs[fi].fmt, nullptr, &k) != BSK_OK)
                    die(bsk_last_error(probe));
                first[fi] = n_records;
                n_records += k;
            }
        bsk_destroy(probe);
        if (ctx && range_needs && bsk_range_set_count(ctx, n_records) != BSK_OK) die(bsk_last_error(ctx));
    }
    // sample: exactly one input dataframe, the parts a `pipe` job hands over included (cli/sample.go:11-13) -- the verdict on a
    // record hangs on its index in that one input, which starts at 0; -n: fraction = Number / Count() (bigseqkit/sample.go:67-73)
    bool sample_needs = false;
    if (use == "sample" && inputs.size() != 1) die("only 1 file needed");
    if (use == "sample") {
        bsk_ctx* probe = fresh();
        int needs = 0;
        bsk_sample_needs_count(probe, &needs);
        sample_needs = needs != 0;
        if (sample_needs)
            for (auto& in : inputs) {
                uint64_t k = 0;
                if (bsk_index_build(probe, in.ptr(), in.size(), in.on_device(), in.fmt, nullptr, &k) != BSK_OK) die(bsk_last_error(probe));
                n_records += k;
            }
        bsk_destroy(probe);
        if (ctx && sample_needs && bsk_sample_set_count(ctx, n_records) != BSK_OK) die(bsk_last_error(ctx));
    }
    for (size_t fi = 0; fi < inputs.size(); ++fi) {
        const Part& in = inputs[fi];
        bsk_out out;
        bsk_ctx* c = ctx ? ctx : fresh();
        if (!ctx && range_needs && bsk_range_set_count(c, n_records) != BSK_OK) die(bsk_last_error(c));
        if (!ctx && sample_needs && bsk_sample_set_count(c, n_records) != BSK_OK) die(bsk_last_error(c));
        if (run_op(use, c, in, (int64_t)fi, first[fi], &out) != BSK_OK) die(bsk_last_error(c));
        if (use == "rmdup" && bsk_rmdup_finish(c) != BSK_OK) die(bsk_last_error(c));
        if (grep_count) {
            uint64_t cnt = 0;
            bsk_grep_last_count(c, &cnt);
            grep_total += cnt;
            continue;
        }
        const int ofmt = use == "translate" || use == "fq2fa" || use == "faidx" ? BSK_FORMAT_FASTA : in.fmt;
        if (!ctx) {  // device-resident part owned by its context
            Part o;
            o.fmt = ofmt;
            o.dptr = out.d_data;
            o.n = out.len;
            o.owner = c;
            res.parts.push_back(o);
            continue;
        }
        res.fmt = rows_out ? -1 : ofmt;
        // (in a `pipe` job only what is stored is compressed: what one job hands to the next stays text on the device)
        res.packed = !keep_on_device && packs_on_device(inv);
        append_result(c, out, res.text, res.packed);
    }
    if (ctx) bsk_destroy(ctx);
    if (grep_count) { res.is_text = true; res.text = std::to_string(grep_total); }  // fmt.Print: no newline (cli/grep.go:14)
    if (rows_out) res.is_text = keep_on_device;  // rows cannot feed another command
    return res;
}

// The key-bucket family of the command line (run_buckets): one row per command.
//   budget_env   the bytes a bucket may hold (rmdup, rename, common and the match buckets of pair and concat: bytes of subjects and
//                their per-record words, not of record text; the order buckets of pair: bytes of record text, the windows of concat:
//                the cost of their records, a bound of the text they collect and join -- both under the same budget); unset: 0
//   hist_run .. bucket_add, mark_hist, mark_buckets   the entry points of the passes all of them share, and their timing marks
//   plan_hint    what a fine bin holds, appended when bsk_shuffle_plan finds one above the budget
//   finish_out / finish_counted   a bucket leaves as text, or ends in its share of a verdict and returns two counters; that verdict
//   verdict_total / verdict_files   began with the records of the input, or with the records of every file
//   emit_run, mark_emit, emit_first_file_only   the emit pass behind the buckets (rmdup, rename, common), over every piece or
//                over those of the first file; pair and concat go on in tails of their own
//   counted, group_first, second_phase   the words of the [timing] summary of a command with a verdict
//   unfit_hint   read_parts: what to do about an input that could not be loaded whole (null: the answer of every other command)
struct BucketCmd {
    const char *use, *budget_env;
    decltype(&bsk_shuffle_hist_run) hist_run;
    decltype(&bsk_shuffle_hist_get) hist_get;
    decltype(&bsk_shuffle_bucket_begin) bucket_begin;
    decltype(&bsk_shuffle_bucket_add) bucket_add;
    const char *mark_hist, *mark_buckets, *plan_hint;
    decltype(&bsk_shuffle_bucket_finish) finish_out = nullptr;
    decltype(&bsk_rmdup_bucket_finish) finish_counted = nullptr;
    decltype(&bsk_rmdup_verdict_begin) verdict_total = nullptr;
    int (*verdict_files)(bsk_ctx*, const uint64_t*, uint32_t) = nullptr;
    decltype(&bsk_rmdup_emit_run) emit_run = nullptr;
    const char* mark_emit = nullptr;
    bool emit_first_file_only = false;
    const char *counted = nullptr, *group_first = nullptr, *second_phase = nullptr, *unfit_hint = nullptr;
};
static int pair_verdict_files(bsk_ctx* c, const uint64_t* r, uint32_t) { return bsk_pair_verdict_begin(c, r); }
static int concat_verdict_files(bsk_ctx* c, const uint64_t* r, uint32_t) { return bsk_concat_verdict_begin(c, r); }
static const BucketCmd kBucketCmds[] = {
    {.use = "shuffle", .budget_env = "BSK_SHUFFLE_BUDGET_BYTES",
     .hist_run = bsk_shuffle_hist_run, .hist_get = bsk_shuffle_hist_get, .bucket_begin = bsk_shuffle_bucket_begin, .bucket_add = bsk_shuffle_bucket_add,
     .mark_hist = "shuffle: histogram of the draws", .mark_buckets = "shuffle: buckets", .plan_hint = "",
     .finish_out = bsk_shuffle_bucket_finish,
     .unfit_hint = "shuffle orders all records of its input in one pass and runs on one device "
                   "(BSK_SHUFFLE_BUDGET_BYTES=<bytes> shuffles it in buckets of at most that many bytes, read once per bucket)"},
    {.use = "sort", .budget_env = "BSK_SORT_BUDGET_BYTES",
     .hist_run = bsk_sort_hist_run, .hist_get = bsk_sort_hist_get, .bucket_begin = bsk_sort_bucket_begin, .bucket_add = bsk_sort_bucket_add,
     .mark_hist = "sort: histogram of the bins", .mark_buckets = "sort: buckets",
     .plan_hint = " -- sort: a fine bin holds the records between two splitter keys; many equal keys, or a run that the sample missed, fill one",
     .finish_out = bsk_sort_bucket_finish,
     .unfit_hint = "sort orders all records of its input in one pass and runs on one device "
                   "(BSK_SORT_BUDGET_BYTES=<bytes> sorts it in buckets of at most that many bytes, read twice and once per bucket)"},
    {.use = "rmdup", .budget_env = "BSK_RMDUP_BUDGET_BYTES",
     .hist_run = bsk_rmdup_hist_run, .hist_get = bsk_rmdup_hist_get, .bucket_begin = bsk_rmdup_bucket_begin, .bucket_add = bsk_rmdup_bucket_add,
     .mark_hist = "rmdup: histogram of the bins", .mark_buckets = "rmdup: buckets",
     .plan_hint = " -- rmdup: a fine bin holds the subjects whose key shares its upper 12 bits; the copies of one subject fill one",
     .finish_counted = bsk_rmdup_bucket_finish, .verdict_total = bsk_rmdup_verdict_begin,
     .emit_run = bsk_rmdup_emit_run, .mark_emit = "rmdup: emit",
     .counted = "record(s) removed", .group_first = "survivor",
     .unfit_hint = "cut it over several GPUs (--devices 0-7), or BSK_RMDUP_BUDGET_BYTES=<bytes> removes the duplicates in buckets of "
                   "the key that hold at most that many bytes of subjects, read twice and once per bucket"},
    {.use = "rename", .budget_env = "BSK_RENAME_BUDGET_BYTES",
     .hist_run = bsk_rename_hist_run, .hist_get = bsk_rename_hist_get, .bucket_begin = bsk_rename_bucket_begin, .bucket_add = bsk_rename_bucket_add,
     .mark_hist = "rename: histogram of the bins", .mark_buckets = "rename: buckets",
     .plan_hint = " -- rename: a fine bin holds the IDs (-n: the names) whose key shares its upper 12 bits, once per record; the records of one ID fill one",
     .finish_counted = bsk_rename_bucket_finish, .verdict_total = bsk_rename_verdict_begin,
     .emit_run = bsk_rename_emit_run, .mark_emit = "rename: emit",
     .counted = "record(s) renamed", .group_first = "first",
     .unfit_hint = "rename numbers the records of an ID over its whole input and runs on one device "
                   "(BSK_RENAME_BUDGET_BYTES=<bytes> renames it in buckets of the key that hold at most that many bytes of "
                   "subjects, read twice and once per bucket)"},
    {.use = "common", .budget_env = "BSK_COMMON_BUDGET_BYTES",
     .hist_run = bsk_common_hist_run, .hist_get = bsk_common_hist_get, .bucket_begin = bsk_common_bucket_begin, .bucket_add = bsk_common_bucket_add,
     .mark_hist = "common: histogram of the bins", .mark_buckets = "common: buckets",
     .plan_hint = " -- common: a fine bin holds the subjects of all files whose key shares its upper 12 bits, once per record; the copies of one subject fill one",
     .finish_counted = bsk_common_bucket_finish, .verdict_files = bsk_common_verdict_begin,
     .emit_run = bsk_common_emit_run, .mark_emit = "common: emit", .emit_first_file_only = true,  // (the kept records of the first file)
     .counted = "record(s) kept", .group_first = "first"},
    {.use = "pair", .budget_env = "BSK_PAIR_BUDGET_BYTES",
     .hist_run = bsk_pair_hist_run, .hist_get = bsk_pair_hist_get, .bucket_begin = bsk_pair_bucket_begin, .bucket_add = bsk_pair_bucket_add,
     .mark_hist = "pair: histogram of the bins", .mark_buckets = "pair: match buckets",
     .plan_hint = " -- pair: a fine bin holds the IDs of both files whose key shares its upper 12 bits, once per record; the records of one ID fill one",
     .finish_counted = bsk_pair_bucket_finish, .verdict_files = pair_verdict_files,
     .counted = "pair(s)", .group_first = "first", .second_phase = "order bucket(s)"},
    {.use = "concat", .budget_env = "BSK_CONCAT_BUDGET_BYTES",
     .hist_run = bsk_concat_hist_run, .hist_get = bsk_concat_hist_get, .bucket_begin = bsk_concat_bucket_begin, .bucket_add = bsk_concat_bucket_add,
     .mark_hist = "concat: histogram of the bins", .mark_buckets = "concat: match buckets",
     .plan_hint = " -- concat: a fine bin holds the IDs of both files whose key shares its upper 12 bits, once per record; the records of one ID fill one",
     .finish_counted = bsk_concat_bucket_finish, .verdict_files = concat_verdict_files,
     .counted = "record(s) with a head", .group_first = "first", .second_phase = "window(s)"},
};
static const BucketCmd* bucket_cmd(const std::string& use) {
    for (const BucketCmd& r : kBucketCmds)
        if (use == r.use) return &r;
    return nullptr;
}
static uint64_t bucket_budget(const std::string& use) {
    const BucketCmd* cmd = bucket_cmd(use);
    const char* e = cmd ? getenv(cmd->budget_env) : nullptr;
    return e ? (uint64_t)strtoull(e, nullptr, 10) : 0;
}
bool g_buckets_unfit = false;  // read_parts: the whole-file load of a `shuffle` / `sort` / `rmdup` / `rename` input failed and a budget is set

// device >= 0: the files go straight to that GPU (bsk_shard_load: several readers, pread || H2D) -- what every command but
// the ones that join their inputs on the host (concat, common, pair) takes; device < 0: host strings
std::vector<Part> read_parts(const std::vector<Input>& inputs, int device = -1, const std::string& use = "") {
    std::vector<Part> parts;
    for (auto& in : inputs) {
        const std::string& f = in.path;
        Part p;
        if (device < 0 || (!in.missing && !in.regular)) {  // (a pipe: read to its end first)
            p.host = read_file(f);
            inflate_host_text(f, p.host);
            p.fmt = sniff_format(f, p.host);
        } else {
            bool segments = false;
            const bool pieces = admit({in}, Route::Device, use, &segments);
            const int fd = open(f.c_str(), O_RDONLY);
            if (fd < 0) die("open " + f + ": no such file or directory");
            if (in.kind == kGzip && stats_streams(use, in.size)) {  // (admitted: BSK_GZIP_STREAM=1) stats: the segment reader streams its text (execute)
                p.fmt = sniff_format(f, std::string(1, gzip_first_text_byte(f)));
                p.gzip_fd = fd;
                parts.push_back(std::move(p));
                continue;
            }
            if (in.kind == kBgzf && stats_streams(use, in.size)) {
                // stats: the file stays where it is, the piece reader streams its text in record-aligned pieces (execute)
                p.fmt = sniff_format(f, std::string(1, bgzf_first_text_byte(f)));
                p.bgzf_fd = fd;
                parts.push_back(std::move(p));
                continue;
            }
            if (in.kind != kPlain) {  // compressed across PCIe, inflated in HBM: from here on an ordinary device part
                if (in.kind == kGzip && bsk_gzip_load(fd, device, 0, 0, &p.dptr, &p.n) != BSK_OK) {  // (whole, unless its pieces were asked for)
                    if (bucket_budget(use) > 0 && segments) {
                        close(fd);
                        g_buckets_unfit = true;
                        release(parts);
                        return parts;
                    }
                    die(f + ": " + bsk_global_error() + " -- a gzip file is inflated whole on one device: it, its text and twice its text in symbols must fit there; "
                        "decompress it first (gzip -d), or recompress it with bgzip to use the paths for larger inputs");
                }
                if (in.kind == kBgzf && bsk_bgzf_load(fd, device, 0, &p.dptr, &p.n) != BSK_OK) {
                    if (bucket_budget(use) > 0 && pieces) {  // (as for a plain file that does not fit: through the buckets, piece by piece)
                        close(fd);
                        g_buckets_unfit = true;
                        release(parts);
                        return parts;
                    }
                    die(f + ": " + bsk_global_error() + " -- a BGZF file is inflated whole on one device: it and its text must fit there; decompress it first (bgzip -d) to use the paths for larger inputs -- "
                        "with BSK_BGZF_STREAM=1, 'stats' and the bucket paths (BSK_<COMMAND>_BUDGET_BYTES) read a larger one in pieces");
                }
                close(fd);
                char first = 0;
                if (p.n && bsk_device_copy(&first, p.dptr, 1, BSK_COPY_D2H) != BSK_OK) die(bsk_global_error());
                p.fmt = sniff_format(f, p.n ? std::string(1, first) : std::string());
                p.owned_alloc = true;
                parts.push_back(std::move(p));
                continue;
            }
            char first = 0;
            const ssize_t got = pread(fd, &first, 1, 0);
            p.fmt = sniff_format(f, got == 1 ? std::string(1, first) : std::string());
            p.n = in.size;
            if (stats_streams(use, p.n) || bsk_shard_load(fd, 0, p.n, device, 0, &p.dptr) != BSK_OK) {
                p.dptr = nullptr;
                if (use != "stats") {
                    close(fd);
                    const std::string what = std::string(bsk_global_error()) + " -- '" + use + "': " + f + " (" + std::to_string(p.n) + " bytes) must fit one GPU next to its result; ";
                    if (bucket_budget(use) > 0) {  // (the mapped files go through the buckets of the draw / of the key instead)
                        g_buckets_unfit = true;
                        release(parts);
                        return parts;
                    }
                    if (const BucketCmd* cmd = bucket_cmd(use))
                        if (cmd->unfit_hint) die(what + cmd->unfit_hint);
                    die(what + "cut it over several GPUs (--devices 0-7: fq2fa, grep, locate, rmdup, sample, seq, stats, subseq, translate)");
                }
                // stats: the file stays on the host, its mapping is streamed in record-aligned chunks
                p.map = mmap(nullptr, p.n, PROT_READ, MAP_SHARED, fd, 0);
                if (p.map == MAP_FAILED) die("mmap " + f + " failed");
                p.map_n = p.n;
                p.n = 0;
                close(fd);
                parts.push_back(std::move(p));
                continue;
            }
            p.owned_alloc = true;
            close(fd);
        }
        parts.push_back(std::move(p));
    }
    return parts;
}

// ---- faidx -d IDX (PARITY.md FAIX): regions fetched through the index, the sequence file never loaded whole
const char* const kFaidxIndexInPipe =
    "faidx: -d (--index-file) inside a 'pipe' job is refused: a job hands its input over as a dataframe on the device, the fetch "
    "through an index reads a file; run 'faidx -d' as a command of its own";
const char* const kFaidxIndexDevices =
    "faidx: -d (--index-file) with --devices is refused: the fetch reads the few spans of the file that the regions name, on one "
    "device (--device N)";

// the regions of `inv` through the present index `idx`: the batches of the plan, in order, are the result
Output run_faidx_fetch(const Invocation& inv, const Input& in, const std::string& idx) {
    const std::string rows = read_file(idx);
    const int fd = open(in.path.c_str(), O_RDONLY);
    if (fd < 0) die("open " + in.path + ": no such file or directory");
    // a BGZF file: the rows' offsets are text offsets, the block table FILE.gzi (htslib's format) turns them into blocks; where
    // that file is absent the table is built by a header walk and written there
    std::string gzi;
    uint64_t size = in.size;
    if (in.kind == kBgzf) {
        const std::string gzi_path = in.path + ".gzi";
        struct stat sb;
        if (stat(gzi_path.c_str(), &sb) == 0) {
            gzi = read_file(gzi_path);
        } else {
            size_t n = 0;
            bsk_bgzf_gzi_build(fd, nullptr, 0, &n, nullptr);
            gzi.assign(n, '\0');
            if (bsk_bgzf_gzi_build(fd, &gzi[0], gzi.size(), &n, nullptr) != BSK_OK) die(bsk_global_error());
            std::ofstream f(gzi_path, std::ios::binary);
            if (f) { f.write(gzi.data(), (std::streamsize)gzi.size()); f.close(); }
            if (!f && inv.pget("quiet") != "true")
                std::cerr << "[INFO] the block table could not be written to " << gzi_path << ": it is built again by the next run\n";
        }
        if (bsk_bgzf_gzi_text_size(fd, gzi.data(), gzi.size(), &size) != BSK_OK) die(bsk_global_error());
    }
    bsk_ctx* c = nullptr;
    const int device = (int)strtol(inv.pget("device").c_str(), nullptr, 10);
    if (bsk_create("Faidx", inv.js.c_str(), device, &c) != BSK_OK) die(bsk_global_error());
    bsk_fai_plan* plan = nullptr;
    if (bsk_faidx_fetch_plan(c, rows.data(), rows.size(), size, -1, 0, &plan) != BSK_OK) die(bsk_last_error(c));
    uint64_t counts[8];
    bsk_faidx_fetch_plan_counts(plan, counts);
    Output o;
    o.fmt = BSK_FORMAT_FASTA;
    o.packed = packs_on_device(inv);
    for (uint64_t b = 0; b < counts[2]; ++b) {
        bsk_out out;
        if (bsk_faidx_fetch_run(c, fd, in.kind == kBgzf ? gzi.data() : nullptr, gzi.size(), plan, (size_t)b, 0, nullptr, &out) != BSK_OK) die(bsk_last_error(c));
        append_result(c, out, o.text, o.packed);
    }
    bsk_faidx_fetch_plan_free(plan);
    bsk_destroy(c);
    close(fd);
    return o;
}

// IDX was absent: the run was today's whole-file run, and the index rows of the file (-f honoured) go to IDX -- the intent of
// StoreFASTX(idx, idxFile), bigseqkit-cli/faidx.go:29-32
void write_faidx_index(const Invocation& inv, const Part& in, const std::string& idx) {
    bsk_ctx* c = nullptr;
    const int device = (int)strtol(inv.pget("device").c_str(), nullptr, 10);
    if (bsk_create("Faidx", inv.js.c_str(), device, &c) != BSK_OK) die(bsk_global_error());
    bsk_out out;
    if (bsk_faidx_run(c, in.ptr(), in.size(), in.on_device(), in.fmt, 0, 0, nullptr, &out) != BSK_OK) die(bsk_last_error(c));
    std::string rows;
    append_result(c, out, rows, false);
    bsk_destroy(c);
    std::ofstream f(idx, std::ios::binary);
    if (f) { f.write(rows.data(), (std::streamsize)rows.size()); f.close(); }
    if (!f) die("write " + idx + " failed");
}

// `pipe` job (bigseqkit-cli/pipe.go:12-40): {"pipe": [job, ...], "cmd": ["grep", "-s", ...]} -- the outputs of the
// jobs under "pipe" become inputs of "cmd", ahead of the files named in it.  ("sh" hooks are not run.)
Output run_job(const bsk::json::Value& j, bool root) {
    std::vector<Part> inputs;
    if (const auto* deps = j.get("pipe")) {
        if (deps->kind == bsk::json::Value::Array)
            for (auto& d : deps->arr) {
                Output o = run_job(*d, false);
                if (o.is_text) die("bad execution dependency");  // pipe.go:26-28: the job produced no dataframe
                for (auto& p : o.parts) inputs.push_back(p);
            }
    }
    const auto* cmd = j.get("cmd");
    if (!cmd || cmd->kind != bsk::json::Value::Array || cmd->arr.empty()) die("incorrect job format");
    std::vector<std::string> args;
    for (auto& a : cmd->arr) args.push_back(a->str);
    Invocation inv = parse_invocation(args);
    // (-d applies to a run with regions only: in a job they come with -l, or as arguments behind the file)
    if (std::string(inv.cmd->use) == "faidx" && !inv.pget("index-file").empty() && (!inv.pget("region-file").empty() || inv.files.size() > 1))
        die(kFaidxIndexInPipe);
    for (auto& p : read_parts(classify_inputs(inv.files), (int)strtol(inv.pget("device").c_str(), nullptr, 10), inv.cmd->use)) inputs.push_back(std::move(p));
    if (inputs.empty()) die("no input for job command " + args[0]);
    Output o = execute(inv, inputs, !root);
    release(inputs);
    return o;
}

void store(const Invocation& inv, const Output& out, const std::vector<std::string>& files) {
    if (out.is_text) { std::cout << out.text; return; }
    const std::string& out_text = out.text;
    // ---- cli/helper.go:105-127
    std::string outp = inv.pget("out-file");
    if (outp.empty()) outp = files.size() == 1 ? files[0] + "-out" : (getenv("IGNIS_JOB_NAME") ? std::string(getenv("IGNIS_JOB_NAME")) + "-out" : std::string());
    if (outp.empty()) die("out file -o required");
    if (outp == "-") { fwrite(out_text.data(), 1, out_text.size(), stdout); return; }
    const bool bgzf = name_is_bgzf(outp);
    if (inv.pget("merge") == "true") {  // StoreFASTX: one file
        write_out_file(outp, bgzf, out.packed, out_text.data(), out_text.size());
        return;
    }
    // StoreFASTXN == SaveAsTextFile: a directory of part files; a record is never split between two parts
    long parts = strtol(inv.pget("partitions").c_str(), nullptr, 10);
    if (parts < 1) parts = 1;
    if (!is_dir(outp) && mkdir(outp.c_str(), 0755) != 0) die("cannot create directory " + outp);
    if (out.packed) {  // (packs_on_device: one part, compressed already)
        write_out_file(outp + "/part00000.gz", true, true, out_text.data(), out_text.size());
        return;
    }
    size_t pos = 0;
    for (long p = 0; p < parts; ++p) {
        size_t end = p + 1 == parts ? out_text.size() : out_text.size() * (size_t)(p + 1) / (size_t)parts;
        if (end < pos) end = pos;
        if (p + 1 < parts && end < out_text.size()) {
            if (out.fmt >= 0) {  // next record start (the anchor rule of the library)
                size_t cut = out_text.size();
                if (bsk_find_record_start((const uint8_t*)out_text.data(), out_text.size(), end, out.fmt, &cut) == BSK_OK) end = cut;
                else end = out_text.size();
            } else {
                while (end < out_text.size() && end > 0 && out_text[end - 1] != '\n') ++end;  // line granularity
            }
        }
        char nm[64];
        snprintf(nm, sizeof nm, "/part%05ld%s", p, part_suffix(bgzf));
        write_out_file(outp + nm, bgzf, false, out_text.data() + pos, end - pos);
        pos = end;
    }
}


// ---------------------------------------------------------------------------
// several GPUs, in THIS process (round 5): one worker thread + one context per device, the collectives of the command
// behind the C ABI (bsk_comm_*: librccl, ncclCommInitAll) -- what ignisDriver does with executors
// (bigseqkit-cli/helper.go:87-141; ReadFASTA/Q[N] + StoreFASTX[N], bigseqkit/helper.go:148-195).  No Python in the process
// tree (until round 4 this flag exec'd `python -m bigseqkit_amd.run`, which stays as the test harness of the Python side).
//   * the FILE is cut, not copied: it is mapped, every cut is the first record start at or behind size * k / world, found in
//     a 1 MiB window of the mapping (bsk_find_record_start: the ReadFixer rule; the window grows while it ends on a record
//     that may be cut off), and every worker brings only its own byte range to its GPU (bsk_shard_load: several readers,
//     pread || H2D in 16 MiB pieces);
//   * seq / grep / locate / subseq / translate / fq2fa: one call over the device-resident shard + bsk_store_put (D2H ||
//     write), or for shards over 48 GB bsk_run_to_store (pinned shard; H2D || kernels || D2H + write in chunks), into
//     <out>/part%05d, one per worker (StoreFASTXN) or, with --merge, into ONE file at offsets from an all-gather of the
//     sizes (the reference passes an MPI token, bigseqkit-lib/helper.go:399-429);
//   * stats: bsk_stats_collect_reduced (StatsReduce: one ncclAllReduce of the stats vector), worker 0 prints the table;
//   * grep -C: bsk_count_allreduce;   rmdup: bsk_rmdup_dist_run (the 24-byte tuple exchange of GroupByKey).
// ---------------------------------------------------------------------------
// BSK_CLI_TIMING=1: where the wall clock of a --devices call goes (stderr)
void mark(const char* what, int rank = -1) {
    static const bool on = getenv("BSK_CLI_TIMING") != nullptr;
    static const auto t0 = std::chrono::steady_clock::now();
    if (!on) return;
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (rank < 0) fprintf(stderr, "[timing] %8.3f s  %s\n", s, what);
    else fprintf(stderr, "[timing] %8.3f s  worker %d: %s\n", s, rank, what);
}

std::vector<int> parse_devices(const std::string& text) {
    std::vector<int> out;
    size_t i = 0;
    while (i <= text.size()) {
        const size_t e = std::min(text.find(',', i), text.size());
        const std::string piece = text.substr(i, e - i);
        if (!piece.empty()) {
            const size_t dash = piece.find('-', 1);
            char* end = nullptr;
            if (dash == std::string::npos) {
                const long v = strtol(piece.c_str(), &end, 10);
                if (*end || v < 0) die("--devices: bad device '" + piece + "'");
                out.push_back((int)v);
            } else {
                const long a = strtol(piece.substr(0, dash).c_str(), &end, 10), b = strtol(piece.substr(dash + 1).c_str(), nullptr, 10);
                if (a < 0 || b < a || b - a > 63) die("--devices: bad range '" + piece + "'");
                for (long v = a; v <= b; ++v) out.push_back((int)v);
            }
        }
        i = e + 1;
    }
    if (out.empty()) die("--devices names no device");
    if (out.size() > 64) die("--devices: at most 64 workers");
    return out;
}

std::vector<size_t> cut_points(const uint8_t* map, size_t size, int world, int fmt) {
    std::vector<size_t> cuts{0};
    for (int k = 1; k < world; ++k) {
        const size_t nominal = (size_t)((unsigned __int128)size * (unsigned)k / (unsigned)world);
        const size_t lo = std::max(nominal, cuts.back());
        if (lo >= size) { cuts.push_back(size); continue; }
        // the window: up to `win` bytes before `lo` (a FASTQ start is also judged by the record that ends there: anchor.hpp)
        // and `win` bytes behind it.  A start is taken when the next larger window names the same one -- a candidate that
        // was passed over because the window cut its record off shows up as a different answer -- and does not
        // sit within 64 KiB of the window's end.
        size_t win = 1u << 20;
        auto look = [&](size_t w, size_t* b_out) {
            const size_t a = lo > w ? lo - w : 0;
            const size_t b = std::min(size, lo + w);
            size_t found = 0;
            if (bsk_find_record_start(map + a, b - a, lo - a, fmt, &found) != BSK_OK) die(bsk_global_error());
            *b_out = b;
            return found + a;
        };
        for (;;) {
            size_t b = 0, b4 = 0;
            const size_t found = look(win, &b);
            if (b < size && (found + (64u << 10) > b || look(win * 4, &b4) != found)) { win *= 4; continue; }
            cuts.push_back(std::min(found, size));
            break;
        }
    }
    cuts.push_back(size);
    return cuts;
}

struct Worker {
    std::string error;            // why this worker gave up ("" = fine)
    uint64_t out_bytes = 0, out_records = 0;
    std::string spool;            // --merge / -o -: this worker's part before it is put in place
    std::string text;             // worker 0: what goes to stdout (stats table, grep -C count)
};

// len bytes of the file at `off` into buf with several readers (a copy out of the page cache is one core's work: ~9 GB/s with
// one thread on the box of round 6, where PCIe takes 55)
static bool parallel_pread(int fd, uint8_t* buf, size_t len, size_t off, int threads = 8) {
    if (len < ((size_t)64 << 20)) threads = 1;
    std::vector<std::future<bool>> jobs;
    const size_t per = (len + (size_t)threads - 1) / (size_t)threads;
    for (int t = 0; t < threads; ++t) {
        const size_t a = std::min(len, per * (size_t)t), b = std::min(len, a + per);
        if (a >= b) break;
        jobs.push_back(std::async(std::launch::async, [=]() {
            size_t done = a;
            while (done < b) {
                const ssize_t got = pread(fd, buf + done, std::min<size_t>(b - done, 64u << 20), (off_t)(off + done));
                if (got <= 0) return false;
                done += (size_t)got;
            }
            return true;
        }));
    }
    bool ok = true;
    for (auto& j : jobs) ok = j.get() && ok;
    return ok;
}

// A file of a streamed input on the host: a regular file is mapped -- only the pages that are handed on are ever read --, a pipe
// is read to its end first (`whole`)
struct MappedFile {
    std::string whole;
    const uint8_t* text = nullptr;
    size_t size = 0;
    bool mapped = false;
    // a BGZF file of the bucket paths is not mapped: its pieces are virtual-offset ranges, inflated on the device when asked for
    bsk_bgzf_reader* reader = nullptr;
    // ... nor is a plain gzip file (BSK_GZIP_STREAM=1): its pieces are ranges of text offsets, asked of the segment reader
    bsk_gzip_reader* gzip_reader = nullptr;
    int fd = -1;
    void unmap() {
        if (mapped && size) munmap((void*)text, size);
        mapped = false;
        if (reader) bsk_bgzf_reader_close(reader);
        if (gzip_reader) bsk_gzip_reader_close(gzip_reader);
        gzip_reader = nullptr;
        if (fd >= 0) close(fd);
        reader = nullptr;
        fd = -1;
    }
};
static void map_file(const std::string& path, MappedFile* f) {
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) die("open " + path + ": no such file or directory");
    struct stat sb;
    f->mapped = fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode);
    if (f->mapped) {
        f->size = (size_t)sb.st_size;
        if (f->size) {
            f->text = (const uint8_t*)mmap(nullptr, f->size, PROT_READ, MAP_SHARED, fd, 0);
            if (f->text == MAP_FAILED) die("mmap " + path + " failed");
        }
    } else {
        f->whole = read_file(path);
        f->text = (const uint8_t*)f->whole.data();
        f->size = f->whole.size();
    }
    close(fd);
}
// the end of the piece of about `piece` bytes that begins at `lo`: the record start behind lo + piece, or the end of the file
static size_t piece_end(const MappedFile& f, size_t lo, size_t piece, int fmt) {
    size_t at = 0;
    if (f.size - lo > piece && bsk_find_record_start(f.text, f.size, lo + piece, fmt, &at) == BSK_OK && at > lo && at < f.size) return at;
    return f.size;
}

// head-genome (cli/head_genome.go:11-15): every file is a run of its own, the results in the order of the files.  The answer
// is a prefix of the file, so the file is not brought to the GPU whole: pieces of its mapping that end on record starts go
// through ONE context, which carries the prefix words, n_1 and "cut reached" from piece to piece (PARITY.md HEADG), and the
// reading stops with the piece that holds the cut -- only the pages of the mapping that were handed over are ever read.  The
// first piece holds 64 MiB and every next one twice the last, up to 1 GiB; BSK_STREAM_PIECE_BYTES pins the size (tests).
Output run_head_genome(const Invocation& inv) {
    const int device = (int)strtol(inv.pget("device").c_str(), nullptr, 10);
    Output res;
    bsk_ctx* ctx = nullptr;
    if (bsk_create(inv.cmd->op, inv.js.c_str(), device, &ctx) != BSK_OK) die(bsk_global_error());
    bsk_ctx_set(ctx, "out", "slices");
    res.packed = packs_on_device(inv);
    const char* pinned = getenv("BSK_STREAM_PIECE_BYTES");
    for (auto& path : inv.files) {
        if (bsk_head_genome_reset(ctx) != BSK_OK) die(bsk_last_error(ctx));
        MappedFile f;
        map_file(path, &f);
        if (f.size && bsk_bgzf_probe(f.text, f.size) != 0) {  // (compressed: inflated on the host, then streamed like a pipe's text)
            std::string text((const char*)f.text, f.size);
            f.unmap();
            f.whole = std::move(text);
            inflate_host_text(path, f.whole);
            f.text = (const uint8_t*)f.whole.data();
            f.size = f.whole.size();
        }
        const int fmt = sniff_format(path, f.size ? std::string((const char*)f.text, 1) : std::string());
        res.fmt = fmt;
        size_t piece = pinned ? std::max<size_t>(1, (size_t)strtoull(pinned, nullptr, 10)) : ((size_t)64 << 20);
        size_t lo = 0;
        int64_t k = 0;
        while (lo < f.size) {
            const size_t hi = piece_end(f, lo, piece, fmt);
            bsk_out out;
            if (bsk_head_genome_run(ctx, f.text + lo, hi - lo, 0, fmt, k++, nullptr, &out) != BSK_OK) die(bsk_last_error(ctx));
            append_result(ctx, out, res.text, res.packed);
            int cut = 0;
            bsk_head_genome_state(ctx, &cut, nullptr);
            if (cut) break;  // the rest of the file is never read
            lo = hi;
            if (!pinned) piece = std::min<size_t>(piece * 2, (size_t)1 << 30);
        }
        f.unmap();
    }
    bsk_destroy(ctx);
    return res;
}

// shuffle in buckets of the draw, sort, rmdup, rename, common, pair and concat in buckets of the key (include/bsk.h; PARITY.md SHUF,
// SORT, RMDUPB, RENB, COMB, PAIRB, CONB): the way of the seven commands for an input that is larger than the byte budget of a bucket
// (budget_env of kBucketCmds) or -- the first four -- that could not be loaded whole.  The files stay on the host, mapped; several files are unioned in order (cli/shuffle.go:11-15,
// cli/sort.go), the record index runs over all of them.  Record-aligned pieces (BSK_STREAM_PIECE_BYTES, default 1 GiB) go
// through ONE context.  The mapping, the piece list, the plan and the timing line are shared; the passes differ:
//   shuffle   once for the histogram of the draws -- each piece's first record index is remembered -- and then once per bucket
//             of the plan: the input is read 1 + B times
//   sort      once for the sample of keys (which gives the splitters), once for the histogram and once per bucket, the pieces of a
//             bucket in input order: 2 + B times, and the FIRST piece once more (bsk_index_build: its record count).  The sample
//             rate comes from the file sizes and the record density of that piece and aims at about 32 samples per fine bin -- a starting value from sample-sort practice, not a measurement.
//             With -r the buckets leave from the last to the first.
//   rmdup     once for the histogram of the bins of the key, once per bucket -- the pieces in input order; a bucket holds subjects
//             and ends in its share of the verdict, it prints nothing -- and once for the emit, whose piece outputs are
//             appended to the result: 2 + B times.  -d / -D are refused by the histogram pass.
//   rename    the passes of rmdup; a bucket ends in its share of the ordinals, and the emit prints every record, renamed
//   common    the passes of rmdup over the pieces of ALL files (at least two, of one format), which are not a union to print but the
//             sets to compare: the histogram pass leaves the record count of every file, a bucket ends in its share of the keep
//             bits of the FIRST file, and the emit runs over the pieces of the first file only: 1 + B times, the first file once more
//   pair      (PARITY.md PAIRB) two files of one format, four outputs in -O <dir>, written share by share.  The match phase: the
//             passes of rmdup over the pieces of both files, a bucket ends in its share of the paired bits and the mates; the rank
//             step; the emit over both files prints paired.1, the unpaired files (-u) and -- file 2 in the order of its mates --
//             paired.2.  Otherwise the order phase prints paired.2: a histogram of the positions over file 2, the plan under the
//             same budget, one pass over file 2 per bucket.  File 1 is read 2 + B1 times; file 2 1 + B1 + 1 times when it is in
//             mate order, else 1 + B1 + 1 + B2 times and once more with -u
//   concat    (PARITY.md CONB) two files of one format.  The match phase: the passes of rmdup over the pieces of both files, a bucket
//             ends in its share of the heads.  The join phase: the weights of the heads over file 2, the histogram of the window
//             costs over file 1, the plan of windows under the same budget, per window the pieces of file 1 that reach into it and
//             every piece of file 2; every window's share is written as it finishes, and with -f the tail over file 2.  File 1 is
//             read 1 + B1 times, once for the window histogram and once across all windows; file 2 1 + B1 times, once for the
//             weights, once per window and once more with -f
// A BGZF input is refused as before unless BSK_BGZF_STREAM=1 asks for it.  Then it is not mapped: the piece reader (bsk_bgzf_reader_*) runs over it once and lists its pieces as ranges of virtual
// offsets, and every later pass asks the reader for the piece again -- inflated on the device, handed over as a device shard.  The
// file is inflated once per pass.  A plain gzip input (BSK_GZIP=1 BSK_GZIP_STREAM=1) goes the same way through the segment reader
// (bsk_gzip_reader_*), its pieces ranges of text offsets; the listing pass checks every member's CRC32 and ISIZE, so a corrupt file
// is refused before a byte of output is written.  Plain, BGZF and gzip inputs may be mixed.
// Every finished bucket is appended to the output.  A piece never spans two files, so a file that ends without a newline
// behaves like the union of the whole-file path: its last record gets the newline.
// The steps are written once: map_pieces (the files, their format and the pieces), plan_buckets (the passes in front of the buckets
// and the plan), then for a command whose buckets leave as text print_buckets, else decide_buckets and -- rmdup, rename, common --
// emit_pieces; pair and concat go on in pair_tail / concat_tail.  What differs between the commands is their row of kBucketCmds.
struct BucketRun {
    const BucketCmd& cmd;
    bsk_ctx* ctx = nullptr;
    uint64_t budget = 0;
    Output res;
    // host bytes, or (p == nullptr) n bytes of text that a reader is asked for: the range [vlo, vhi) of virtual offsets of a BGZF
    // file, or of text offsets of a plain gzip file
    enum PieceKind { kHostBytes, kBgzfRange, kGzipRange };
    struct Piece { const uint8_t* p; size_t n; uint64_t first; size_t file; uint64_t count; uint64_t vlo = 0, vhi = 0; PieceKind kind = kHostBytes; };
    struct View { const void* p; size_t n; int on_device; };
    std::vector<MappedFile> files;
    std::vector<Piece> pieces;
    std::vector<uint64_t> file_records;  // (behind the histogram pass)
    uint64_t total_bytes = 0;
    static constexpr uint32_t kBins = 4096;  // the fine bins of all of them (include/bsk.h)
    std::vector<uint64_t> hist = std::vector<uint64_t>(kBins), bounds = std::vector<uint64_t>(kBins + 1);
    int n_buckets = 0, n_second = 0;    // (n_second: the order buckets of pair, the windows of concat)
    uint64_t counted = 0, flagged = 0;  // (rmdup: removed; rename: renamed; common: kept; pair: pairs; concat: records with a head)

    void ok(int rc) const { if (rc != BSK_OK) die(bsk_last_error(ctx)); }
    // what an operator is handed for a piece: the mapped bytes, or the piece inflated on the device (valid until the second
    // view of a piece of the same file after it)
    View view(const Piece& pc) {
        if (pc.kind == kHostBytes) return {pc.p, pc.n, 0};
        const void* p = nullptr;
        size_t n = 0;
        if ((pc.kind == kGzipRange ? bsk_gzip_reader_piece(files[pc.file].gzip_reader, pc.vlo, pc.vhi, &p, &n)
                                   : bsk_bgzf_reader_piece(files[pc.file].reader, pc.vlo, pc.vhi, &p, &n)) != BSK_OK)
            die(bsk_global_error());
        return {p, n, 1};
    }
    // the files mapped, of one format, and cut into record-aligned pieces; a piece never spans two files
    void map_pieces(const std::vector<Input>& ins, size_t n_files, int device) {
        const char* pinned = getenv("BSK_STREAM_PIECE_BYTES");
        const size_t piece = pinned ? std::max<size_t>(1, (size_t)strtoull(pinned, nullptr, 10)) : ((size_t)1 << 30);
        files.resize(n_files);
        int fmt = -1;
        for (size_t fi = 0; fi < n_files; ++fi) {
            MappedFile& f = files[fi];
            const std::string& path = ins[fi].path;
            if (ins[fi].kind == kBgzf) {  // BGZF: the reader runs over the file once and lists its pieces; plain and BGZF inputs may be mixed
                f.fd = open(path.c_str(), O_RDONLY);
                if (f.fd < 0) die("open " + path + ": no such file or directory");
                const int ffmt = sniff_format(path, std::string(1, bgzf_first_text_byte(path)));
                if (fmt >= 0 && ffmt != fmt) die(std::string(cmd.use) + ": inputs of different formats");
                fmt = ffmt;
                const BgzfSizes z = bgzf_sizes();
                if (bsk_bgzf_reader_open(f.fd, device, fmt, z.piece, z.look, z.chunk, &f.reader) != BSK_OK) die(path + ": " + bsk_global_error());
                for (int last = 0; !last;) {
                    Piece pc{nullptr, 0, 0, fi, 0};
                    const void* p = nullptr;
                    if (bsk_bgzf_reader_next(f.reader, &p, &pc.n, &pc.vlo, &pc.vhi, &last) != BSK_OK) die(path + ": " + bsk_global_error());
                    pc.kind = kBgzfRange;
                    total_bytes += pc.n;
                    if (pc.n) pieces.push_back(pc);
                }
                continue;
            }
            if (ins[fi].kind == kGzip) {  // (admitted: BSK_GZIP_STREAM=1) the listing pass reads the whole file and checks every member
                f.fd = open(path.c_str(), O_RDONLY);
                if (f.fd < 0) die("open " + path + ": no such file or directory");
                const int ffmt = sniff_format(path, std::string(1, gzip_first_text_byte(path)));
                if (fmt >= 0 && ffmt != fmt) die(std::string(cmd.use) + ": inputs of different formats");
                fmt = ffmt;
                const GzipSizes z = gzip_sizes();
                if (bsk_gzip_reader_open(f.fd, device, fmt, z.piece, z.look, z.segment, z.chunk, &f.gzip_reader) != BSK_OK) die(path + ": " + bsk_global_error());
                for (int last = 0; !last;) {
                    Piece pc{nullptr, 0, 0, fi, 0};
                    const void* p = nullptr;
                    if (bsk_gzip_reader_next(f.gzip_reader, &p, &pc.n, &pc.vlo, &pc.vhi, &last) != BSK_OK) die(path + ": " + bsk_global_error());
                    pc.kind = kGzipRange;
                    total_bytes += pc.n;
                    if (pc.n) pieces.push_back(pc);
                }
                continue;
            }
            map_file(path, &f);
            const int ffmt = sniff_format(path, f.size ? std::string((const char*)f.text, 1) : std::string());
            if (fmt >= 0 && ffmt != fmt) die(std::string(cmd.use) + ": inputs of different formats");
            fmt = ffmt;
            total_bytes += f.size;
            for (size_t lo = 0; lo < f.size;) {
                const size_t hi = piece_end(f, lo, piece, fmt);
                pieces.push_back({f.text + lo, hi - lo, 0, fi, 0});
                lo = hi;
            }
        }
        res.fmt = fmt < 0 ? BSK_FORMAT_FASTA : fmt;
    }
    // the pass over all pieces that counts the records: it leaves every piece's first record index and its count
    template <class Call>
    void count_pass(Call call) {
        uint64_t g = 0;
        int64_t k = 0;
        for (auto& pc : pieces) {
            uint64_t cnt = 0;
            pc.first = g;
            ok(call(pc, k++, g, &cnt));
            g += cnt;
            pc.count = cnt;
        }
    }
    // sort: the sample of keys and the splitters; all: the histogram over all pieces and the plan of the buckets
    void plan_buckets() {
        if (std::string(cmd.use) == "sort") {
            double rate = 1.0;
            if (!pieces.empty()) {
                uint64_t cnt = 0;
                const View v = view(pieces[0]);
                ok(bsk_index_build(ctx, v.p, v.n, v.on_device, res.fmt, nullptr, &cnt));
                const double records = (double)total_bytes * (double)cnt / (double)std::max<size_t>(pieces[0].n, 1);
                rate = std::min(1.0, 32.0 * (double)kBins / std::max(records, 1.0));
            }
            count_pass([&](const Piece& pc, int64_t k, uint64_t g, uint64_t* cnt) {
                const View v = view(pc);
                return bsk_sort_sample_run(ctx, v.p, v.n, v.on_device, res.fmt, k, g, rate, nullptr, cnt);
            });
            uint32_t n_bins = 0;
            ok(bsk_sort_splitters_build(ctx, kBins, &n_bins));
            mark("sort: sample of the keys, splitters");
        }
        count_pass([&](const Piece& pc, int64_t k, uint64_t g, uint64_t* cnt) {
            const View v = view(pc);
            return cmd.hist_run(ctx, v.p, v.n, v.on_device, res.fmt, k, g, nullptr, cnt);
        });
        mark(cmd.mark_hist);
        file_records.assign(files.size(), 0);
        for (auto& pc : pieces) file_records[pc.file] += pc.count;
        ok(cmd.hist_get(ctx, hist.data(), nullptr));
        if (bsk_shuffle_plan(hist.data(), budget, bounds.data(), &n_buckets) != BSK_OK) die(std::string(bsk_global_error()) + cmd.plan_hint);
    }
    // bucket b of the plan opened and every piece added to it, in input order
    void fill_bucket(int b) {
        ok(cmd.bucket_begin(ctx, (uint32_t)bounds[b], (uint32_t)bounds[b + 1]));
        int64_t k = 0;
        for (auto& pc : pieces) {
            const View v = view(pc);
            ok(cmd.bucket_add(ctx, v.p, v.n, v.on_device, res.fmt, k++, pc.first, nullptr));
        }
    }
    void append_out(const bsk_out& out) { append_result(ctx, out, res.text, res.packed); }
    // shuffle, sort: every finished bucket is appended to the output; backwards (sort -r): from the last to the first
    void print_buckets(bool backwards) {
        for (int i = 0; i < n_buckets; ++i) {
            fill_bucket(backwards ? n_buckets - 1 - i : i);
            bsk_out out;
            ok(cmd.finish_out(ctx, nullptr, &out));
            append_out(out);
        }
        mark(cmd.mark_buckets);
    }
    // the others: the verdict begins; every bucket over all pieces, in order, ends in its share of it
    void decide_buckets() {
        uint64_t total_records = 0;
        for (uint64_t n : file_records) total_records += n;
        ok(cmd.verdict_total ? cmd.verdict_total(ctx, total_records) : cmd.verdict_files(ctx, file_records.data(), (uint32_t)file_records.size()));
        for (int b = 0; b < n_buckets; ++b) {
            fill_bucket(b);
            uint64_t r = 0, f = 0;
            ok(cmd.finish_counted(ctx, nullptr, &r, &f));
            counted += r;
            flagged += f;
        }
        mark(cmd.mark_buckets);
    }
    // rmdup, rename, common: one emit pass prints the records in file order
    void emit_pieces() {
        int64_t k = 0;
        for (auto& pc : pieces) {
            if (cmd.emit_first_file_only && pc.file != 0) break;
            bsk_out out;
            const View v = view(pc);
            ok(cmd.emit_run(ctx, v.p, v.n, v.on_device, res.fmt, k++, pc.first, nullptr, &out));
            append_out(out);
        }
        mark(cmd.mark_emit);
    }
    void pair_tail(const Invocation& inv, const std::string& outdir);
    void concat_tail(const Invocation& inv);
};

// pair behind its match buckets: the rank step, the emit over both files and -- file 2 out of mate order -- the order buckets
void BucketRun::pair_tail(const Invocation& inv, const std::string& outdir) {
    const bool unp = inv.pget("save-unpaired") == "true";
    if (!is_dir(outdir) && mkdir(outdir.c_str(), 0755) != 0) die("cannot create directory " + outdir);
    const char* names[4] = {"paired.1", "paired.2", "unpaired.1", "unpaired.2"};
    std::ofstream outf[4];
    for (int k = 0; k < (unp ? 4 : 2); ++k) {
        outf[k].open(outdir + "/" + names[k], std::ios::binary);
        if (!outf[k]) die("cannot create " + outdir + "/" + names[k]);
    }
    std::string share;
    auto write_share = [&](int k, const bsk_out& out) {
        if (!out.len || !outf[k].is_open()) return;
        share.resize(out.len);
        ok(bsk_out_to_host(ctx, &out, &share[0], out.len));
        outf[k].write(share.data(), (std::streamsize)share.size());
        if (!outf[k]) die("write " + outdir + "/" + names[k] + " failed");
    };
    decide_buckets();
    uint64_t n_pairs = 0;
    int in_mate_order = 0;
    ok(bsk_pair_order_begin(ctx, nullptr, &n_pairs, &in_mate_order));
    const char* forced = getenv("BSK_PAIR_ORDER");  // (the switch pair_order of the context: the emit leaves paired.2 to the order phase)
    const bool by_emit = in_mate_order && !(forced && std::string(forced) == "buckets");
    // the emit: paired.1 and unpaired.1 from the pieces of file 1; unpaired.2 -- and paired.2 when it is a filter of file 2 --
    // from those of file 2, which are not read when neither is wanted
    int64_t k = 0;
    for (auto& pc : pieces) {
        if (pc.file == 1 && !unp && !by_emit) break;
        bsk_out outs[3];
        const View v = view(pc);
        ok(bsk_pair_emit_run(ctx, v.p, v.n, v.on_device, res.fmt, k++, pc.first, nullptr, outs));
        if (pc.file == 0) write_share(0, outs[0]);
        else write_share(1, outs[2]);
        write_share(pc.file == 0 ? 2 : 3, outs[1]);
    }
    mark("pair: emit");
    if (n_pairs && !by_emit) {
        // paired.2 in buckets of the position: the histogram over the pieces of file 2, the plan, one pass per bucket
        for (auto& pc : pieces) {
            uint64_t cnt = 0;
            if (pc.file != 1) continue;
            const View v = view(pc);
            ok(bsk_pair_order_hist_run(ctx, v.p, v.n, v.on_device, res.fmt, k++, pc.first, nullptr, &cnt));
        }
        ok(bsk_pair_order_hist_get(ctx, hist.data(), nullptr));
        if (bsk_shuffle_plan(hist.data(), budget, bounds.data(), &n_second) != BSK_OK)
            die(std::string(bsk_global_error()) + " -- pair: an order bin holds the text of the records of paired.2 whose positions share their upper bits, "
                                                   "at most a 4096th of the pairs rounded up to a power of two");
        for (int b = 0; b < n_second; ++b) {
            ok(bsk_pair_order_bucket_begin(ctx, (uint32_t)bounds[b], (uint32_t)bounds[b + 1]));
            for (auto& pc : pieces) {
                if (pc.file != 1) continue;
                const View v = view(pc);
                ok(bsk_pair_order_bucket_add(ctx, v.p, v.n, v.on_device, res.fmt, k++, pc.first, nullptr));
            }
            bsk_out out;
            ok(bsk_pair_order_bucket_finish(ctx, nullptr, &out));
            write_share(1, out);
        }
        mark("pair: order buckets");
    }
    for (int j = 0; j < 4; ++j)
        if (outf[j].is_open()) {
            outf[j].close();
            if (!outf[j]) die("write " + outdir + "/" + names[j] + " failed");
        }
}

// concat behind its match buckets: the weights, the window histogram and its plan, the windows and -- -f -- the tail
void BucketRun::concat_tail(const Invocation& inv) {
    // one file (-o <file> --merge) or the standard output (-o -) receives the shares as they finish; a directory of part files
    // is cut from the whole result, which is collected on the host then (store)
    const std::string outp = inv.pget("out-file");
    const bool to_stdout = outp == "-", to_file = !outp.empty() && !to_stdout && inv.pget("merge") == "true";
    std::ofstream outf;
    if (to_file) {
        outf.open(outp, std::ios::binary);
        if (!outf) die("cannot create " + outp);
    }
    res.stored = to_file || to_stdout;
    const bool pack = to_file && name_is_bgzf(outp);
    std::string share;
    auto write_share = [&](const bsk_out& out) {
        if (!res.stored) return append_out(out);
        if (!out.len) return;
        share.clear();
        append_result(ctx, out, share, pack);
        if (to_stdout) fwrite(share.data(), 1, share.size(), stdout);
        else outf.write(share.data(), (std::streamsize)share.size());
        if (to_file && !outf) die("write " + outp + " failed");
    };
    decide_buckets();
    // the weights over the pieces of file 2, the window histogram over those of file 1, the plan of the windows
    ok(bsk_concat_join_begin(ctx, nullptr));
    int64_t k = 0;
    for (int file = 1; file >= 0; --file)
        for (auto& pc : pieces) {
            uint64_t cnt = 0;
            if ((int)pc.file != file) continue;
            const View v = view(pc);
            ok((file ? bsk_concat_weigh_run : bsk_concat_window_hist_run)(ctx, v.p, v.n, v.on_device, res.fmt, k++, pc.first, nullptr, &cnt));
        }
    ok(bsk_concat_window_hist_get(ctx, hist.data(), nullptr));
    if (bsk_shuffle_plan(hist.data(), budget, bounds.data(), &n_second) != BSK_OK)
        die(std::string(bsk_global_error()) + " -- concat: a window bin holds the cost of at most a 4096th of the records of file 1, rounded up to a "
                                               "power of two: their text, the text of the records of file 2 with their IDs, and a bound of the joined "
                                               "records; an ID with many records in both files fills one");
    mark("concat: weights, histogram of the windows");
    uint32_t shift = 0;
    while (file_records[0] && ((file_records[0] - 1) >> shift) >= kBins) ++shift;
    for (int b = 0; b < n_second; ++b) {
        const uint64_t lo = bounds[b], hi = bounds[b + 1];
        ok(bsk_concat_window_begin(ctx, (uint32_t)lo, (uint32_t)hi));
        for (auto& pc : pieces) {
            // (a piece of file 1 wholly outside the window adds nothing)
            if (pc.file == 0 && (pc.count == 0 || ((pc.first + pc.count - 1) >> shift) < lo || (pc.first >> shift) >= hi)) continue;
            const View v = view(pc);
            ok(bsk_concat_window_add(ctx, v.p, v.n, v.on_device, res.fmt, k++, pc.first, nullptr));
        }
        bsk_out out;
        ok(bsk_concat_window_finish(ctx, nullptr, &out));
        write_share(out);
    }
    mark("concat: windows");
    if (inv.pget("full") == "true") {
        for (auto& pc : pieces) {
            if (pc.file != 1) continue;
            bsk_out out;
            const View v = view(pc);
            ok(bsk_concat_tail_run(ctx, v.p, v.n, v.on_device, res.fmt, k++, pc.first, nullptr, &out));
            write_share(out);
        }
        mark("concat: tail");
    }
    if (to_file) {
        if (pack) outf.write(eof_block().data(), 28);
        outf.close();
        if (!outf) die("write " + outp + " failed");
    }
}

Output run_buckets(const Invocation& inv, const std::vector<Input>& ins) {
    const std::string use = inv.cmd->use;
    const bool pair = use == "pair", concat = use == "concat";
    if (concat && inv.files.size() != 2) die("2 files needed");  // cli/concat.go
    if (use == "common" && inv.files.size() < 2) die("at least 2 files needed");  // cli/common.go
    const std::string outdir = pair ? inv.pget("out-dir") : std::string();
    if (pair) {  // cli/pair.go:13-66, the checks of the whole-file path
        if (inv.files.size() < 2) die("2 files needed");
        if (outdir.empty()) die("out-dir required");
    }
    admit(ins, Route::Buckets, use);  // (plain gzip has pieces only with BSK_GZIP_STREAM=1: said before a device is touched)
    const int device = (int)strtol(inv.pget("device").c_str(), nullptr, 10);
    BucketRun R{*bucket_cmd(use)};
    R.res.packed = !pair && packs_on_device(inv);  // (pair -O writes its four files under fixed names: plain)
    R.budget = bucket_budget(use);
    if (bsk_create(inv.cmd->op, inv.js.c_str(), device, &R.ctx) != BSK_OK) die(bsk_global_error());
    const bool timing = getenv("BSK_CLI_TIMING") != nullptr;
    if (timing) bsk_profile_enable(R.ctx, 1);
    R.map_pieces(ins, pair || concat ? 2 : ins.size(), device);
    R.plan_buckets();
    if (concat) {
        R.concat_tail(inv);
    } else if (pair) {
        R.pair_tail(inv, outdir);
    } else if (R.cmd.finish_out) {
        R.print_buckets(use == "sort" && inv.pget("reverse") == "true");
    } else {
        R.decide_buckets();
        R.emit_pieces();
    }
    if (timing) {
        std::vector<char> buf(1 << 16);
        if (bsk_profile_dump(R.ctx, buf.data(), buf.size()) == BSK_OK)
            fprintf(stderr, "[timing] %s in %d bucket(s) of at most %llu bytes, %zu piece(s); stages: %s\n", use.c_str(), R.n_buckets,
                    (unsigned long long)R.budget, R.pieces.size(), buf.data());
        if (R.cmd.counted) {
            fprintf(stderr, "[timing] %s: %llu %s, %llu flagged (subject differed from the %s of its key group)", use.c_str(),
                    (unsigned long long)R.counted, R.cmd.counted, (unsigned long long)R.flagged, R.cmd.group_first);
            if (R.cmd.second_phase) fprintf(stderr, ", %d %s", R.n_second, R.cmd.second_phase);
            fprintf(stderr, "\n");
        }
    }
    for (auto& f : R.files) f.unmap();
    bsk_destroy(R.ctx);
    return R.res;
}

int run_devices(const Invocation& inv) {
    const std::string use = inv.cmd->use;
    static const char* const kStreamed[] = {"seq", "grep", "locate", "subseq", "translate", "fq2fa", "replace", "fa2fq", "sample"};
    bool streamed = false;
    for (const char* u : kStreamed) streamed = streamed || use == u;
    if (!streamed && use != "stats" && use != "rmdup")
        die("'" + use + "' runs on one device (bigseqkit " + use + " ... --device N); several GPUs: fa2fq, fq2fa, grep, locate, replace, rmdup, sample, seq, stats, subseq, translate");
    if (inv.files.size() != 1) die("--devices: exactly one input file (it is cut into one shard per GPU)");
    const std::vector<int> devices = parse_devices(inv.pget("devices"));
    const int world = (int)devices.size();
    const std::vector<Input> ins = classify_inputs(inv.files);
    const bool admit_pieces = admit(ins, Route::Devices);  // (BSK_BGZF_STREAM=1: `stats` may read a worker's range in pieces)
    // (admitted: BSK_BGZF_DEVICES=1) a BGZF file is cut at block starts near size * k / world, found from the file's bytes there,
    // and at the first record start of the text behind them (bsk_bgzf_cut_points: PARITY.md BGZF "workers"); a worker's range is
    // a pair of virtual offsets, its shard what bsk_bgzf_shard_load inflates of it -- from there on a device shard as any other
    const bool bgzf_in = ins[0].kind == kBgzf;
    mark("start");
    if (bsk_device_count() <= 0) die("no HIP device visible (the hot path has no CPU fallback)");
    const std::string& path = inv.files[0];
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) die("open " + path + ": no such file or directory");
    struct stat sb;
    if (fstat(fd, &sb) != 0) die("stat " + path + " failed");
    const size_t size = (size_t)sb.st_size;
    const uint8_t* map = nullptr;
    if (size && !bgzf_in) {
        map = (const uint8_t*)mmap(nullptr, size, PROT_READ, MAP_SHARED, fd, 0);
        if (map == MAP_FAILED) die("mmap " + path + " failed");
    }
    const int fmt = bgzf_in ? sniff_format(path, std::string(1, bgzf_first_text_byte(path))) : sniff_format(path, size ? std::string((const char*)map, 1) : std::string());
    const std::vector<size_t> cuts = size && !bgzf_in ? cut_points(map, size, world, fmt) : std::vector<size_t>((size_t)world + 1, 0);
    if (map) munmap((void*)map, size);
    mark("device count + cut points");
    std::vector<uint64_t> voffs((size_t)world + 1, 0);
    if (bgzf_in) {
        if (bsk_bgzf_cut_points(fd, fmt, world, voffs.data()) != BSK_OK) die(path + ": " + bsk_global_error());
        mark("bgzf cut points");
    }
    // RCCL greets on file descriptor 1 (its version banner, when a communicator is first used) -- and stdout is where
    // `stats`, `grep -C` and `-o -` put their RESULT.  For the rest of this call descriptor 1 IS stderr; results go to the
    // real stdout through a duplicate of it.
    fflush(stdout);
    const int real_out = dup(1);
    if (real_out < 0 || dup2(2, 1) < 0) die("cannot duplicate the standard output");
    std::vector<bsk_comm*> comms((size_t)world, nullptr);
    if (bsk_comm_init_all(world, devices.data(), comms.data()) != BSK_OK) die(bsk_comm_error(nullptr));
    mark("communicators");

    std::string out_file = inv.pget("out-file");
    if (out_file.empty()) out_file = path + "-out";
    const bool merge = inv.pget("merge") == "true", to_stdout = out_file == "-";
    const bool bgzf = name_is_bgzf(out_file);  // (every store below writes BGZF then: bsk_store_set_bgzf)
    const bool grep_count = use == "grep" && inv.pget("count") == "true";
    const bool records = !(use == "stats" || grep_count);
    bsk_store* dir_store = nullptr;
    char token[64];
    snprintf(token, sizeof token, "%d-%08x", (int)getpid(), (unsigned)((uintptr_t)&token ^ (uintptr_t)time(nullptr) * 2654435761u));
    if (records && !merge && !to_stdout) {
        if (!is_dir(out_file) && mkdir(out_file.c_str(), 0755) != 0) die("cannot create directory " + out_file);
        // (part files of an earlier run with MORE workers would be read as part of this result: ADVICE r04)
        for (int k = world; k < world + 4096; ++k) {
            char nm[64];
            snprintf(nm, sizeof nm, "/part%05d%s", k, part_suffix(bgzf));
            if (unlink((out_file + nm).c_str()) != 0) break;
        }
        if (bsk_store_open(out_file.c_str(), 0, &dir_store) != BSK_OK) die("cannot open the directory " + out_file);
        bsk_store_set_bgzf(dir_store, bgzf);
    }
    std::vector<Worker> W((size_t)world);
    std::atomic<int> failed{0};
    // shard + output + tables of a record operator next to each other in 288 GB: shards up to 48 GB (translate -f 6 writes
    // twice its input); BSK_HOST_PIPELINE_FROM moves the line (tests: 0 = always the chunked host pipeline)
    size_t host_pipeline_from = (size_t)48 << 30;
    if (const char* e = getenv("BSK_HOST_PIPELINE_FROM")) host_pipeline_from = (size_t)strtoull(e, nullptr, 10);

    auto work = [&](int rank) {
        Worker& me = W[(size_t)rank];
        bsk_comm* comm = comms[(size_t)rank];
        const int device = devices[(size_t)rank];
        const size_t lo = cuts[(size_t)rank];
        size_t n = cuts[(size_t)rank + 1] - lo;  // (a BGZF shard: its text, known once it is inflated)
        const uint64_t v_lo = voffs[(size_t)rank], v_hi = voffs[(size_t)rank + 1];
        // the compressed bytes of a BGZF shard, to the start of the next worker's first block (its own last block may add 64 KiB)
        const size_t comp_n = bgzf_in ? (size_t)((v_hi >> 16) - (v_lo >> 16)) + ((v_hi & 0xFFFFu) ? 1 : 0) : 0;
        bsk_ctx* ctx = nullptr;
        void* d_shard = nullptr;
        void* h = nullptr;
        // stats: a shard that does not fit (or whose allocation fails) is streamed from the file in pinned pieces (below)
        const bool stats_stream = bgzf_in ? v_hi > v_lo && stats_streams(use, comp_n) : use == "stats" && n > 0 && n >= std::min(host_pipeline_from * 4, whole_file_limit());
        const bool via_host = !bgzf_in && streamed && n > host_pipeline_from;
        bsk_store* own = nullptr;
        bool stream_stats = stats_stream;
        auto give_up = [&](const std::string& m) { if (me.error.empty()) me.error = m.empty() ? "failed" : m; failed.fetch_add(1); };
        do {
            if (bsk_create(inv.cmd->op, inv.js.c_str(), device, &ctx) != BSK_OK) { give_up(bsk_global_error()); break; }
            bsk_ctx_set(ctx, "out", "slices");  // (the shard stays on the device until bsk_store_put has drained the result)
            mark("context", rank);
            // this worker's bytes, and only they: from the file to the device in pieces, several readers (bsk_shard_load).
            // A record operator whose shard AND output may not fit the GPU side by side keeps the chunked host pipeline
            // (bsk_run_to_store: pinned shard, 256 MiB chunks through two device buffers).
            if (stats_stream) break;
            if (bgzf_in) {
                // (v_hi == v_lo, an empty shard -- more workers than blocks, or one record over the whole range -- is loaded as well)
                if (bsk_bgzf_shard_load(fd, v_lo, v_hi, device, 0, &d_shard, &n) != BSK_OK) {
                    d_shard = nullptr;
                    n = 0;
                    const std::string why = bsk_global_error();
                    // (the join check, a damaged block: said as it is.  No room: stats reads the range in pieces instead)
                    const bool no_room = why.find("do not fit") != std::string::npos || why.find("allocation") != std::string::npos;
                    if (use == "stats" && no_room) { stream_stats = true; break; }
                    give_up(path + ": " + why + (no_room ? " -- '" + use + "' needs every worker's shard (" + std::to_string(comp_n) + " compressed bytes here) and its text in HBM: more devices make smaller shards" : std::string()));
                    break;
                }
                mark("bgzf shard on the device", rank);
                // the pipelined host path is not built for compressed shards: the line that sends a plain shard there refuses this one
                if (use != "stats" && n > host_pipeline_from) {
                    give_up(path + ": this worker's shard (" + std::to_string(comp_n) + " compressed bytes, " + std::to_string(n) + " bytes of text) is above the " +
                            std::to_string(host_pipeline_from) + " bytes that '" + use + "' keeps on the device next to its result, and a compressed shard is not streamed through the host: "
                            "more devices make smaller shards, or decompress the file first (bgzip -d)");
                    break;
                }
                break;
            }
            if (!via_host) {
                if (bsk_shard_load(fd, (uint64_t)lo, n, device, 0, &d_shard) != BSK_OK) {
                    if (use == "stats") { d_shard = nullptr; stream_stats = true; break; }  // (no room: streamed below)
                    if (use == "rmdup")
                        give_up(std::string(bsk_global_error()) + " -- rmdup needs every worker's shard (" + std::to_string(n) +
                                " bytes here) in HBM next to its tables: more devices make smaller shards");
                    else give_up(bsk_global_error());
                    break;
                }
                mark("shard on the device", rank);
                break;
            }
            // (round 6: the shard is NOT read into one pinned buffer first -- 100 GB took 12 s to pin and 10 s to read with one
            // thread before the first kernel ran: grep on the whole C2 file 29.5 s, bench.py end_to_end_config_size.  It is
            // streamed below in pieces through two pinned buffers, the pread of piece k + 1 under the pipeline of piece k.)
        } while (false);
        // every worker enters every collective, also the one that has given up (its contribution is empty): the others must
        // not wait for it for ever
        if (bgzf_in) {
            // the barrier of the join check: every worker has loaded its shard and walked its chain before any operator runs, so
            // a run that is refused there has written no part file, no spool and no table
            if (me.error.empty() && stream_stats && !admit_pieces)
                give_up(path + ": this worker's range (" + std::to_string(comp_n) + " compressed bytes) is not loaded whole; set BSK_BGZF_STREAM=1 to have 'stats' read it in "
                        "record-aligned pieces, or use more devices: they make smaller shards");
            uint64_t bad = (uint64_t)failed.load();
            if (bsk_count_allreduce(comm, &bad, nullptr) != BSK_OK) { give_up(bsk_comm_error(comm)); bad = 1; }
            if (bad) {
                if (d_shard) bsk_device_free(d_shard);
                if (ctx) bsk_destroy(ctx);
                return;
            }
        }
        const bool ok0 = me.error.empty();
        if (use == "stats") {
            std::vector<int64_t> keys(1 << 20), vals(1 << 20);
            size_t cnt = 0;
            int rc = ok0 ? bsk_stats_reset(ctx, nullptr) : BSK_ERR_INVALID_ARG;
            if (rc == BSK_OK && n && !stream_stats) rc = bsk_stats_run(ctx, d_shard, n, 1, fmt, rank, nullptr, nullptr);
            if (rc == BSK_OK && bgzf_in && stream_stats && v_hi > v_lo) {
                // the worker's range through the piece reader on its device: seek, then piece after piece; the piece that would run
                // past the next worker's start is asked for again by its offsets -- which also is this path's join check: an
                // offset that is not on the reader's chain is no position of the text, and the reader says so
                const BgzfSizes z = bgzf_sizes();
                bsk_bgzf_reader* rd = nullptr;
                rc = bsk_bgzf_reader_open(fd, device, fmt, z.piece, z.look, z.chunk, &rd);
                if (rc == BSK_OK) rc = bsk_bgzf_reader_seek(rd, v_lo);
                for (int64_t k = 0; rc == BSK_OK; ++k) {
                    const void* p = nullptr;
                    size_t pn = 0;
                    uint64_t plo = 0, phi = 0;
                    int last = 0;
                    rc = bsk_bgzf_reader_next(rd, &p, &pn, &plo, &phi, &last);
                    if (rc == BSK_OK && phi > v_hi) rc = bsk_bgzf_reader_piece(rd, plo, v_hi, &p, &pn);
                    if (rc != BSK_OK) break;
                    if (pn && bsk_stats_run(ctx, p, pn, 1, fmt, (int64_t)rank * 1000000 + k, nullptr, nullptr) != BSK_OK) { rc = BSK_ERR_INVALID_ARG; give_up(bsk_last_error(ctx)); break; }
                    if (last || phi >= v_hi) break;
                }
                if (rc != BSK_OK && me.error.empty()) give_up(path + ": " + bsk_global_error());
                if (rd) bsk_bgzf_reader_close(rd);
                mark("bgzf range streamed in pieces", rank);
            } else if (rc == BSK_OK && n && stream_stats) {
                // Round 6: a shard larger than the GPU's memory (the reference takes any file size through its partitions,
                // bigseqkit/helper.go:148-178).  Pieces of ~1 GiB that end on record starts are read into two pinned buffers
                // -- the pread of piece i + 1 runs while piece i crosses PCIe under the kernels (bsk_stats_run with a host
                // pointer: record-aligned chunks through two device buffers) -- and accumulate into the one stats vector.
                const size_t piece = std::max<size_t>(1 << 16, getenv("BSK_STATS_PIECE_BYTES") ? (size_t)strtoull(getenv("BSK_STATS_PIECE_BYTES"), nullptr, 10) : ((size_t)1 << 30));
                const uint8_t* fmap = (const uint8_t*)mmap(nullptr, size, PROT_READ, MAP_SHARED, fd, 0);  // (only the pages around the cuts are touched)
                uint8_t* pin[2] = {(uint8_t*)bsk_host_alloc(piece + (64 << 20)), (uint8_t*)bsk_host_alloc(piece + (64 << 20))};
                if (fmap == MAP_FAILED || !pin[0] || !pin[1]) { rc = BSK_ERR_HIP; give_up("stats: no pinned memory / mapping for the streamed shard"); }
                else {
                    std::vector<size_t> pc{lo};
                    while (pc.back() < lo + n) {
                        size_t nxt = lo + n;
                        if (lo + n - pc.back() > piece) {
                            size_t at = 0;
                            if (bsk_find_record_start(fmap, lo + n, pc.back() + piece, fmt, &at) == BSK_OK && at > pc.back() && at < lo + n && at - pc.back() <= piece + (64u << 20)) nxt = at;
                        }
                        pc.push_back(nxt);
                    }
                    auto read_piece = [&](size_t k) -> bool { return parallel_pread(fd, pin[k & 1], pc[k + 1] - pc[k], pc[k]); };
                    bool okr = read_piece(0);
                    for (size_t k = 0; k + 1 < pc.size() && okr && rc == BSK_OK; ++k) {
                        std::future<bool> next;
                        if (k + 2 < pc.size()) next = std::async(std::launch::async, read_piece, k + 1);
                        rc = bsk_stats_run(ctx, pin[k & 1], pc[k + 1] - pc[k], 0, fmt, (int64_t)rank * 1000000 + (int64_t)k, nullptr, nullptr);
                        if (next.valid()) okr = next.get();
                    }
                    if (!okr && rc == BSK_OK) { rc = BSK_ERR_INVALID_ARG; give_up("short read of " + path); }
                    mark("shard streamed from the file", rank);
                }
                if (fmap != MAP_FAILED) munmap((void*)fmap, size);
                for (uint8_t* q : pin) if (q) bsk_host_free(q);
            }
            if (ok0 && rc != BSK_OK) give_up(bsk_last_error(ctx));
            uint64_t bad = (uint64_t)failed.load();
            if (bsk_count_allreduce(comm, &bad, nullptr) != BSK_OK) { give_up(bsk_comm_error(comm)); return; }
            if (bad) return;  // (somebody failed before the reduction: nobody enters it)
            rc = bsk_stats_collect_reduced(ctx, comm, nullptr, nullptr, keys.data(), vals.data(), keys.size(), &cnt);
            if (rc != BSK_OK) { give_up(bsk_last_error(ctx)); }
            else if (rank == 0) {
                bsk_statinfo info;
                bsk_stats_finalize(ctx, keys.data(), vals.data(), cnt, &info);
                std::vector<char> buf(1 << 16);
                if (bsk_stats_string(ctx, "input0", "N/A", &info, buf.data(), buf.size()) != BSK_OK) give_up(bsk_last_error(ctx));
                else {
                    const std::string table = buf.data();
                    const size_t nl = table.find('\n');
                    me.text = table.substr(0, nl + 1) + table.substr(nl + 1) + "\n";  // (head + Join(lines[1:]) + "\n", as the single-device CLI)
                }
            }
        } else if (grep_count) {
            uint64_t cnt = 0;
            if (ok0) {
                bsk_out o;
                if (bsk_grep_run(ctx, d_shard, n, 1, fmt, rank, nullptr, &o) != BSK_OK || bsk_grep_last_count(ctx, &cnt) != BSK_OK) give_up(bsk_last_error(ctx));
            }
            uint64_t bad = (uint64_t)failed.load();
            if (bsk_count_allreduce(comm, &bad, nullptr) != BSK_OK) { give_up(bsk_comm_error(comm)); return; }
            if (!bad) {
                if (bsk_count_allreduce(comm, &cnt, nullptr) != BSK_OK) give_up(bsk_comm_error(comm));
                else if (rank == 0) me.text = std::to_string(cnt);  // fmt.Print: no newline (bigseqkit-cli/grep.go:14)
            }
        } else {
            // sample: the verdict on a record hangs on its index in the WHOLE file -- every worker counts its shard, the counts
            // are gathered, the prefix is this worker's first record and the sum serves -n (bigseqkit/sample.go:67-73)
            uint64_t first_record = 0;
            if (use == "sample") {
                int needs = 0;
                if (ctx) bsk_sample_needs_count(ctx, &needs);
                if (needs || world > 1) {  // (the same on every worker: all of them enter the collective, or none)
                    uint64_t k = 0;
                    if (me.error.empty() && via_host)
                        give_up(needs ? "sample -n (--number) needs the record count of the whole input before the first record is judged, and this "
                                        "input is streamed from the file in pieces: use -p (--proportion), as the command's own help advises "
                                        "for large files"
                                      : "sample: a shard that is streamed from the file in pieces is not counted first; run it on one worker "
                                        "(--devices N) or on more devices, so that every shard fits its GPU");
                    else if (me.error.empty() && n && bsk_index_build(ctx, d_shard, n, 1, fmt, nullptr, &k) != BSK_OK) give_up(bsk_last_error(ctx));
                    std::vector<uint64_t> all((size_t)world, 0);
                    if (bsk_comm_allgather_u64(comm, k, all.data(), nullptr) != BSK_OK) give_up(bsk_comm_error(comm));
                    uint64_t total = 0;
                    for (int r = 0; r < world; ++r) { if (r < rank) first_record += all[(size_t)r]; total += all[(size_t)r]; }
                    if (me.error.empty() && needs && bsk_sample_set_count(ctx, total) != BSK_OK) give_up(bsk_last_error(ctx));
                }
                if (me.error.empty()) bsk_sample_set_first_record(ctx, first_record);  // (where bsk_run_to_store starts counting)
            }
            bsk_store* st = dir_store;
            uint64_t part = (uint64_t)rank;
            if (ok0 && !dir_store) {  // --merge / -o -: this worker's part goes to a spool file of its own first
                char nm[96];
                snprintf(nm, sizeof nm, ".bsk-%s-part%05d.tmp", token, rank);
                me.spool = (to_stdout ? std::string(getenv("TMPDIR") ? getenv("TMPDIR") : "/tmp") + "/bsk-stdout" : out_file) + nm;
                const int tfd = open(me.spool.c_str(), O_CREAT | O_EXCL | O_WRONLY, 0600);  // (never through a planted link)
                if (tfd < 0) give_up("cannot create " + me.spool);
                else {
                    close(tfd);
                    if (bsk_store_open(me.spool.c_str(), 1, &own) != BSK_OK) give_up("cannot create " + me.spool);
                    else bsk_store_set_bgzf(own, bgzf ? 2 : 0);  // (a spool is a piece: no EOF block, the parent appends the one)
                    st = own;
                    part = 0;
                }
            }
            if (use == "rmdup") {
                bsk_out o{nullptr, 0, 0};
                uint64_t bad = (uint64_t)failed.load();
                if (bsk_count_allreduce(comm, &bad, nullptr) != BSK_OK) { give_up(bsk_comm_error(comm)); bad = 1; }
                if (!bad) {
                    if (bsk_rmdup_dist_run(ctx, comm, d_shard, n, fmt, nullptr, &o) != BSK_OK) give_up(bsk_last_error(ctx));
                    else if (bsk_store_put(st, ctx, part, &o) != BSK_OK) give_up(bsk_store_error(st));
                    me.out_bytes = o.len; me.out_records = o.records;
                }
            } else if (me.error.empty() && via_host) {
                // A shard that does not fit the GPU next to its result: pieces of ~2 GiB that end on record starts (found on a
                // mapping of the file: only the pages around the cuts are touched) go through bsk_run_to_store one after the
                // other -- inside, 256 MiB chunks cross PCIe under the kernels and the drain of the chunk before -- while a
                // reader thread fills the other pinned buffer.  The pieces are the parts 0, 1, 2 ... of ONE file: this worker's
                // spool (--merge / -o -) or its part%05d of the directory, written through a store of its own.
                bsk_store* mine = own;
                uint64_t p0 = 0;
                if (!mine) {
                    char nm[64];
                    snprintf(nm, sizeof nm, "/part%05d%s", rank, part_suffix(bgzf));
                    if (bsk_store_open((out_file + nm).c_str(), 1, &mine) != BSK_OK) give_up("cannot create " + out_file + nm);
                    else bsk_store_set_bgzf(mine, bgzf);
                }
                const size_t piece = std::max<size_t>(1 << 16, getenv("BSK_STREAM_PIECE_BYTES") ? (size_t)strtoull(getenv("BSK_STREAM_PIECE_BYTES"), nullptr, 10) : ((size_t)2 << 30));
                const uint8_t* fmap = (const uint8_t*)mmap(nullptr, size, PROT_READ, MAP_SHARED, fd, 0);
                uint8_t* pin[2] = {(uint8_t*)bsk_host_alloc(piece + (64 << 20)), (uint8_t*)bsk_host_alloc(piece + (64 << 20))};
                if (me.error.empty() && (fmap == MAP_FAILED || !pin[0] || !pin[1])) give_up("no pinned memory / mapping for the streamed shard");
                if (me.error.empty()) {
                    bsk_ctx_set(ctx, "pin_alphabet", "1");  // (one partition through several calls: one alphabet guess)
                    std::vector<size_t> pc{lo};
                    while (pc.back() < lo + n) {
                        size_t nxt = lo + n;
                        if (lo + n - pc.back() > piece) {
                            size_t at = 0;
                            if (bsk_find_record_start(fmap, lo + n, pc.back() + piece, fmt, &at) == BSK_OK && at > pc.back() && at < lo + n && at - pc.back() <= piece + (64u << 20)) nxt = at;
                        }
                        pc.push_back(nxt);
                    }
                    auto read_piece = [&](size_t k) -> bool { return parallel_pread(fd, pin[k & 1], pc[k + 1] - pc[k], pc[k]); };
                    bool okr = read_piece(0);
                    for (size_t k = 0; k + 1 < pc.size() && okr && me.error.empty(); ++k) {
                        std::future<bool> next;
                        if (k + 2 < pc.size()) next = std::async(std::launch::async, read_piece, k + 1);
                        uint64_t ob = 0, orec = 0;
                        // (pid: the header row of `locate` belongs to the first chunk of partition 0 -- the first piece of worker 0 only)
                        const int64_t pid = (rank == 0 && k == 0) ? 0 : (int64_t)rank * 1000000 + (int64_t)k + 1;
                        if (bsk_run_to_store(ctx, pin[k & 1], pc[k + 1] - pc[k], fmt, pid, mine, p0 + k, &ob, &orec) != BSK_OK) give_up(bsk_last_error(ctx));
                        me.out_bytes += ob; me.out_records += orec;
                        if (next.valid()) okr = next.get();
                    }
                    if (!okr) give_up("short read of " + path);
                    mark("shard streamed through the host pipeline", rank);
                }
                if (fmap != MAP_FAILED) munmap((void*)fmap, size);
                for (uint8_t* q : pin) if (q) bsk_host_free(q);
                if (mine && mine != own) { uint64_t tot = 0; if (bsk_store_close(mine, &tot) != BSK_OK) give_up("closing this worker's part failed"); }
            } else if (me.error.empty()) {
                // the shard is on the device: one call over all of it, its output drained in pieces (bsk_store_put: the
                // copy of a piece runs while the piece before it is written)
                Part in;
                in.fmt = fmt; in.dptr = d_shard; in.n = n;
                bsk_out o{nullptr, 0, 0};
                if (n && run_op(use, ctx, in, rank, first_record, &o) != BSK_OK) give_up(bsk_last_error(ctx));
                else if (bsk_store_put(st, ctx, part, &o) != BSK_OK) give_up(bsk_store_error(st));
                me.out_bytes = o.len; me.out_records = o.records;
            }
            if (own) {
                uint64_t tot = 0;
                if (bsk_store_close(own, &tot) != BSK_OK) give_up("closing " + me.spool + " failed");
            }
        }
        mark("command done", rank);
        if (d_shard) bsk_device_free(d_shard);
        if (h) bsk_host_free(h);
        if (ctx) bsk_destroy(ctx);
        mark("released", rank);
    };
    std::vector<std::thread> threads;
    for (int r = 0; r < world; ++r) threads.emplace_back(work, r);
    for (auto& t : threads) t.join();
    for (auto* c : comms) bsk_comm_destroy(c);
    mark("communicators destroyed");
    close(fd);
    uint64_t tot = 0;
    if (dir_store && bsk_store_close(dir_store, &tot) != BSK_OK) { W[0].error = "closing the output failed"; failed.fetch_add(1); }
    auto drop_spools = [&] { for (auto& w : W) if (!w.spool.empty()) unlink(w.spool.c_str()); };
    if (failed.load()) {
        drop_spools();
        for (int r = 0; r < world; ++r)
            if (!W[(size_t)r].error.empty()) die("worker " + std::to_string(r) + " (device " + std::to_string(devices[(size_t)r]) + "): " + W[(size_t)r].error);
        die("a worker failed");
    }
    if (!records) {
        size_t w = 0;
        while (w < W[0].text.size()) {
            const ssize_t k = write(real_out, W[0].text.data() + w, W[0].text.size() - w);
            if (k <= 0) die("write to the standard output failed");
            w += (size_t)k;
        }
        return 0;
    }
    if (dir_store) {
        for (int r = 0; r < world; ++r)  // (an empty part file still marks the partition, as SaveAsTextFile does)
            if (W[(size_t)r].out_bytes == 0) {
                char nm[64];
                snprintf(nm, sizeof nm, "/part%05d%s", r, part_suffix(bgzf));
                // (O_TRUNC: a non-empty part of an earlier run into the same directory must not pass for this run's -- ADVICE r05)
                const int e = open((out_file + nm).c_str(), O_CREAT | O_TRUNC | O_WRONLY, 0644);
                if (e >= 0 && bgzf && write(e, eof_block().data(), 28) != 28) die("write " + out_file + nm + " failed");
                if (e >= 0) close(e);
            }
        return 0;
    }
    // ---- one file (or stdout): the parts in rank order == file order (FileStore's order)
    const int dst = to_stdout ? real_out : open(out_file.c_str(), O_CREAT | O_TRUNC | O_WRONLY, 0644);
    if (dst < 0) { drop_spools(); die("cannot create " + out_file); }
    bool okw = true;
    std::vector<char> buf(8u << 20);
    for (int r = 0; r < world && okw; ++r) {
        const int src = open(W[(size_t)r].spool.c_str(), O_RDONLY);
        if (src < 0) { okw = false; break; }
        for (;;) {
            const ssize_t k = read(src, buf.data(), buf.size());
            if (k < 0) { okw = false; break; }
            if (k == 0) break;
            ssize_t w = 0;
            while (w < k) { const ssize_t x = write(dst, buf.data() + w, (size_t)(k - w)); if (x <= 0) { okw = false; break; } w += x; }
            if (!okw) break;
        }
        close(src);
    }
    if (okw && bgzf && write(dst, eof_block().data(), 28) != 28) okw = false;  // (the spools are BGZF without it: the ONE EOF block)
    if (!to_stdout && close(dst) != 0) okw = false;
    drop_spools();
    if (!okw) die("write " + out_file + " failed");
    return 0;
}

}  // namespace

static int run_main(int argc, char** argv) {
    if (argc < 2 || !strcmp(argv[1], "-h") || !strcmp(argv[1], "--help")) { usage(); return argc < 2; }
    std::vector<std::string> args(argv + 1, argv + argc);
    if (args[0] == "pipe") {
        // bigseqkit pipe --job job.json [files...] [-o out] [--merge] ...   (bigseqkit-cli/pipe.go:42-67)
        std::string job;
        std::vector<std::string> rest{"seq"};  // the persistent flags are parsed with any command table
        for (size_t i = 1; i < args.size(); ++i) {
            if (args[i] == "--job" && i + 1 < args.size()) job = args[++i];
            else if (args[i].rfind("--job=", 0) == 0) job = args[i].substr(6);
            else rest.push_back(args[i]);
        }
        if (job.empty()) die("job not defined");
        Invocation inv = parse_invocation(rest);
        bsk::json::ValuePtr j;
        try {
            const std::string text = read_file(job);
            j = bsk::json::Parser(text).parse();
        } catch (const std::exception&) { die("incorrect job format"); }
        g_pipe_job = true;
        Output o = run_job(*j, true);
        g_pipe_job = false;
        // the files given to `pipe` itself are appended unchanged (pipe.go:61-66)
        for (auto& p : read_parts(classify_inputs(inv.files))) o.text += p.host;
        store(inv, o, inv.files);
        return 0;
    }
    Invocation inv = parse_invocation(args);
    bool faidx_query = false;
    if (std::string(inv.cmd->use) == "faidx") {
        // cli/faidx.go: the first argument is the file, the others are regions ("id", "id:b-e", ...)
        std::string regions;
        for (size_t k = 1; k < inv.files.size(); ++k) regions += (k > 1 ? "," : "") + jquote(inv.files[k]);
        if (inv.files.size() > 1) inv.files.resize(1);
        inv.js.insert(inv.js.rfind('}'), ",\"Regions\":[" + regions + "]");
        faidx_query = !regions.empty() || !inv.pget("region-file").empty();
    }
    if (inv.pget("dry-run") == "true") {
        std::cout << inv.cmd->op << "\n" << inv.js << "\n";
        for (auto& f : inv.files) std::cout << f << "\n";
        return 0;
    }
    if (inv.pget("plan") == "true") {
        // what the multi-GPU launcher needs to know, decided by THIS program's flag tables (no second parser in Python)
        std::string files;
        for (size_t k = 0; k < inv.files.size(); ++k) files += (k ? "," : "") + jquote(inv.files[k]);
        std::cout << "{\"use\":" << jquote(inv.cmd->use) << ",\"op\":" << jquote(inv.cmd->op) << ",\"opts\":" << inv.js
                  << ",\"files\":[" << files << "],\"out_file\":" << jquote(inv.pget("out-file"))
                  << ",\"merge\":" << (inv.pget("merge") == "true" ? "true" : "false")
                  << ",\"partitions\":" << strtol(inv.pget("partitions").c_str(), nullptr, 10) << "}\n";
        return 0;
    }
    if (std::string(inv.cmd->use) == "sample" && inv.files.size() > 1) die("only 1 file needed");  // cli/sample.go:11-13
    if (std::string(inv.cmd->use) == "head-genome" && !inv.pget("devices").empty())
        die("'head-genome' runs on one device (bigseqkit head-genome ... --device N): the cut is sequential over the whole input, "
            "a worker could not judge its shard before the shards in front of it are done, so --devices is refused");
    // faidx -d IDX applies to a run with regions only (PARITY.md FAIX); what it refuses is decided here, on the flags
    const std::string faidx_idx = faidx_query ? inv.pget("index-file") : std::string();
    if (!faidx_idx.empty() && !inv.pget("devices").empty()) die(kFaidxIndexDevices);
    if (!inv.pget("devices").empty()) return run_devices(inv);  // several GPUs: worker threads + librccl, in this process
    if (inv.files.empty()) die("no input files (stdin is not supported by the IgnisHPC CLI either)");
    const std::vector<Input> ins = classify_inputs(inv.files);
    admit(ins, Route::Any);  // (gzip that is not BGZF is read by no path without the switch: said before a device is touched)
    g_faidx_query = faidx_query;
    bool faidx_idx_present = false;
    if (!faidx_idx.empty()) {
        if (ins[0].kind == kGzip)
            die(ins[0].path + " is gzip but not BGZF: faidx -d addresses bases by their offsets, and a gzip stream has none to enter at; "
                "recompress it with bgzip (gzip -dc FILE | bgzip > FILE.gz), or run without -d");
        struct stat sb;
        faidx_idx_present = stat(faidx_idx.c_str(), &sb) == 0;
        if (faidx_idx_present && (inv.val.scalar.count("id-regexp") || inv.pget("id-ncbi") == "true"))
            die("faidx: -d with the present index " + faidx_idx + " and --id-regexp / --id-ncbi is refused: the names of an index are those of the "
                "default ID rule and cannot restate another one; run without -d");
        if (faidx_idx_present && !ins[0].regular) die("faidx: -d needs a file it can read at offsets: " + ins[0].path);
    }
    const std::string use_cmd = inv.cmd->use;
    const bool joins_on_host = use_cmd == "concat" || use_cmd == "common" || use_cmd == "pair";
    if (!joins_on_host && bsk_device_count() <= 0) die("no HIP device visible (the hot path has no CPU fallback)");
    if (use_cmd == "head-genome") {
        Output o = run_head_genome(inv);
        store(inv, o, inv.files);
        return 0;
    }
    if (faidx_idx_present) {
        Output o = run_faidx_fetch(inv, ins[0], faidx_idx);
        store(inv, o, inv.files);
        return 0;
    }
    if (bucket_budget(use_cmd) > 0) {  // (shuffle, sort, rmdup, rename, common, pair, concat)
        // more bytes than a bucket may hold: not loaded whole (a pipe has no size: it takes the whole-file path)
        uint64_t total = 0;
        for (auto& in : ins)
            if (in.regular) total += in.size;
        if (total > bucket_budget(use_cmd)) {
            Output o = run_buckets(inv, ins);
            if (use_cmd != "pair" && !o.stored) store(inv, o, inv.files);  // (pair has written its four files, concat its shares)
            return 0;
        }
    }
    std::vector<Part> inputs = read_parts(ins, joins_on_host ? -1 : (int)strtol(inv.pget("device").c_str(), nullptr, 10), use_cmd);
    if (g_buckets_unfit) {
        Output o = run_buckets(inv, ins);
        store(inv, o, inv.files);
        return 0;
    }
    if (std::string(inv.cmd->use) == "concat") {
        if (inputs.size() != 2) die("2 files needed");
        if (inputs[0].fmt != inputs[1].fmt) die("concat: inputs of different formats");
        std::string both = inputs[0].host;
        if (!both.empty() && both.back() != '\n') both += '\n';
        const size_t n_first = both.size();
        both += inputs[1].host;
        bsk_ctx* c = nullptr;
        const int device = (int)strtol(inv.pget("device").c_str(), nullptr, 10);
        if (bsk_create("Concat", inv.js.c_str(), device, &c) != BSK_OK) die(bsk_global_error());
        bsk_out out;
        const int crc = bsk_concat_run(c, both.data(), both.size(), n_first, 0, inputs[0].fmt, nullptr, &out);
        if (crc == BSK_ERR_HIP)
            die(std::string(bsk_last_error(c)) + " -- 'concat': both files (" + std::to_string(both.size()) + " bytes) must fit one GPU next to their grouping tables and "
                "the output; BSK_CONCAT_BUDGET_BYTES=<bytes> matches them in buckets of the key that hold at most that many bytes of IDs, and joins them in "
                "windows of file 1 whose records, their mates of file 2 and their joined records are bounded by that many bytes");
        if (crc != BSK_OK) die(bsk_last_error(c));
        Output o;
        o.fmt = inputs[0].fmt;
        o.packed = packs_on_device(inv);
        append_result(c, out, o.text, o.packed);
        bsk_destroy(c);
        store(inv, o, inv.files);
        return 0;
    }
    if (std::string(inv.cmd->use) == "common") {
        // cli/common.go: at least two files; the records of the first one that are common to all
        if (inputs.size() < 2) die("at least 2 files needed");
        std::string all;
        std::vector<uint64_t> ends;
        for (auto& p : inputs) {
            if (p.fmt != inputs[0].fmt) die("common: inputs of different formats");
            all += p.host;
            if (!p.host.empty() && p.host.back() != '\n') all += '\n';
            ends.push_back(all.size());
        }
        bsk_ctx* c = nullptr;
        const int device = (int)strtol(inv.pget("device").c_str(), nullptr, 10);
        if (bsk_create("Common", inv.js.c_str(), device, &c) != BSK_OK) die(bsk_global_error());
        bsk_out out;
        if (bsk_common_run(c, all.data(), all.size(), ends.data(), (uint32_t)ends.size(), 0, inputs[0].fmt, nullptr, &out) != BSK_OK)
            die(bsk_last_error(c));
        Output o;
        o.fmt = inputs[0].fmt;
        o.packed = packs_on_device(inv);
        append_result(c, out, o.text, o.packed);
        bsk_destroy(c);
        store(inv, o, inv.files);
        return 0;
    }
    if (std::string(inv.cmd->use) == "pair") {
        // cli/pair.go:13-66: two files; <out-dir>/paired.1, paired.2 and, with -u, unpaired.1, unpaired.2
        if (inputs.size() < 2) die("2 files needed");
        const std::string outdir = inv.pget("out-dir");
        if (outdir.empty()) die("out-dir required");
        if (inputs[0].fmt != inputs[1].fmt) die("pair: inputs of different formats");
        if (!is_dir(outdir) && mkdir(outdir.c_str(), 0755) != 0) die("cannot create directory " + outdir);
        std::string both = inputs[0].host;
        if (!both.empty() && both.back() != '\n') both += '\n';
        const size_t n_first = both.size();
        both += inputs[1].host;
        bsk_ctx* c = nullptr;
        const int device = (int)strtol(inv.pget("device").c_str(), nullptr, 10);
        if (bsk_create("Pair", inv.js.c_str(), device, &c) != BSK_OK) die(bsk_global_error());
        bsk_out outs[4];
        const int prc = bsk_pair_run(c, both.data(), both.size(), n_first, 0, inputs[0].fmt, nullptr, outs);
        if (prc == BSK_ERR_HIP)
            die(std::string(bsk_last_error(c)) + " -- 'pair': both files (" + std::to_string(both.size()) + " bytes) must fit one GPU next to their grouping tables and "
                "the four outputs; BSK_PAIR_BUDGET_BYTES=<bytes> pairs them in buckets of the key that hold at most that many bytes of IDs, and prints "
                "paired.2 in buckets of at most that many bytes of text when file 2 is not in the order of its mates");
        if (prc != BSK_OK) die(bsk_last_error(c));
        const char* names[4] = {"paired.1", "paired.2", "unpaired.1", "unpaired.2"};
        const bool unp = inv.pget("save-unpaired") == "true";
        for (int k = 0; k < (unp ? 4 : 2); ++k) {
            std::string text(outs[k].len, '\0');
            if (outs[k].len && bsk_out_to_host(c, &outs[k], &text[0], text.size()) != BSK_OK) die(bsk_last_error(c));
            std::ofstream f(outdir + "/" + names[k], std::ios::binary);
            if (!f) die("cannot create " + outdir + "/" + names[k]);
            f.write(text.data(), (std::streamsize)text.size());
            f.close();
            if (!f) die("write " + outdir + "/" + names[k] + " failed");
        }
        bsk_destroy(c);
        return 0;
    }
    Output o = execute(inv, inputs, false);
    if (!faidx_idx.empty() && !inputs.empty()) write_faidx_index(inv, inputs[0], faidx_idx);
    store(inv, o, inv.files);
    return 0;
}

// a crash names its frames on stderr (the tests show stderr when a run fails) instead of leaving a bare signal number
static void on_crash(int sig) {
    static const char msg[] = "bigseqkit: fatal signal, frames:\n";
    if (write(2, msg, sizeof msg - 1) < 0) {}
    void* frames[64];
    const int n = backtrace(frames, 64);
    backtrace_symbols_fd(frames, n, 2);
    signal(sig, SIG_DFL);
    raise(sig);
}

int main(int argc, char** argv) {
    signal(SIGSEGV, on_crash);
    signal(SIGBUS, on_crash);
    signal(SIGABRT, on_crash);
    leave(run_main(argc, argv));
}
