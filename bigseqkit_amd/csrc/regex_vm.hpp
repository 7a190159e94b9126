// Regular expressions WITH positions: a Pike VM (Thompson program, thread lists in priority order) that finds the
// leftmost-first match and the bounds of capture group 1 -- what Go's regexp.FindSubmatch / FindSubmatchIndex return.
// Used where the reference needs more than "matches or not":
//   * custom --id-regexp: ID = FindSubmatch(head)[1]        (/root/reference/bigseqkit-lib/helper.go:362-368)
//   * locate -r with matches of variable length: FindSubmatchIndex in a loop (bigseqkit-lib/locate.go:583-667)
// The search routine is compiled for the host (bsk_create vets programs, CPU tests compare it with std::regex) and for
// the device (one lane per record; thread lists in private memory -- a rare path, not a fast one).
// Syntax: what regex_nfa.hpp parses (RE2 subset), plus capture groups and lazy quantifiers, which matter here.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define BSK_VM_HD __host__ __device__
#else
#define BSK_VM_HD
#endif

namespace bsk {

constexpr int VM_MAX_INST = 64;
constexpr int VM_MAX_SETS = 24;
enum : uint8_t { VM_CHAR = 0, VM_SPLIT = 1, VM_JMP = 2, VM_SAVE = 3, VM_BEGIN = 4, VM_END = 5, VM_MATCH = 6, VM_WORDB = 7, VM_NWORDB = 8 };

struct VmInst { uint8_t op, arg; uint8_t x, y; };  // CHAR: arg = set; SPLIT: x first (preferred), y second; JMP: x; SAVE: arg = slot
struct VmProgram {
    uint32_t n = 0;
    uint32_t ngroups = 0;  // capture groups in the expression (bounds are kept for groups 1..max_group of compile_vm)
    VmInst inst[VM_MAX_INST];
    uint32_t sets[VM_MAX_SETS][8];
};

// throws OptError (unsupported syntax, too many instructions / classes).  Bounds are recorded for groups 1..max_group
// (SAVE slots 2g, 2g + 1); `names` (optional) receives the name of every group, "" for unnamed ones, index 0 = the match.
VmProgram compile_vm(const std::string& expr, int max_group = 1, std::vector<std::string>* names = nullptr);

// leftmost-first match of the program in text[0, n), searching from `from` (^ matches at 0 only, $ at n only).
// caps[0..1] = bounds of the match, caps[2g..2g+1] = bounds of group g < NCAP / 2 (0xFFFFFFFF when it did not take part).
// (text(i): byte i of the target -- a plain pointer, a wrapped FASTA record, or the reverse complement read backwards)
// NCAP is the number of slots each thread carries: the thread lists live in private memory, so --id-regexp and locate
// keep 4; replace instantiates 8 or 20 only when its template asks for groups beyond 1.
template <int NCAP = 4, class TextFn>
BSK_VM_HD inline bool vm_search_fn(const VmProgram& P, const TextFn& text, uint32_t n, uint32_t from, uint32_t* caps) {
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    struct Th { uint8_t pc; uint32_t c[NCAP]; };
    Th la[VM_MAX_INST], lb[VM_MAX_INST];
    Th* cl = la;
    Th* nl = lb;
    uint32_t ncl = 0, nnl = 0;
    uint32_t mark[VM_MAX_INST];
    for (uint32_t i = 0; i < P.n; ++i) mark[i] = NONE;
    bool matched = false;
    Th stack[VM_MAX_INST];
    // addthread with an explicit stack: follows JMP / SPLIT / SAVE / assertions in priority order
    auto add = [&](Th* list, uint32_t& cnt, uint8_t pc0, const uint32_t* c0, uint32_t sp) {
        uint32_t top = 0;
        stack[top].pc = pc0;
        for (int k = 0; k < NCAP; ++k) stack[top].c[k] = c0[k];
        ++top;
        while (top) {
            Th t = stack[--top];
            for (;;) {
                if (mark[t.pc] == sp) break;
                mark[t.pc] = sp;
                const VmInst I = P.inst[t.pc];
                if (I.op == VM_JMP) { t.pc = I.x; continue; }
                if (I.op == VM_SPLIT) {
                    if (top < (uint32_t)VM_MAX_INST) { stack[top] = t; stack[top].pc = I.y; ++top; }  // the second branch waits
                    t.pc = I.x;
                    continue;
                }
                if (I.op == VM_SAVE) { if (I.arg < NCAP) t.c[I.arg] = sp; ++t.pc; continue; }
                if (I.op == VM_BEGIN) { if (sp != 0) break; ++t.pc; continue; }
                if (I.op == VM_END) { if (sp != n) break; ++t.pc; continue; }
                if (I.op == VM_WORDB || I.op == VM_NWORDB) {  // \b / \B: ASCII word characters [0-9A-Za-z_] (RE2)
                    auto word = [](uint8_t ch) { return (ch >= '0' && ch <= '9') || (ch >= 'a' && ch <= 'z') || (ch >= 'A' && ch <= 'Z') || ch == '_'; };
                    const bool before = sp > 0 && word(text(sp - 1)), after = sp < n && word(text(sp));
                    if ((before != after) != (I.op == VM_WORDB)) break;
                    ++t.pc;
                    continue;
                }
                list[cnt++] = t;  // CHAR or MATCH
                break;
            }
        }
    };
    uint32_t fresh[NCAP];
    for (int k = 0; k < NCAP; ++k) fresh[k] = NONE;
    for (uint32_t sp = from;; ++sp) {
        if (!matched) add(cl, ncl, 0, fresh, sp);  // a new attempt starts here, below every running one
        if (ncl == 0) {
            if (matched || sp >= n) break;
            continue;  // (an expression that can only begin further on, e.g. at the end of the text)
        }
        nnl = 0;
        for (uint32_t i = 0; i < ncl; ++i) {
            const Th t = cl[i];
            const VmInst I = P.inst[t.pc];
            if (I.op == VM_MATCH) {
                for (int k = 0; k < NCAP; ++k) caps[k] = t.c[k];
                matched = true;
                break;  // threads below this one are cut off
            }
            if (sp < n) {
                const uint8_t ch = text(sp);
                if ((P.sets[I.arg][ch >> 5] >> (ch & 31)) & 1u) {
                    // marks of step sp + 1: distinct from step sp because `mark` holds the step number
                    add(nl, nnl, (uint8_t)(t.pc + 1), t.c, sp + 1);
                }
            }
        }
        Th* tmp = cl; cl = nl; nl = tmp;
        ncl = nnl;
        if (sp >= n) break;
    }
    return matched;
}

BSK_VM_HD inline bool vm_search(const VmProgram& P, const uint8_t* text, uint32_t n, uint32_t from, uint32_t* caps) {
    return vm_search_fn(P, [text](uint32_t i) { return text[i]; }, n, from, caps);
}


// ---- replace (bigseqkit-lib/replace.go): Go's Regexp.ReplaceAll and Regexp.Expand, byte for byte, host and device.
// Sinks: out(c) receives every output byte; the size pass counts, the write pass stores.

// Regexp.Expand of template tp[0, tn) against one match: caps[2g], caps[2g + 1] = bounds of group g inside src
// (NONE: did not take part) for g < ncap / 2; groups up to `ngroups` exist.  group_of(name, len) -> group of that
// name or -1.  "$$" -> "$"; "$name" takes the longest run of [A-Za-z0-9_]; "${name}"; all digits (no leading zero) =
// a group number; a group that does not exist or did not take part expands to nothing; a malformed '$' stays.
template <class Src, class Names, class Out>
BSK_VM_HD inline void vm_expand(const uint8_t* tp, uint32_t tn, const Src& src, const uint32_t* caps, uint32_t ncap,
                                uint32_t ngroups, const Names& group_of, Out& out) {
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    auto word = [](uint8_t ch) { return (ch >= '0' && ch <= '9') || (ch >= 'a' && ch <= 'z') || (ch >= 'A' && ch <= 'Z') || ch == '_'; };
    uint32_t i = 0;
    while (i < tn) {
        const uint8_t ch = tp[i];
        if (ch != '$') { out(ch); ++i; continue; }
        ++i;
        if (i < tn && tp[i] == '$') { out((uint8_t)'$'); ++i; continue; }
        // extract()
        uint32_t j = i;
        const bool brace = j < tn && tp[j] == '{';
        if (brace) ++j;
        const uint32_t n0 = j;
        while (j < tn && word(tp[j])) ++j;
        const uint32_t nl = j - n0;
        bool ok = nl > 0;
        if (ok && brace) { if (j >= tn || tp[j] != '}') ok = false; else ++j; }
        if (!ok) { out((uint8_t)'$'); continue; }  // malformed: '$' as text, the rest is read again
        i = j;
        long long num = 0;
        for (uint32_t k = 0; k < nl; ++k) {
            const uint8_t d = tp[n0 + k];
            if (d < '0' || d > '9' || num >= 100000000ll) { num = -1; break; }
            num = num * 10 + (d - '0');
        }
        if (tp[n0] == '0' && nl > 1) num = -1;
        int g = num >= 0 ? (num <= (long long)ngroups ? (int)num : -1) : group_of(tp + n0, nl);
        if (g < 0 || 2u * (uint32_t)g + 1u >= ncap) continue;
        const uint32_t a = caps[2 * g], b = caps[2 * g + 1];
        if (a == NONE || b == NONE) continue;
        for (uint32_t k = a; k < b; ++k) out(src(k));
    }
}

// Regexp.ReplaceAll(text, template) (Go regexp.go replaceAll): the search restarts at searchPos with ^ and \b still
// seeing the whole text; an empty match right after the previous match inserts nothing (unless at 0); the search
// advances at least one byte.  Returns the number of matches (0: the text is unchanged).
template <int NCAP, class TextFn, class Names, class Out>
BSK_VM_HD inline uint32_t vm_replace_all(const VmProgram& P, const TextFn& text, uint32_t n, const uint8_t* tp, uint32_t tn,
                                         const Names& group_of, Out& out) {
    uint32_t caps[NCAP];
    uint32_t last = 0, pos = 0, hits = 0;
    while (pos <= n) {
        if (!vm_search_fn<NCAP>(P, text, n, pos, caps)) break;
        ++hits;
        for (uint32_t k = last; k < caps[0]; ++k) out(text(k));
        if (caps[1] > last || caps[0] == 0) vm_expand(tp, tn, text, caps, (uint32_t)NCAP, P.ngroups, group_of, out);
        last = caps[1];
        pos = pos + 1 > caps[1] ? pos + 1 : caps[1];
    }
    for (uint32_t k = last; k < n; ++k) out(text(k));
    return hits;
}

// Regexp.FindAllSubmatch(text, -1) up to two matches (Go regexp.go allMatches: an empty match right after the previous
// one is skipped).  Returns min(matches, 2); caps = the first one.
template <int NCAP, class TextFn>
BSK_VM_HD inline uint32_t vm_find_two(const VmProgram& P, const TextFn& text, uint32_t n, uint32_t* caps) {
    uint32_t c[NCAP];
    uint32_t pos = 0, found = 0;
    long long prev_end = -1;
    while (found < 2 && pos <= n) {
        if (!vm_search_fn<NCAP>(P, text, n, pos, c)) break;
        bool accept = true;
        if (c[1] == pos) {
            if ((long long)c[0] == prev_end) accept = false;
            pos = pos < n ? pos + 1 : n + 1;
        } else {
            pos = c[1];
        }
        prev_end = c[1];
        if (accept) {
            if (found == 0) for (int k = 0; k < NCAP; ++k) caps[k] = c[k];
            ++found;
        }
    }
    return found;
}

}  // namespace bsk
