// The key of `sort` (PARITY.md SORT) as device code: where the string key of a record lives, the natural-order rewrite, and
// the canonical key -- a byte string, compared as bytes with the shorter one zero-padded -- as a view that hands out one byte
// at a time.  Shared by the radix passes (ops_sort.hip: k_sort_natlen / k_sort_natkeys / k_sort_keylen / k_sort_chunk) and the
// bucket passes (ops_sort_buckets.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "index.hpp"
#include "ops_sort.hpp"
#include "text_dev.hpp"

namespace bsk {

// where the string key of record i lives: head bytes [off, off + len) for modes 0 / 1, the sequence for mode 2
__device__ __forceinline__ uint32_t key_span(const uint8_t* __restrict__ buf, const RecordTable& t, const SortParams& P,
                                             uint64_t i, uint32_t* off) {
    *off = 0;
    if (P.mode == 2) {
        const uint32_t L = t.l_seq[i];
        return (P.prefix_len == 0 || L <= P.prefix_len) ? L : P.prefix_len;  // sort.go:74-87
    }
    const uint8_t* h = buf + t.start[i] + 1;
    const uint32_t lh = t.l_head[i];
    const uint32_t hl = lh > 0 ? lh - 1 : 0;
    if (P.mode == 1) return hl;                                  // record.Name
    return id_span_rec(t, i, h, hl, P.id_mode, off, P.buf_end);         // record.ID
}

// Natural order (natsort.Compare, PARITY.md SORT): the key is cut into runs of digits and runs of other bytes; digit runs
// compare as integers, other runs as strings, a key that runs out first comes first.  Rewritten so that plain byte order
// gives the same result:  digit run -> '0', number of significant digits, the significant digits;  other run -> its
// bytes (lower-cased with -i) and a 0 terminator.  One thread per record (keys are IDs / headers: short).
template <bool WRITE>
__device__ __forceinline__ uint32_t natural_key(const uint8_t* __restrict__ k, uint32_t len, bool fold, uint8_t* __restrict__ o) {
    uint32_t n = 0, i = 0;
    while (i < len) {
        if (k[i] >= '0' && k[i] <= '9') {
            uint32_t j = i;
            while (j < len && k[j] >= '0' && k[j] <= '9') ++j;
            uint32_t z = i;
            while (z + 1 < j && k[z] == '0') ++z;  // leading zeros do not count (an all-zero run keeps one '0')
            const uint32_t nd = j - z;
            if (WRITE) { o[n] = '0'; o[n + 1] = (uint8_t)(nd > 255u ? 255u : nd); for (uint32_t q = 0; q < nd; ++q) o[n + 2 + q] = k[z + q]; }
            n += 2 + nd;
            i = j;
        } else {
            while (i < len && !(k[i] >= '0' && k[i] <= '9')) {
                uint8_t c = k[i];
                if (fold && c >= 'A' && c <= 'Z') c += 32;
                if (WRITE) o[n] = c;
                ++n;
                ++i;
            }
            if (WRITE) o[n] = 0;
            ++n;
        }
    }
    return n;
}

// The canonical key of record i: `len` bytes, byte k = at(k).  String keys (modes 0..2) read the shard -- or the rewritten
// keys of -N -- and fold with -i; the integer keys (-l / -b, `num` = what k_sort_intkeys wrote) are 4 big-endian bytes.
// The ONE statement of the key bytes: k_sort_chunk packs them into its 8-byte radix chunks, the bucket passes compare them
// with splitters.
struct SortKeyView {
    Text T;          // the bytes: a sequence (mode 2; wrapped FASTA read in place, text_dev.hpp) or W = 0: head bytes / -N keys
    uint32_t len;
    uint32_t num;
    int kind;        // 0 bytes of T, 1 the 32-bit number
    int fold;
    __device__ __forceinline__ uint8_t at(uint32_t k) const {
        if (kind) return (uint8_t)(num >> (24u - 8u * k));
        uint8_t c = T.at(k);
        if (fold && c >= 'A' && c <= 'Z') c += 32;
        return c;
    }
};

__device__ __forceinline__ SortKeyView sort_key_view(const uint8_t* __restrict__ buf, const RecordTable& t, const TextTable& tt,
                                                     const SortParams& P, const uint64_t* __restrict__ int_keys, uint64_t i) {
    SortKeyView K;
    K.T.p = nullptr; K.T.L = 0; K.T.W = 0; K.len = 4; K.num = 0; K.kind = 0; K.fold = 0;
    if (P.mode >= 3) {
        K.kind = 1;
        K.num = (uint32_t)int_keys[i];
    } else if (P.nat) {
        K.T.p = P.nat + P.nat_off[i];  // already folded
        K.len = (uint32_t)(P.nat_off[i + 1] - P.nat_off[i]);
    } else if (P.mode == 2) {
        uint32_t off;
        K.T = text_of(buf, t, tt, i);
        K.len = key_span(buf, t, P, i, &off);
        K.fold = P.ignore_case;
    } else {
        uint32_t off;
        K.len = key_span(buf, t, P, i, &off);
        K.T.p = buf + t.start[i] + 1 + off;
        K.fold = P.ignore_case;
    }
    return K;
}

}  // namespace bsk
