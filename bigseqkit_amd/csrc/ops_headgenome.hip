// head-genome: the verdict passes over the record table (see ops_headgenome.hpp).  One lane per record; a lane reads its
// header line and the prefix words (a few dozen bytes that every lane shares, so they stay in cache).  The reduction is a
// minimum per wave (shuffles), per block (LDS, 64 bytes) and one atomicMin per block and result word.
#include <hip/hip_runtime.h>

#include "anchor.hpp"
#include "ops_headgenome.hpp"
#include "text_dev.hpp"

namespace bsk {
namespace {

__device__ __forceinline__ bool hg_blank(uint8_t c) { return c == ' ' || c == '\t'; }

// Desc of record i (parseHeadIDAndDesc, helper.go:329-369): length, *doff = where it begins inside the header text `h`
__device__ __forceinline__ uint32_t hg_desc(const RecordTable& t, uint64_t i, const uint8_t* h, uint32_t n, int id_mode, const uint8_t* lim,
                                            uint32_t* doff) {
    uint32_t ioff;
    const uint32_t il = id_span_rec(t, i, h, n, id_mode, &ioff, lim);
    *doff = n;
    return ioff == 0 ? desc_of(h, n, id_mode, il, doff) : 0u;
}

__global__ __launch_bounds__(256) void k_hg_counts(const uint8_t* __restrict__ buf, uint64_t buf_n, RecordTable t, uint64_t n_use, int id_mode,
                                                   HgPrefix P, uint64_t skip, uint32_t* __restrict__ counts) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_use) return;
    const uint32_t lh = t.l_head[i];
    const uint8_t* h = buf + t.start[i] + 1;
    const uint32_t n = lh > 0 ? lh - 1 : 0;
    uint32_t p;
    const uint32_t dl = hg_desc(t, i, h, n, id_mode, buf + buf_n, &p);
    if (dl == 0) { counts[i] = HG_NO_DESC; return; }
    uint32_t k = 0;
    if (i != skip) {
        // stringutil.Split(Desc, "\t "): maximal runs of bytes other than ' ' and '\t'; the leading words equal to the prefix's
        while (k < P.nwords) {
            while (p < n && hg_blank(h[p])) ++p;
            if (p >= n) break;
            const uint32_t w0 = P.off[k], wl = P.off[k + 1] - w0;
            uint32_t j = 0;
            while (p + j < n && !hg_blank(h[p + j]) && j < wl && h[p + j] == P.bytes[w0 + j]) ++j;
            if (j != wl || (p + j < n && !hg_blank(h[p + j]))) break;  // a byte differs, or one word is longer than the other
            p += j;
            ++k;
        }
    }
    counts[i] = k;
}

__device__ __forceinline__ uint64_t wave_min(uint64_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t o = (uint64_t)__shfl_down((unsigned long long)v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(256) void k_hg_cut(const uint32_t* __restrict__ counts, uint64_t n_use, uint64_t first_cmp, int n1_known,
                                                uint32_t n1_in, uint32_t min_words, uint64_t* __restrict__ res) {
    __shared__ uint64_t s_min[2][4];
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t cut = HG_NONE, nd = HG_NONE;
    if (i < n_use) {
        const uint32_t ni = counts[i];
        if (ni == HG_NO_DESC) nd = i;
        else if (i >= first_cmp) {
            const uint32_t n1 = n1_known ? n1_in : counts[first_cmp];  // (first_cmp <= i < n_use)
            if (ni < min_words || ni != n1) cut = i;
        }
    }
    cut = wave_min(cut);
    nd = wave_min(nd);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { s_min[0][wave] = cut; s_min[1][wave] = nd; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            cut = s_min[0][w] < cut ? s_min[0][w] : cut;
            nd = s_min[1][w] < nd ? s_min[1][w] : nd;
        }
        if (cut != HG_NONE) atomicMin((unsigned long long*)&res[HG_CUT], (unsigned long long)cut);
        if (nd != HG_NONE) atomicMin((unsigned long long*)&res[HG_NODESC], (unsigned long long)nd);
    }
}

__global__ void k_hg_finish(const uint8_t* __restrict__ buf, RecordTable t, const uint32_t* __restrict__ counts, uint64_t n_use,
                            uint64_t first_cmp, int id_mode, uint64_t* __restrict__ res) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint64_t cut = res[HG_CUT], nd = res[HG_NODESC];
    res[HG_CUT_BYTE] = t.start[cut < n_use ? cut : n_use];  // (start[t.n] = the end of the last record)
    res[HG_N1] = first_cmp < n_use ? (uint64_t)counts[first_cmp] : HG_NONE;
    if (nd < n_use) {
        const uint32_t lh = t.l_head[nd];
        uint32_t ioff;
        const uint32_t il = id_span_rec(t, nd, buf + t.start[nd] + 1, lh > 0 ? lh - 1 : 0, id_mode, &ioff);
        res[HG_ND_START] = t.start[nd];
        res[HG_ND_LHEAD] = lh;
        res[HG_ND_IDOFF] = ioff;
        res[HG_ND_IDLEN] = il;
    }
}

__global__ void k_hg_fastq_start(const uint8_t* __restrict__ buf, uint64_t n, uint64_t from, uint64_t* __restrict__ res) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint64_t at = find_fastq_start(buf, n, from, from + ANCHOR_SEARCH_BYTES);
    res[HG_END] = at == ANCHOR_NONE ? n : at;
}

inline dim3 grid_of(uint64_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

hipError_t launch_hg_counts(const uint8_t* buf, uint64_t buf_n, const RecordTable& t, uint64_t n_use, int id_mode, const HgPrefix& P,
                            uint64_t skip, uint32_t* counts, hipStream_t st) {
    if (n_use == 0) return hipSuccess;
    hipLaunchKernelGGL(k_hg_counts, grid_of(n_use), dim3(256), 0, st, buf, buf_n, t, n_use, id_mode, P, skip, counts);
    return hipGetLastError();
}

hipError_t launch_hg_cut(const uint32_t* counts, uint64_t n_use, uint64_t first_cmp, int n1_known, uint32_t n1, uint32_t min_words,
                         uint64_t* res, hipStream_t st) {
    if (n_use == 0) return hipSuccess;
    hipLaunchKernelGGL(k_hg_cut, grid_of(n_use), dim3(256), 0, st, counts, n_use, first_cmp, n1_known, n1, min_words, res);
    return hipGetLastError();
}

hipError_t launch_hg_finish(const uint8_t* buf, const RecordTable& t, const uint32_t* counts, uint64_t n_use, uint64_t first_cmp,
                            int id_mode, uint64_t* res, hipStream_t st) {
    hipLaunchKernelGGL(k_hg_finish, dim3(1), dim3(64), 0, st, buf, t, counts, n_use, first_cmp, id_mode, res);
    return hipGetLastError();
}

hipError_t launch_hg_fastq_start(const uint8_t* buf, uint64_t n, uint64_t from, uint64_t* res, hipStream_t st) {
    hipLaunchKernelGGL(k_hg_fastq_start, dim3(1), dim3(64), 0, st, buf, n, from, res);
    return hipGetLastError();
}

}  // namespace bsk
