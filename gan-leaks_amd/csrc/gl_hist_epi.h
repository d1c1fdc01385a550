// The histogram epilogue of the exact-integer pair loop (gl_hist.hip): every pair lands somewhere, unlike gl_count_epi.h, which is written
// for the sparse case.  For a window (lo, shift, n_bins):  hist[b] += #{ pairs : lo <= S and (S - lo) >> shift == b },  b < n_bins.
//
//   1. every lane holds the exact S of its pairs in its accumulator registers (formed in place by the kernel) and tests each against the
//      window.  A workgroup without a pair inside (__syncthreads_or) returns: at the refined levels of a radix-select almost all do.
//   2. a table unsigned [n_bins] in LDS (the slice buffers are free after the K loop; a tile holds at most 65 536 pairs) takes the lanes'
//      pairs: one LDS atomic per in-window pair.
//   3. the workgroup adds ONE value per non-zero bin to hist[b] (64-bit atomicAdd).
// Integer adds commute: the histogram is a function of the multiset of pair distances, whatever the tile, the chunking or the sharding.
// Rows clamped into a ragged last tile and queries beyond nq are masked (they are duplicates of the last valid row).
#pragma once
#include "gl_common.h"
#include "gl_count_epi.h"

namespace gl_hist {

// the window of one launch in the type S has in the kernel: the pairs with lo <= S <= hi, hi = lo + (n_bins << shift) - 1 clamped to the
// largest value of the type (filled in by the host); lo <= the largest S there is (the host returns early otherwise)
template <typename ST> struct hist_args {
    ST lo, hi;
    int shift, n_bins;   // 0 <= shift <= 40, 1 <= n_bins <= GL_HIST_MAX_BINS
};

// NI: 16-row groups of bank rows per wave (4 or 8).  s_of(i, j, r): S of the lane's bank row i * 16 + r (valid while < n_left) and its query
// column j (query qcol0 + j * 16 + (lane & 15) of the tile, valid while < q_left).  Every thread of the workgroup must call this (barriers);
// smem must hold a.n_bins words and be free.
// FRESH: the second pass compares against copies of lo and hi the compiler cannot see through.  Otherwise it keeps the NI * 16 lane masks
// of the first pass in scalar registers for the second, hundreds of them, which are spilled to lanes of vector registers set aside for the
// whole kernel: the kernels on gl_pair256::mainloop at 8 accumulator rows have none to give without spilling inside their K loop.
template <int NI, typename ST, bool FRESH = false, typename SOf>
__device__ __forceinline__ void hist_epilogue(SOf s_of, int n_left, int qcol0, int q_left, const hist_args<ST> &a,
                                              unsigned long long *__restrict__ hist, char *smem, int lane)
{
    const int frow = lane & 15;
    ST lo = a.lo, hi = a.hi;
    const int shift = a.shift;
    unsigned rvalid = 0;                                  // bit i * 4 + r: the bank row is a real one
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) rvalid |= (i * 16 + r < n_left ? 1u : 0u) << (i * 4 + r);
    // two compares per pair here; the bin is formed below, only for the pairs inside and one at a time, so that no second value per pair
    // has to stay live next to the accumulators
    auto inside = [&](int i, int j, int r, bool qvalid) -> bool {
        const ST s = s_of(i, j, r);
        return qvalid && ((rvalid >> (i * 4 + r)) & 1u) && s >= lo && s <= hi;
    };
    int hit = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool qvalid = qcol0 + j * 16 + frow < q_left;
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) hit |= inside(i, j, r, qvalid) ? 1 : 0;
    }
    // (also the barrier after which the slice buffers may be overwritten)
    if (!__syncthreads_or(hit)) return;

    if constexpr (FRESH) asm volatile("" : "+s"(lo), "+s"(hi));
    unsigned *tab = reinterpret_cast<unsigned *>(smem);   // [n_bins]; at most 65 536 per entry
    for (int e = threadIdx.x; e < a.n_bins; e += blockDim.x) tab[e] = 0u;
    __syncthreads();
    if (hit) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool qvalid = qcol0 + j * 16 + frow < q_left;
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (!inside(i, j, r, qvalid)) continue;
                    // (64-bit shift: `shift` may exceed the width of a 32-bit S; the bin is below n_bins because S <= hi)
                    atomicAdd(&tab[(unsigned)((unsigned long long)(ST)(s_of(i, j, r) - lo) >> shift)], 1u);
                }
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < a.n_bins; e += blockDim.x) {
        const unsigned c = tab[e];
        if (c != 0u) atomicAdd(&hist[e], (unsigned long long)c);
    }
}

}  // namespace gl_hist
