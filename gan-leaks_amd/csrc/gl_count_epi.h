// The counting epilogue shared by the epsilon-ball count kernels: gl_count.hip (exact integer S, thresholds as unsigned / 64-bit integers)
// and gl_feat_count.hip (the fp32 distance of the l2-lpips search, thresholds as floats); a second form, further down, takes the thresholds of
// every query from device memory (gl_count_rows.hip).
//
//   1. every lane holds the distance of its pairs in its accumulator registers and tests it against thr[T-1] (the largest ball): one compare
//      per pair.  Almost every pair lies outside, so the rest is entered only by workgroups (__syncthreads_or) and waves (__any) that hold a hit.
//   2. per threshold t and query column j the lane counts its rows, the four lane groups that share a query column (lane >> 4) are folded with
//      __shfl_xor(.., 16) / (.., 32), and the lanes of group 0 add the wave's count into an LDS table [queries of the tile][T] (the slice
//      buffers are free after the K loop), which folds the waves that share a query.
//   3. the workgroup adds ONE value per (query, t) to counts[q][t] (64-bit atomicAdd), skipping zeros.
// Integer adds commute: the result is a function of the multiset of pair distances, whatever the tile, the chunking or the sharding.
// Rows clamped into a ragged last tile and queries beyond nq are masked (they are duplicates of the last valid row).
#pragma once
#include "gl_common.h"

namespace gl_count {

// thresholds of one launch: thr[0..n) ascending and non-negative, in the type the distance has in the kernel; column t of the launch is column
// col0 + t of the caller's counters (negative thresholds, which nothing meets, are dropped by the host), rows of `pitch` counters
template <typename ST> struct count_args {
    ST thr[GL_COUNT_MAX_T];
    int n, col0, pitch;
};

// rows / queries that are real ones, counted from `first`, as a small int (a tile has at most 256)
__device__ __forceinline__ int rows_left(int64_t total, int64_t first)
{
    const int64_t left = total - first;
    return left < 0 ? 0 : (left > 1024 ? 1024 : (int)left);
}

// NI: 16-row groups of bank rows per wave (4 or 8).  s_of(i, j, r): distance of the lane's bank row i * 16 + r (valid while < n_left) and its
// query column j (query qcol0 + j * 16 + (lane & 15) of the tile, valid while < q_left).  q0: first query of the tile; tile_q: queries per tile.
// Every thread of the workgroup must call this (barriers); smem must hold tile_q * a.n words and be free.
template <int NI, typename ST, typename SOf>
__device__ __forceinline__ void count_epilogue(SOf s_of, int n_left, int64_t q0, int qcol0, int q_left, int tile_q, const count_args<ST> &a,
                                               unsigned long long *__restrict__ counts, char *smem, int lane)
{
    const int frow = lane & 15, fk = lane >> 4;
    const ST top = a.thr[a.n - 1];
    unsigned rvalid = 0;                                  // bit i * 4 + r: the bank row is a real one
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) rvalid |= (i * 16 + r < n_left ? 1u : 0u) << (i * 4 + r);
    int hit = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool qvalid = qcol0 + j * 16 + frow < q_left;
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) hit |= (qvalid && ((rvalid >> (i * 4 + r)) & 1u) && s_of(i, j, r) <= top) ? 1 : 0;
    }
    // (also the barrier after which the slice buffers may be overwritten)
    if (!__syncthreads_or(hit)) return;

    unsigned *cnt = reinterpret_cast<unsigned *>(smem);   // [tile_q][a.n]; at most 256 per entry
    const int entries = tile_q * a.n;
    for (int e = threadIdx.x; e < entries; e += blockDim.x) cnt[e] = 0u;
    __syncthreads();
    if (__any(hit)) {
        for (int t = 0; t < a.n; ++t) {
            const ST th = a.thr[t];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned c = 0;
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) c += (((rvalid >> (i * 4 + r)) & 1u) && s_of(i, j, r) <= th) ? 1u : 0u;
                c += __shfl_xor(c, 16, 64);
                c += __shfl_xor(c, 32, 64);
                const int ql = qcol0 + j * 16 + frow;
                if (fk == 0 && c != 0u && ql < q_left) atomicAdd(&cnt[ql * a.n + t], c);
            }
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < entries; e += blockDim.x) {
        const unsigned c = cnt[e];
        const int ql = e / a.n, t = e - ql * a.n;
        if (c != 0u && ql < q_left) atomicAdd(&counts[(q0 + ql) * a.pitch + a.col0 + t], (unsigned long long)c);
    }
}

// ---- thresholds per query (gl_l2_count_rows_i8*): thr_dev[nq][n] int64 in DEVICE memory, ascending within each row; a negative threshold counts
// nothing, one >= s_max (= 65025 d, the largest S) every pair.  The counters have n columns.
struct rows_args {
    const long long *thr;
    long long s_max;
    int n;
};

// "S <= thr" as "S < bound": bound = clamp(thr, -1, s_max) + 1 in the unsigned type of S.  s_max + 1 fits: 65025 * 66051 + 1 < 2^32 in the
// 32-bit kernels, and the 64-bit ones have room to spare.
template <typename ST> __device__ __forceinline__ ST rows_bound(long long thr, long long s_max)
{
    return (ST)((thr < 0 ? -1ll : (thr > s_max ? s_max : thr)) + 1ll);
}

constexpr int ROWS_THR_OFFSET = 256 * GL_COUNT_MAX_T * 4;   // the bounds follow the largest counter table (256 queries x 16 x 4 bytes)

// The same epilogue with the thresholds of the lane's own query columns.  Step 1 tests each pair against the LAST threshold of its query (four
// bounds per lane, read from global memory once the accumulators hold S); workgroups and waves without a hit leave as above.  The others stage
// the tile's bounds into the slice buffers, turned to [t][query] so that the sixteen query columns of a read fall into sixteen banks (the four
// lane groups of a column read one address), and step 2 reads one bound per (t, j): no threshold stays live next to the accumulators.
// Queries beyond nq get the bound 0, which nothing meets.  smem must hold ROWS_THR_OFFSET + tile_q * a.n * sizeof(ST) bytes and be free.
template <int NI, typename ST, typename SOf>
__device__ __forceinline__ void count_epilogue(SOf s_of, int n_left, int64_t q0, int qcol0, int q_left, int tile_q, const rows_args &a,
                                               unsigned long long *__restrict__ counts, char *smem, int lane)
{
    const int frow = lane & 15, fk = lane >> 4;
    unsigned rvalid = 0;                                  // bit i * 4 + r: the bank row is a real one
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) rvalid |= (i * 16 + r < n_left ? 1u : 0u) << (i * 4 + r);
    const long long *thr_tile = a.thr + q0 * a.n;
    int hit = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ql = qcol0 + j * 16 + frow;
        const ST top = ql < q_left ? rows_bound<ST>(thr_tile[(int64_t)ql * a.n + a.n - 1], a.s_max) : (ST)0;
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) hit |= (((rvalid >> (i * 4 + r)) & 1u) && s_of(i, j, r) < top) ? 1 : 0;
    }
    // (also the barrier after which the slice buffers may be overwritten)
    if (!__syncthreads_or(hit)) return;

    unsigned *cnt = reinterpret_cast<unsigned *>(smem);   // [tile_q][a.n]; at most 256 per entry
    ST *bound = reinterpret_cast<ST *>(smem + ROWS_THR_OFFSET);   // [a.n][tile_q]
    const int entries = tile_q * a.n;
    for (int e = threadIdx.x; e < entries; e += blockDim.x) {
        const int ql = e / a.n, t = e - ql * a.n;
        cnt[e] = 0u;
        bound[t * tile_q + ql] = ql < q_left ? rows_bound<ST>(thr_tile[e], a.s_max) : (ST)0;
    }
    __syncthreads();
    if (__any(hit)) {
        for (int t = 0; t < a.n; ++t) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ql = qcol0 + j * 16 + frow;
                const ST th = bound[t * tile_q + ql];
                unsigned c = 0;
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) c += (((rvalid >> (i * 4 + r)) & 1u) && s_of(i, j, r) < th) ? 1u : 0u;
                c += __shfl_xor(c, 16, 64);
                c += __shfl_xor(c, 32, 64);
                if (fk == 0 && c != 0u) atomicAdd(&cnt[ql * a.n + t], c);
            }
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < entries; e += blockDim.x) {
        const unsigned c = cnt[e];
        if (c != 0u) atomicAdd(&counts[q0 * a.n + e], (unsigned long long)c);
    }
}

}  // namespace gl_count
