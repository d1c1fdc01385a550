// L2 nearest neighbour for ARBITRARY fp32 images (values not on the 8-bit lattice): the general form of
// attack_models/utils.py:163 `mean((y - x)**2, dim=[1,2,3])` inside custom_knn (attack_models/fbb.py:73-88).
//
// The reference's own fp32 result depends on its reduction order (different on its CPU and CUDA builds), so
// this path fixes ONE order, shared bit for bit with the oracle (oracle/fbb_oracle.c gl_oracle_l2_f32):
//     d_k   = fl32(y_k - x_k)
//     c_j   = fmaf chain over k = j, j+4, j+8, ...            (j = 0..3, ascending k)
//     dist  = fl32( fl32( fl32(c_0 + c_1) + fl32(c_2 + c_3) ) / D )
// Every pair is an independent chain, so the result does not depend on tiling, launch shape or shard count.
// key = (float bits of dist) << 32 | global index, merged with atomicMin like the integer path.
//
// VALU kernel (2 ops per element pair; the matrix cores cannot form y - x before squaring without losing
// the fp32 difference).  Tile: 64 queries x 64 bank rows per workgroup, 256 threads x (4 x 4) pairs,
// K slices of 32 floats staged through LDS (row stride 36 floats: conflict-free float4 reads).
#include "gl_count_epi.h"
#include "gl_hist_epi.h"
#include "gl_kde_epi.h"
#include "gl_topk_sel.h"
#include <cmath>

namespace {

constexpr int TQ = 64, TN = 64, KS = 32, LDS_STRIDE = KS + 4, THREADS = 256;

__device__ __forceinline__ float4 load_row4(const float *__restrict__ base, int64_t row, int64_t nrows, int64_t d, int64_t k, bool vec)
{
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row >= nrows) return v;
    const float *p = base + row * d + k;
    if (vec) {
        if (k + 3 < d) return *reinterpret_cast<const float4 *>(p);
    }
    if (k + 0 < d) v.x = p[0];
    if (k + 1 < d) v.y = p[1];
    if (k + 2 < d) v.z = p[2];
    if (k + 3 < d) v.w = p[3];
    return v;
}

// what an epilogue does with the tile's distances
template <int EPI> struct f32_sink;
template <> struct f32_sink<0> {
    unsigned long long *keys;        // [nq], atomicMin of float_bits(D32) << 32 | index_base + n
    int64_t index_base;
};
template <> struct f32_sink<1> {
    gl_count::count_args<float> a;
    unsigned long long *counts;      // [nq][a.pitch]
};
template <> struct f32_sink<2> {
    unsigned *pieces;                // [ceil(n_rows / 4)][nq][4], n_rows and nq the kernel's (one slice)
};
template <> struct f32_sink<3> {
    gl_hist::hist_args<unsigned> a;  // the window on the bit pattern of D32, hi <= 0x7F800000 (+inf): NaN patterns lie outside every window
    unsigned long long *hist;        // [a.n_bins]
};
template <> struct f32_sink<4> {
    gl_count::rows_args a;           // thr[nq][a.n] on the bit pattern of D32, s_max = 0x7F800000 (+inf)
    unsigned long long *counts;      // [nq][a.n]
};
template <> struct f32_sink<5> {
    gl_kde::kde_f32_args a;          // D0[nq], bound[nq] on the bit pattern of D32, coef[a.n] descending
    unsigned long long *sums;        // [nq][a.n]
};

// The K loop of one 64 x 64 tile, shared by every epilogue: dist[a][b] = D32(query q0 + tq * 4 + a, bank row n0 + tn + 16 * b), the chain of
// the header comment.  Rows beyond n_rows and queries beyond nq are zero-filled in LDS: their distance is finite and the epilogues mask them.
// Ends behind a barrier: sq and sb are free when it returns.
__device__ __forceinline__ void pair_tile_f32(const float *__restrict__ bank, int64_t n_rows, int64_t n0, const float *__restrict__ query, int64_t nq,
                                              int64_t q0, int64_t d, float *sq, float *sb, int tid, float (&dist)[4][4])
{
    const int tq = tid >> 4, tn = tid & 15;          // 16 x 16 threads, each 4 queries x 4 bank rows
    const bool vec = ((d & 3) == 0) && (((reinterpret_cast<uintptr_t>(bank) | reinterpret_cast<uintptr_t>(query)) & 15) == 0);

    float acc[4][4][4];                               // [query][bank row][chain j]
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[a][b][j] = 0.0f;

    for (int64_t k0 = 0; k0 < d; k0 += KS) {
        // stage: 64 rows x 8 float4 per operand = 512 float4, 2 per thread per operand (zero beyond d / beyond the rows)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = tid + i * THREADS;
            const int r = e >> 3, c = (e & 7) * 4;
            *reinterpret_cast<float4 *>(&sq[r * LDS_STRIDE + c]) = load_row4(query, q0 + r, nq, d, k0 + c, vec);
            *reinterpret_cast<float4 *>(&sb[r * LDS_STRIDE + c]) = load_row4(bank, n0 + r, n_rows, d, k0 + c, vec);
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < KS; kk += 4) {
            float4 qv[4], bv[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) qv[a] = *reinterpret_cast<const float4 *>(&sq[(tq * 4 + a) * LDS_STRIDE + kk]);
#pragma unroll
            for (int b = 0; b < 4; ++b) bv[b] = *reinterpret_cast<const float4 *>(&sb[(tn + 16 * b) * LDS_STRIDE + kk]);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    float t;
                    t = __fsub_rn(qv[a].x, bv[b].x); acc[a][b][0] = fmaf(t, t, acc[a][b][0]);
                    t = __fsub_rn(qv[a].y, bv[b].y); acc[a][b][1] = fmaf(t, t, acc[a][b][1]);
                    t = __fsub_rn(qv[a].z, bv[b].z); acc[a][b][2] = fmaf(t, t, acc[a][b][2]);
                    t = __fsub_rn(qv[a].w, bv[b].w); acc[a][b][3] = fmaf(t, t, acc[a][b][3]);
                }
        }
        __syncthreads();
    }

    const float fd = (float)d;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const float s = __fadd_rn(__fadd_rn(acc[a][b][0], acc[a][b][1]), __fadd_rn(acc[a][b][2], acc[a][b][3]));
            dist[a][b] = __fdiv_rn(s, fd);
        }
}

// EPI 0: keys[q] = min(keys[q], float_bits(D32) << 32 | global index)   (gl_l2_knn_f32)
// EPI 1: counts[q][col0 + t] += #{ n : D32(q, n) <= thr[t] }, the steps of gl_count_epi.h in this kernel's thread layout: one compare per pair
//        against the largest radius and __syncthreads_or, so that tiles without a hit leave; the others turn the tile through the freed slice
//        buffers so that 4 neighbouring lanes hold a query's 64 distances, fold the per-threshold counts with two shuffles (no second wave
//        shares the query: no LDS table is needed to fold waves) and add ONE value per non-zero (query, t) with a 64-bit atomicAdd.
// EPI 2: float_bits(D32) as pieces[((n >> 2) * nq + q) * 4 + (n & 3)] for gl_topk_select_merge(elem = 4, shift = 32).  A thread's four rows are
//        16 apart, so the tile is turned through LDS and leaves as 16-byte pieces, 64 consecutive queries (1 KiB) per wave and store.
//        D32 >= +0 (a sum of squares divided by d > 0 never gives -0) and is not NaN for finite rows: unsigned order of the bits is the
//        order of the floats, and 0xFFFFFFFF, the value of a masked piece, never occurs.
// EPI 3: hist[b] += #{ pairs : lo <= bits(D32) <= hi and (bits(D32) - lo) >> shift == b }, the steps of gl_hist_epi.h in this kernel's thread
//        layout: two compares per pair and __syncthreads_or, so that tiles without a pair inside the window leave (at the refined levels of
//        a radix-select almost all do); the others bin their pairs into a table unsigned [n_bins] in the freed slice buffers (one LDS atomic
//        per pair inside; a tile holds 4096 pairs) and add ONE value per non-zero bin with a 64-bit atomicAdd.  The bin is formed from the
//        distance registers one pair at a time.  Integer adds of a function of the two rows alone: nothing depends on tile, chunk or shard.
// EPI 4: counts[q][t] += #{ n : bits(D32(q, n)) <= thr[q][t] }, EPI 1 with the thresholds of every query from device memory (int64 on the
//        pattern of D32, ascending per query; gl_count_epi.h's rows_bound turns "<= thr" into "< bound", at most 0x7F800001).  D32 >= +0, so
//        the unsigned compare of the patterns is the float compare; NaN patterns lie above every bound.  One compare per pair against
//        +inf and __syncthreads_or first (see there for what it buys), then the tile is turned as EPI 1 turns it, so that 4 neighbouring
//        lanes hold a query's 64 distances; each of them reads four of the query's sixteen bounds (after the K loop: no bound is live in
//        it) and they hand them round by shuffle.  The bounds are walked from the query's LAST one down and a wave stops at the first one
//        it holds nothing within (a query lives in one wave: no barrier is needed for that), so tiles without a hit cost one compare per
//        pair; the others count per bound, fold with two shuffles and add ONE value per non-zero (query, t) with a 64-bit atomicAdd.
//        Queries beyond nq get the bound 0, which nothing meets.
// EPI 5: sums[q][t] += sum over n of gl_kde_weight_f32(D32(q, n), D0[q], coef[t]) (gl_kde_epi.h), the soft-min sums of gl_kde.hip on this
//        distance, in EPI 4's shape: the tile reduced to one bit right behind the K loop (here: "holds a pattern that is not NaN" -- padding
//        gives finite distances, so a tile without one consists of real NaN pairs and raises the NaN bit of the flag), then turned through
//        LDS as patterns, masked pairs as +inf, which lies at or above every bound and weighs nothing.  D0 and the bound of the query
//        (gl_kde_cut_bits under the smallest coefficient) are read after the K loop; a pattern above +inf raises the NaN bit, one below
//        bits(D0) the below-offset bit.  A wave without a pattern below a bound leaves; the others form D32 - D0 once per pair, sum the
//        weights per coefficient, fold with two 64-bit shuffles and add ONE value per non-zero (query, t) with a 64-bit atomicAdd (a query
//        lives in one wave: no LDS table).  Integer adds of a pure function of (D32, D0, coef): nothing depends on tile, chunk or shard.
template <int EPI>
__global__ void __launch_bounds__(THREADS) l2_pairs_f32_kernel(const float *__restrict__ bank, int64_t n_rows, const float *__restrict__ query, int64_t nq,
                                                                int64_t d, int q_tiles, const f32_sink<EPI> sink)
{
    __shared__ __attribute__((aligned(16))) float smem[(TQ + TN) * LDS_STRIDE];
    const int qt = blockIdx.x % q_tiles, nt = blockIdx.x / q_tiles;
    const int64_t q0 = (int64_t)qt * TQ, n0 = (int64_t)nt * TN;
    const int tid = threadIdx.x;
    const int tq = tid >> 4, tn = tid & 15;

    float dist[4][4];
    pair_tile_f32(bank, n_rows, n0, query, nq, q0, d, smem, smem + TQ * LDS_STRIDE, tid, dist);

    if constexpr (EPI == 0) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int64_t q = q0 + tq * 4 + a;
            unsigned long long best = ~0ull;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int64_t n = n0 + tn + 16 * b;
                const unsigned long long key = ((unsigned long long)__float_as_uint(dist[a][b]) << 32) | (unsigned long long)(sink.index_base + n);
                if (n < n_rows && key < best) best = key;
            }
            // the 16 threads tn = 0..15 (consecutive lanes) hold the other bank rows of this query
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) {
                const unsigned long long other = __shfl_xor(best, o, 64);
                best = other < best ? other : best;
            }
            if (tn == 0 && q < nq && best != ~0ull) atomicMin(&sink.keys[q], best);
        }
    } else {
        const int n_left = gl_count::rows_left(n_rows, n0), q_left = gl_count::rows_left(nq, q0);
        unsigned valid = 0;                           // bit a * 4 + b: the pair is a real one
        if constexpr (EPI != 4 && EPI != 5) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) valid |= ((tq * 4 + a < q_left && tn + 16 * b < n_left) ? 1u : 0u) << (a * 4 + b);
        }

        if constexpr (EPI == 1) {
            const gl_count::count_args<float> &A = sink.a;
            const float top = A.thr[A.n - 1];
            int hit = 0;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) hit |= (((valid >> (a * 4 + b)) & 1u) && dist[a][b] <= top) ? 1 : 0;
            if (!__syncthreads_or(hit)) return;

            // the tile turned through LDS, query-major (masked pairs as NaN, which no radius meets): a query's 64 distances then sit with 4
            // neighbouring lanes, 16 each, and the per-threshold work needs nothing of the K loop's registers
            constexpr int TS = TN + 4;
            float *turn = smem;                                     // [TQ][TS]
            static_assert(TQ * TS + GL_COUNT_MAX_T <= (TQ + TN) * LDS_STRIDE, "the turned tile and the radii must fit the slice buffers");
            float *thr = smem + TQ * TS;                            // a run-time index into kernel arguments would cost registers
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) turn[(tq * 4 + a) * TS + tn + 16 * b] = ((valid >> (a * 4 + b)) & 1u) ? dist[a][b] : __builtin_nanf("");
            if (tid == 0) {
#pragma unroll
                for (int t = 0; t < GL_COUNT_MAX_T; ++t) thr[t] = A.thr[t];
            }
            __syncthreads();
            const int ql = tid >> 2, part = tid & 3;
            float4 v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = *reinterpret_cast<const float4 *>(&turn[ql * TS + part * 16 + i * 4]);
            for (int t = A.n - 1; t >= 0; --t) {
                const float th = thr[t];
                unsigned c = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) c += (v[i].x <= th ? 1u : 0u) + (v[i].y <= th ? 1u : 0u) + (v[i].z <= th ? 1u : 0u) + (v[i].w <= th ? 1u : 0u);
                if (!__any(c != 0u)) break;                         // ascending radii: the wave holds nothing within the smaller ones either
                c += __shfl_xor(c, 1, 64);
                c += __shfl_xor(c, 2, 64);
                if (part == 0 && c != 0u) atomicAdd(&sink.counts[(q0 + ql) * A.pitch + A.col0 + t], (unsigned long long)c);
            }
        } else if constexpr (EPI == 4) {
            // One compare per pair first, as in EPI 1, here against +inf, the largest bound there is: a tile that holds nothing but NaN
            // leaves.  (The bounds of the queries are not read yet.  Reduced to this one bit right behind the K loop, the distances leave
            // the loop at EPI 1's register count, two waves per SIMD; turned without it, the kernel needs more than 256 registers and runs
            // at one, as it does when the masks below are formed from the thread index the K loop holds: hence the opaque copy.)
            int alive = 0;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) alive |= __float_as_uint(dist[a][b]) <= 0x7F800000u ? 1 : 0;
            if (!__syncthreads_or(alive)) return;
            int etid = tid;
            asm volatile("" : "+v"(etid));
            const int etq = etid >> 4, etn = etid & 15;

            // the tile turned through LDS as for EPI 1, as patterns (masked pairs as 0xFFFFFFFF, which lies above every bound): a query's 64
            // distances then sit with 4 neighbouring lanes, 16 each, and nothing below needs the K loop's registers or another barrier
            constexpr int TS = TN + 4;
            static_assert(TQ * TS <= (TQ + TN) * LDS_STRIDE, "the turned tile must fit the slice buffers");
            unsigned *turn = reinterpret_cast<unsigned *>(smem);   // [TQ][TS]
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    turn[(etq * 4 + a) * TS + etn + 16 * b] =
                        (etq * 4 + a < q_left && etn + 16 * b < n_left) ? __float_as_uint(dist[a][b]) : 0xFFFFFFFFu;
            __syncthreads();
            const int ql = etid >> 2, part = etid & 3, lane = etid & 63;
            uint4 v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = *reinterpret_cast<const uint4 *>(&turn[ql * TS + part * 16 + i * 4]);
            // each of the query's four lanes reads four of its (at most sixteen) bounds, here and not before: none is live in the K loop
            const int n_thr = sink.a.n;
            const long long *thr_q = sink.a.thr + (q0 + (ql < q_left ? ql : 0)) * n_thr;
            unsigned mine[4];                                       // bounds part * 4 .. part * 4 + 3
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = part * 4 + i;
                const unsigned bound = gl_count::rows_bound<unsigned>(thr_q[t < n_thr ? t : n_thr - 1], sink.a.s_max);
                mine[i] = (ql < q_left && t < n_thr) ? bound : 0u;
            }
            // from the query's LAST bound down: a wave that holds nothing within it leaves at once (ascending bounds: nothing within the
            // smaller ones either), which is where almost every tile of a refined search ends
            for (int t = n_thr - 1; t >= 0; --t) {
                const int i = t & 3;
                const unsigned own = i == 0 ? mine[0] : (i == 1 ? mine[1] : (i == 2 ? mine[2] : mine[3]));
                const unsigned th = __shfl(own, (lane & ~3) | (t >> 2), 64);
                unsigned c = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) c += (v[k].x < th ? 1u : 0u) + (v[k].y < th ? 1u : 0u) + (v[k].z < th ? 1u : 0u) + (v[k].w < th ? 1u : 0u);
                if (!__any(c != 0u)) break;
                c += __shfl_xor(c, 1, 64);
                c += __shfl_xor(c, 2, 64);
                if (part == 0 && c != 0u) atomicAdd(&sink.counts[(q0 + ql) * n_thr + t], (unsigned long long)c);
            }
        } else if constexpr (EPI == 5) {
            int alive = 0;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) alive |= __float_as_uint(dist[a][b]) <= 0x7F800000u ? 1 : 0;
            if (!__syncthreads_or(alive)) {
                if (tid == 0) atomicOr(sink.a.flag, gl_kde::KDE_FLAG_NAN);     // nothing but NaN: no padded pair among them, all are real
                return;
            }
            int etid = tid;                                         // (the opaque copy: see EPI 4)
            asm volatile("" : "+v"(etid));
            const int etq = etid >> 4, etn = etid & 15;

            constexpr int TS = TN + 4;
            static_assert(TQ * TS + GL_COUNT_MAX_T <= (TQ + TN) * LDS_STRIDE, "the turned tile and the coefficients must fit the slice buffers");
            unsigned *turn = reinterpret_cast<unsigned *>(smem);   // [TQ][TS]
            float *coef = smem + TQ * TS;                           // a run-time index into kernel arguments would cost registers
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    turn[(etq * 4 + a) * TS + etn + 16 * b] =
                        (etq * 4 + a < q_left && etn + 16 * b < n_left) ? __float_as_uint(dist[a][b]) : 0x7F800000u;
            if (etid == 0) {
#pragma unroll
                for (int t = 0; t < GL_COUNT_MAX_T; ++t) coef[t] = sink.a.coef[t];
            }
            __syncthreads();
            const int ql = etid >> 2, part = etid & 3;
            uint4 v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = *reinterpret_cast<const uint4 *>(&turn[ql * TS + part * 16 + i * 4]);
            // D0 and the bound of the lane's query, here and not before: neither is live in the K loop
            const float d0 = ql < q_left ? sink.a.d0[q0 + ql] : 0.0f;
            const unsigned top = ql < q_left ? sink.a.bound[q0 + ql] : 0u;
            const unsigned b0 = __float_as_uint(d0);
            float delta[16];                                        // D32 - D0 of the pairs that take part
            unsigned in = 0;                                        // bit k: pair k takes part
            int bad = 0;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const uint4 &p = v[k >> 2];
                const unsigned s = (k & 3) == 0 ? p.x : ((k & 3) == 1 ? p.y : ((k & 3) == 2 ? p.z : p.w));
                if (s > 0x7F800000u) bad |= gl_kde::KDE_FLAG_NAN;
                if (s < top && s < b0) bad |= gl_kde::KDE_FLAG_BELOW;
                const bool take = s < top && s >= b0;
                in |= (take ? 1u : 0u) << k;
                delta[k] = gl_kde_add(__uint_as_float(s), -d0);
            }
            if (bad) atomicOr(sink.a.flag, bad);
            if (!__any(in != 0u)) return;                           // (no barrier follows)
            const int n_coef = sink.a.n;
            for (int t = n_coef - 1; t >= 0; --t) {
                const float c = coef[t];
                unsigned long long w = 0ull;
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if ((in >> k) & 1u) w += gl_kde_weight_x(gl_kde_mul(delta[k], c));      // = gl_kde_weight_f32(D32, D0, c)
                w += __shfl_xor(w, 1, 64);
                w += __shfl_xor(w, 2, 64);
                if (part == 0 && w != 0ull) atomicAdd(&sink.sums[(q0 + ql) * n_coef + t], w);
            }
        } else if constexpr (EPI == 3) {
            const unsigned lo = sink.a.lo, hi = sink.a.hi;
            const int shift = sink.a.shift, n_bins = sink.a.n_bins;
            auto inside = [&](int a, int b) -> bool {
                const unsigned s = __float_as_uint(dist[a][b]);
                return ((valid >> (a * 4 + b)) & 1u) && s >= lo && s <= hi;
            };
            int hit = 0;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) hit |= inside(a, b) ? 1 : 0;
            if (!__syncthreads_or(hit)) return;

            static_assert(GL_HIST_MAX_BINS * 4 <= (TQ + TN) * LDS_STRIDE * 4, "the bin table must fit the slice buffers");
            unsigned *tab = reinterpret_cast<unsigned *>(smem);     // [n_bins]; at most 4096 per entry
            for (int e = tid; e < n_bins; e += THREADS) tab[e] = 0u;
            __syncthreads();
            if (hit) {
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (inside(a, b)) atomicAdd(&tab[(__float_as_uint(dist[a][b]) - lo) >> shift], 1u);      // below n_bins because bits <= hi
            }
            __syncthreads();
            for (int e = tid; e < n_bins; e += THREADS) {
                const unsigned c = tab[e];
                if (c != 0u) atomicAdd(&sink.hist[e], (unsigned long long)c);
            }
        } else {
            constexpr int TS = TN + 4;                 // row stride of the turned tile: 16-byte aligned pieces
            static_assert(TQ * TS <= (TQ + TN) * LDS_STRIDE, "the turned tile must fit the slice buffers");
            unsigned *turn = reinterpret_cast<unsigned *>(smem);   // [TQ][TS]: query-major, bank rows contiguous
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    turn[(tq * 4 + a) * TS + tn + 16 * b] = ((valid >> (a * 4 + b)) & 1u) ? __float_as_uint(dist[a][b]) : 0xFFFFFFFFu;
            __syncthreads();
            // 64 queries x 16 pieces, 4 per thread; consecutive lanes take consecutive queries of one piece row
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = tid + i * THREADS;
                const int ql = e & (TQ - 1), g = e >> 6;
                if (ql < q_left && g * 4 < n_left)
                    *reinterpret_cast<uint4 *>(sink.pieces + (((n0 >> 2) + g) * nq + q0 + ql) * 4) = *reinterpret_cast<const uint4 *>(&turn[ql * TS + g * 4]);
            }
        }
    }
}

// per-row distances (Loss('l2').forward for float inputs), same chain definition; one wave per row pair is
// not possible (the chain is sequential), so one THREAD per row: only used for BATCH_SIZE-sized calls.
__global__ void l2_rows_f32_kernel(const float *__restrict__ xh, int64_t b, const float *__restrict__ xg, int64_t b_gt, int64_t d,
                                   float *__restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= b) return;
    const float *pa = xh + r * d;
    const float *pb = xg + (b_gt == 1 ? 0 : r) * d;
    float c[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t k = 0; k < d; ++k) {
        const float t = __fsub_rn(pb[k], pa[k]);
        c[k & 3] = fmaf(t, t, c[k & 3]);
    }
    out[r] = __fdiv_rn(__fadd_rn(__fadd_rn(c[0], c[1]), __fadd_rn(c[2], c[3])), (float)d);
}

__global__ void keys_unpack_f32_kernel(const unsigned long long *__restrict__ keys, int64_t nq, float *__restrict__ dist, int64_t *__restrict__ idx)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const unsigned long long k = keys[i];
    dist[i] = __uint_as_float((unsigned)(k >> 32));
    idx[i] = (int64_t)(k & 0xFFFFFFFFull);
}

}  // namespace

extern "C" {

int gl_l2_knn_f32(gl_ctx *ctx, const float *bank_dev, int64_t n_rows, int64_t index_base, const float *query_dev, int64_t nq, int64_t d,
                  uint64_t *keys_dev)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx && n_rows >= 0 && nq >= 0 && d > 0, "gl_l2_knn_f32: bad sizes");
    GL_REQUIRE(index_base >= 0 && index_base + n_rows <= 0xFFFFFFFFll, "gl_l2_knn_f32: global index does not fit 32 bits");
    if (n_rows == 0 || nq == 0) return GL_OK;
    GL_REQUIRE(bank_dev && query_dev && keys_dev, "gl_l2_knn_f32: NULL device pointer");
    const int64_t q_tiles = gl_ceil_div(nq, TQ), n_tiles = gl_ceil_div(n_rows, TN);
    GL_REQUIRE(q_tiles * n_tiles < (1ll << 31), "gl_l2_knn_f32: grid too large");
    f32_sink<0> sink;
    sink.keys = reinterpret_cast<unsigned long long *>(keys_dev);
    sink.index_base = index_base;
    hipLaunchKernelGGL(l2_pairs_f32_kernel<0>, dim3((unsigned)(q_tiles * n_tiles)), dim3(THREADS), 0, ctx->stream, bank_dev, n_rows, query_dev, nq, d,
                       (int)q_tiles, sink);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int gl_l2_count_f32(gl_ctx *ctx, const float *bank_dev, int64_t n_rows, const float *query_dev, int64_t nq, int64_t d, const float *thr_host, int n_thr,
                    uint64_t *counts_dev)
{
    static const char *fn = "gl_l2_count_f32";
    gl_make_current(ctx);
    GL_REQUIRE(ctx && n_rows >= 0 && nq >= 0 && d > 0, "%s: bad sizes", fn);
    GL_REQUIRE(n_thr >= 1 && n_thr <= GL_COUNT_MAX_T, "%s: n_thr=%d outside [1, %d]", fn, n_thr, GL_COUNT_MAX_T);
    GL_REQUIRE(thr_host, "%s: NULL thresholds", fn);
    for (int t = 0; t < n_thr; ++t) {
        GL_REQUIRE(!std::isnan(thr_host[t]), "%s: thr[%d] is NaN", fn, t);
        GL_REQUIRE(t == 0 || thr_host[t - 1] <= thr_host[t], "%s: thresholds must be ascending (thr[%d]=%g > thr[%d]=%g)", fn, t - 1,
                   (double)thr_host[t - 1], t, (double)thr_host[t]);
    }
    if (n_rows == 0 || nq == 0) return GL_OK;
    GL_REQUIRE(bank_dev && query_dev && counts_dev, "%s: NULL device pointer", fn);
    GL_REQUIRE((reinterpret_cast<uintptr_t>(counts_dev) & 7) == 0, "%s: the counters must be 8-byte aligned", fn);
    const int64_t q_tiles = gl_ceil_div(nq, TQ), n_tiles = gl_ceil_div(n_rows, TN);
    GL_REQUIRE(q_tiles * n_tiles < (1ll << 31), "%s: grid too large", fn);
    if (thr_host[n_thr - 1] < 0.0f) return GL_OK;        // D32 >= +0: no pair lies within a negative radius
    int skip = 0;
    while (thr_host[skip] < 0.0f) ++skip;                 // ... so those columns stay as they are
    f32_sink<1> sink;
    sink.a.n = n_thr - skip;
    sink.a.col0 = skip;
    sink.a.pitch = n_thr;
    for (int t = 0; t < GL_COUNT_MAX_T; ++t) sink.a.thr[t] = thr_host[skip + (t < sink.a.n ? t : sink.a.n - 1)];
    sink.counts = reinterpret_cast<unsigned long long *>(counts_dev);
    hipLaunchKernelGGL(l2_pairs_f32_kernel<1>, dim3((unsigned)(q_tiles * n_tiles)), dim3(THREADS), 0, ctx->stream, bank_dev, n_rows, query_dev, nq, d,
                       (int)q_tiles, sink);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int gl_l2_count_rows_f32(gl_ctx *ctx, const float *bank_dev, int64_t n_rows, const float *query_dev, int64_t nq, int64_t d, const int64_t *thr_dev,
                         int n_thr, uint64_t *counts_dev)
{
    static const char *fn = "gl_l2_count_rows_f32";
    gl_make_current(ctx);
    GL_REQUIRE(ctx && n_rows >= 0 && nq >= 0 && d > 0, "%s: bad sizes", fn);
    GL_REQUIRE(n_thr >= 1 && n_thr <= GL_COUNT_MAX_T, "%s: n_thr=%d outside [1, %d]", fn, n_thr, GL_COUNT_MAX_T);
    if (n_rows == 0 || nq == 0) return GL_OK;
    GL_REQUIRE(thr_dev, "%s: NULL thresholds", fn);
    GL_REQUIRE((reinterpret_cast<uintptr_t>(thr_dev) & 7) == 0, "%s: the thresholds must be 8-byte aligned", fn);
    GL_REQUIRE(bank_dev && query_dev && counts_dev, "%s: NULL device pointer", fn);
    GL_REQUIRE((reinterpret_cast<uintptr_t>(counts_dev) & 7) == 0, "%s: the counters must be 8-byte aligned", fn);
    const int64_t q_tiles = gl_ceil_div(nq, TQ), n_tiles = gl_ceil_div(n_rows, TN);
    GL_REQUIRE(q_tiles * n_tiles < (1ll << 31), "%s: grid too large", fn);
    f32_sink<4> sink;
    sink.a.thr = reinterpret_cast<const long long *>(thr_dev);
    sink.a.s_max = 0x7F800000ll;                          // +inf: the largest pattern of a D32 that is not NaN
    sink.a.n = n_thr;
    sink.counts = reinterpret_cast<unsigned long long *>(counts_dev);
    hipLaunchKernelGGL(l2_pairs_f32_kernel<4>, dim3((unsigned)(q_tiles * n_tiles)), dim3(THREADS), 0, ctx->stream, bank_dev, n_rows, query_dev, nq, d,
                       (int)q_tiles, sink);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int gl_l2_kde_rows_f32(gl_ctx *ctx, const float *bank_dev, int64_t n_rows, const float *query_dev, int64_t nq, int64_t d, const float *D0_dev,
                       const uint32_t *bound_dev, const float *coef_host, int n_coef, uint64_t *sums_dev)
{
    static const char *fn = "gl_l2_kde_rows_f32";
    gl_make_current(ctx);
    GL_REQUIRE(ctx && n_rows >= 0 && nq >= 0 && d > 0, "%s: bad sizes", fn);
    GL_REQUIRE(n_coef >= 1 && n_coef <= GL_COUNT_MAX_T, "%s: n_coef=%d outside [1, %d]", fn, n_coef, GL_COUNT_MAX_T);
    GL_REQUIRE(coef_host, "%s: NULL coefficients", fn);
    f32_sink<5> sink;
    for (int t = 0; t < GL_COUNT_MAX_T; ++t) sink.a.coef[t] = 0.0f;
    for (int t = 0; t < n_coef; ++t) {
        GL_REQUIRE(coef_host[t] >= 0.0f && coef_host[t] <= 3.402823466e38f, "%s: coef[%d] is not a finite value >= 0", fn, t);
        GL_REQUIRE(t == 0 || coef_host[t] <= coef_host[t - 1], "%s: the coefficients must be descending (coef[%d] > coef[%d])", fn, t, t - 1);
        sink.a.coef[t] = coef_host[t];
    }
    if (n_rows == 0 || nq == 0) return GL_OK;
    GL_REQUIRE(D0_dev && bound_dev, "%s: NULL offsets or bounds", fn);
    GL_REQUIRE(((reinterpret_cast<uintptr_t>(D0_dev) | reinterpret_cast<uintptr_t>(bound_dev)) & 3) == 0, "%s: offsets and bounds must be 4-byte aligned", fn);
    GL_REQUIRE(bank_dev && query_dev && sums_dev, "%s: NULL device pointer", fn);
    GL_REQUIRE((reinterpret_cast<uintptr_t>(sums_dev) & 7) == 0, "%s: the sums must be 8-byte aligned", fn);
    const int64_t q_tiles = gl_ceil_div(nq, TQ), n_tiles = gl_ceil_div(n_rows, TN);
    GL_REQUIRE(q_tiles * n_tiles < (1ll << 31), "%s: grid too large", fn);
    sink.a.d0 = D0_dev;
    sink.a.bound = bound_dev;
    sink.a.flag = ctx->kde_flag;
    sink.a.n = n_coef;
    sink.sums = reinterpret_cast<unsigned long long *>(sums_dev);
    hipLaunchKernelGGL(l2_pairs_f32_kernel<5>, dim3((unsigned)(q_tiles * n_tiles)), dim3(THREADS), 0, ctx->stream, bank_dev, n_rows, query_dev, nq, d,
                       (int)q_tiles, sink);
    GL_LAUNCH_CHECK();
    return gl_kde_flag_check(fn, ctx);
}

int gl_l2_hist_f32(gl_ctx *ctx, const float *bank_dev, int64_t n_rows, const float *query_dev, int64_t nq, int64_t d, uint32_t lo, int shift, int n_bins,
                   uint64_t *hist_dev)
{
    static const char *fn = "gl_l2_hist_f32";
    constexpr unsigned kMaxBits = 0x7F800000u;            // +inf: the largest pattern of a D32 that is not NaN
    gl_make_current(ctx);
    GL_REQUIRE(ctx && n_rows >= 0 && nq >= 0 && d > 0, "%s: bad sizes", fn);
    GL_REQUIRE(n_bins >= 1 && n_bins <= GL_HIST_MAX_BINS, "%s: n_bins=%d outside [1, %d]", fn, n_bins, GL_HIST_MAX_BINS);
    GL_REQUIRE(shift >= 0 && shift <= 31, "%s: shift=%d outside [0, 31]", fn, shift);
    if (n_rows == 0 || nq == 0) return GL_OK;
    GL_REQUIRE(bank_dev && query_dev && hist_dev, "%s: NULL device pointer", fn);
    GL_REQUIRE((reinterpret_cast<uintptr_t>(hist_dev) & 7) == 0, "%s: the histogram must be 8-byte aligned", fn);
    const int64_t q_tiles = gl_ceil_div(nq, TQ), n_tiles = gl_ceil_div(n_rows, TN);
    GL_REQUIRE(q_tiles * n_tiles < (1ll << 31), "%s: grid too large", fn);
    if (lo > kMaxBits) return GL_OK;                      // the window lies above every pattern
    const unsigned long long last = (unsigned long long)lo + ((unsigned long long)n_bins << shift) - 1ull;
    f32_sink<3> sink;
    sink.a.lo = lo;
    sink.a.hi = (unsigned)(last < kMaxBits ? last : kMaxBits);
    sink.a.shift = shift;
    sink.a.n_bins = n_bins;
    sink.hist = reinterpret_cast<unsigned long long *>(hist_dev);
    hipLaunchKernelGGL(l2_pairs_f32_kernel<3>, dim3((unsigned)(q_tiles * n_tiles)), dim3(THREADS), 0, ctx->stream, bank_dev, n_rows, query_dev, nq, d,
                       (int)q_tiles, sink);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int gl_l2_topk_f32(gl_ctx *ctx, const float *bank_dev, int64_t n_rows, int64_t index_base, const float *query_dev, int64_t nq, int64_t d, int k,
                   uint64_t *topk_keys_dev)
{
    static const char *fn = "gl_l2_topk_f32";
    gl_make_current(ctx);
    GL_REQUIRE(ctx && n_rows >= 0 && nq >= 0 && d > 0, "%s: bad sizes", fn);
    GL_REQUIRE(k >= 1 && k <= GL_TOPK_MAX, "%s: k=%d outside [1, %d]", fn, k, GL_TOPK_MAX);
    GL_REQUIRE(index_base >= 0 && index_base + n_rows <= 0xFFFFFFFFll, "%s: global index does not fit 32 bits", fn);
    if (n_rows == 0 || nq == 0) return GL_OK;
    GL_REQUIRE(bank_dev && query_dev && topk_keys_dev, "%s: NULL device pointer", fn);
    GL_REQUIRE((reinterpret_cast<uintptr_t>(topk_keys_dev) & 7) == 0, "%s: the key lists must be 8-byte aligned", fn);

    // slices: qs queries x rs bank rows of D32 within the budget, whole tiles (or the whole extent), never below one tile
    const int64_t budget = (int64_t)gl_topk_workspace_budget(ctx);
    int64_t qs = budget / (TQ * 4) / TQ * TQ;
    if (qs < TQ) qs = TQ;
    if (qs > GL_TOPK_MAX_QUERY_SLICE) qs = GL_TOPK_MAX_QUERY_SLICE;
    if (qs > nq) qs = nq;
    int64_t rs = budget / (qs * 4) / TN * TN;
    if (rs < TN) rs = TN;
    if (rs > n_rows) rs = n_rows;
    GL_REQUIRE(gl_ceil_div(qs, TQ) * gl_ceil_div(rs, TN) < (1ll << 31), "%s: grid too large", fn);
    const int64_t groups = gl_ceil_div(rs, 4);
    const int64_t segs = gl_topk_segments(qs, rs);

    gl_scratch_guard mem{ctx};
    int rc = gl_malloc(ctx, (size_t)(groups * qs * 16), &mem.p[0]);
    if (rc != GL_OK) return rc;
    rc = gl_malloc(ctx, (size_t)(segs * qs * k * 8), &mem.p[1]);
    if (rc != GL_OK) return rc;
    f32_sink<2> sink;
    sink.pieces = static_cast<unsigned *>(mem.p[0]);
    unsigned long long *lists = static_cast<unsigned long long *>(mem.p[1]);
    unsigned long long *dst = reinterpret_cast<unsigned long long *>(topk_keys_dev);

    for (int64_t q_lo = 0; q_lo < nq; q_lo += qs) {
        const int64_t nqs = nq - q_lo < qs ? nq - q_lo : qs;
        for (int64_t r_lo = 0; r_lo < n_rows; r_lo += rs) {
            const int64_t nrs = n_rows - r_lo < rs ? n_rows - r_lo : rs;
            const int64_t q_tiles = gl_ceil_div(nqs, TQ), n_tiles = gl_ceil_div(nrs, TN);
            hipLaunchKernelGGL(l2_pairs_f32_kernel<2>, dim3((unsigned)(q_tiles * n_tiles)), dim3(THREADS), 0, ctx->stream, bank_dev + r_lo * d, nrs,
                               query_dev + q_lo * d, nqs, d, (int)q_tiles, sink);
            GL_LAUNCH_CHECK();
            rc = gl_topk_select_merge(ctx, mem.p[0], 4, nrs, nqs, k, 32, index_base + r_lo, dst + q_lo * k, lists, segs);
            if (rc != GL_OK) return rc;
        }
    }
    return GL_OK;
}

int gl_l2_rows_f32(gl_ctx *ctx, const float *x_hat_dev, int64_t b, const float *x_gt_dev, int64_t b_gt, int64_t d, float *out_dev)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx && b >= 0 && d > 0, "gl_l2_rows_f32: bad ctx/b/d");
    GL_REQUIRE(b_gt == 1 || b_gt == b, "gl_l2_rows_f32: x_gt must hold 1 row or %lld rows, got %lld", (long long)b, (long long)b_gt);
    if (b == 0) return GL_OK;
    GL_REQUIRE(x_hat_dev && x_gt_dev && out_dev, "gl_l2_rows_f32: NULL device pointer");
    hipLaunchKernelGGL(l2_rows_f32_kernel, dim3((unsigned)gl_ceil_div(b, 64)), dim3(64), 0, ctx->stream, x_hat_dev, b, x_gt_dev, b_gt, d, out_dev);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int gl_keys_unpack_f32(gl_ctx *ctx, const uint64_t *keys_dev, int64_t nq, float *dist_dev, int64_t *idx_dev)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx && nq >= 0, "gl_keys_unpack_f32: bad ctx/nq");
    if (nq == 0) return GL_OK;
    GL_REQUIRE(keys_dev && dist_dev && idx_dev, "gl_keys_unpack_f32: NULL device pointer");
    hipLaunchKernelGGL(keys_unpack_f32_kernel, dim3((unsigned)gl_ceil_div(nq, 256)), dim3(256), 0, ctx->stream,
                       reinterpret_cast<const unsigned long long *>(keys_dev), nq, dist_dev, idx_dev);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

}  // extern "C"
