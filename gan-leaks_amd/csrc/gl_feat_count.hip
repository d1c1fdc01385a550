// Other reductions over the pairwise distances of the l2-lpips search (0.2 LPIPS + L2, attack_models/utils.py:166-176): epsilon-ball counts
// (the Monte-Carlo membership score of Hilprecht et al. under the reference's own fbb distance, attack_models/fbb.py:148) and the stored
// [nq][n_rows] distance matrix for small cases.
//
// The kernels are the searches of gl_lpips.hip with another epilogue: feat_pairs_h1_kernel<.., true> walks the super-tiles of
// feat_knn_h1c_kernel (persistent, 8 clusters), feat_pairs_h1_kernel<.., false> the tiles of feat_knn_h1s_kernel (persistent, no clusters),
// feat_pairs_split_kernel is feat_knn_kernel's 128 x 128 tile on split rows.  Same main loop (gl_pair256::mainloop), same K slices, same K
// segments and the same order of the segment totals, so the fp32 value they reduce is bit for bit the one the search packs into its key:
//     D32(q, n) = fmaxf(fmaf(-2 inv_s2, acc, qn + bn), 0)
// EPI = 0: counts[q][col0 + t] += #{ n < n_rows : D32(q, n) <= thr[t] } through gl_count_epi.h's count_epilogue, i.e. one compare per pair, the
//          per-threshold work only in waves that hold a hit, an LDS table in the slice buffers, one 64-bit atomicAdd per non-zero (query, t).
//          Integer adds commute, and D32 of a pair does not depend on where in a tile, a chunk or a shard the pair sits (every accumulator
//          sees the same K order): the counts are functions of the multiset of D32 values.
// EPI = 1: out[q * ld + n] = D32(q, n).
// EPI = 2: the bit pattern of D32(q, n) into the piece layout gl_topk.hip's selection reads, pieces[((n >> 2) * nq + q) * 4 + (n & 3)]: the
//          top-K nearest neighbours under l2-lpips (gl_feat_topk*) are the k smallest keys float_bits(D32) << 32 | global index.
//          D32 >= +0: fmaxf(., 0) never yields -0 here, because -2 inv_s2 acc and qn + bn cannot both be -0 (norms are sums of squares, and
//          (+0) + (+0) = +0), so an exactly cancelling fmaf gives +0 under round-to-nearest.  Unsigned comparison of the bits of non-negative
//          floats is float comparison, so the order of the keys is the order of (D32, index): column 0 is the search's key.  D32 is never
//          NaN after fmaxf, so 0xFFFFFFFF never occurs in the top half and ~0 stays the empty slot.  As D32 of a pair does not depend on
//          where the pair sits, neither does the set of keys: the lists need no rescoring and do not depend on tile, slice, chunk or shard.
// EPI = 3: hist[b] += #{ pairs : lo <= bits(D32) <= hi and (bits(D32) - lo) >> shift == b } through gl_hist_epi.h's hist_epilogue on the uint32
//          pattern of D32: D32 >= +0 (see EPI = 2), so the unsigned order of the patterns is the order of the floats and a host radix-select
//          over such windows (attack.select_ranks with s_max = 0x7F800000, the pattern of +inf) finds the exact D32 at any rank.  The bin table
//          (at most 8 KiB) lives in the slice buffers, as the table of EPI = 0 does.  Integer adds of a value that does not depend on where the
//          pair sits: the histogram is a function of the multiset of D32 values.
// EPI = 4: counts[q][t] += #{ n < n_rows : bits(D32(q, n)) <= thr[q][t] }, the thresholds of every query from device memory, through
//          gl_count_epi.h's second count_epilogue (rows_args) on the uint32 pattern of D32 with s_max = 0x7F800000 (+inf): D32 >= +0 (see
//          EPI = 2), so the unsigned compare of the patterns IS the float compare D32 <= float(thr), and a host search over integer brackets
//          (attack.select_kth_rows) finds the exact D32 of any rank per query.  Same commuting integer adds as EPI = 0.
// EPI = 5: sums[q][t] += sum over n < n_rows of gl_kde_weight_f32(D32(q, n), D0[q], coef[t]), the soft-min (kernel-density) sums of
//          gl_kde.hip on the float distance, through gl_kde_epi.h's kde_epilogue_f32 on the uint32 pattern of D32: one compare per pair
//          against its query's bound (gl_kde_cut_bits under the smallest coefficient, from device memory like D0), an LDS table, one 64-bit
//          atomicAdd per non-zero (query, t).  The weight is a pure function of (D32, D0, coef) and D32 does not depend on where the pair
//          sits: the sums are functions of the multiset of D32 values.  A pair below D0 raises bit 1 of the context's kde flag.
#include "gl_conv.h"
#include "gl_count_epi.h"
#include "gl_feat_pair.h"
#include "gl_hist_epi.h"
#include "gl_kde_epi.h"
#include "gl_pair256.h"
#include "gl_topk_sel.h"
#include <cmath>

using namespace gl_feat_pair;

namespace {

template <int EPI> struct pair_sink;
template <> struct pair_sink<0> {
    gl_count::count_args<float> a;
    unsigned long long *counts;      // [nq][a.pitch]
};
template <> struct pair_sink<1> {
    float *dist;                     // [nq][ld]
    int64_t ld;
};
template <> struct pair_sink<2> {
    unsigned *pieces;                // [ceil(n_rows / 4)][nq][4], n_rows and nq the kernel's (one slice)
};
template <> struct pair_sink<3> {
    gl_hist::hist_args<unsigned> a;  // the window on the bit pattern of D32
    unsigned long long *hist;        // [a.n_bins]
};
template <> struct pair_sink<4> {
    gl_count::rows_args a;           // thr[nq][a.n] on the bit pattern of D32, s_max = 0x7F800000
    unsigned long long *counts;      // [nq][a.n]
};
template <> struct pair_sink<5> {
    gl_kde::kde_f32_args a;          // D0[nq], bound[nq] on the bit pattern of D32, coef[a.n] descending
    unsigned long long *sums;        // [nq][a.n]
};

// The epilogue of one tile.  acc holds the dot products of the lane's NI x 4 tiles of 16 x 16 (column = query qcol0 + j * 16 + (lane & 15) of
// the tile, row = bank row nbase + i * 16 + r); D32 replaces them in place, so that no norm stays live next to the accumulators.
// Every thread of the workgroup must call this (EPI = 0, EPI = 3, EPI = 4 and EPI = 5 have barriers and use smem).
// EPI = 2: acc[i][j] is 4 consecutive bank rows (from a multiple of 4) of one query = one piece, a 16-byte store; the 16 lanes of a column
// group are 16 consecutive queries = 256 contiguous bytes.  Pieces whose first row is past n_rows are not written; rows past n_rows inside a
// written piece hold whatever the clamped operands gave (the selection masks n < n_rows).
template <int EPI, int NI>
__device__ __forceinline__ void finish_tile(v4f (&acc)[NI][4], const float *__restrict__ bank_norm, int64_t n_rows, int64_t nbase,
                                            const float *__restrict__ query_norm, int64_t nq, int64_t q0, int qcol0, int tile_q, float inv_s2,
                                            const pair_sink<EPI> &sink, char *smem, int lane)
{
    const int frow = lane & 15;
    const int n_left = gl_count::rows_left(n_rows, nbase), q_left = gl_count::rows_left(nq, q0);
    const float m2 = -2.0f * inv_s2;
    float qn[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ql = qcol0 + j * 16 + frow;
        qn[j] = ql < q_left ? query_norm[q0 + ql] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float bn = i * 16 + r < n_left ? bank_norm[nbase + i * 16 + r] : 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j][r] = fmaxf(fmaf(m2, acc[i][j][r], __fadd_rn(qn[j], bn)), 0.0f);      // as the search forms it
        }
    if constexpr (EPI == 0) {
        auto s_of = [&](int i, int j, int r) -> float { return acc[i][j][r]; };
        gl_count::count_epilogue<NI, float>(s_of, n_left, q0, qcol0, q_left, tile_q, sink.a, sink.counts, smem, lane);
    } else if constexpr (EPI == 3) {
        auto s_of = [&](int i, int j, int r) -> unsigned { return __float_as_uint(acc[i][j][r]); };
        gl_hist::hist_epilogue<NI, unsigned, true>(s_of, n_left, qcol0, q_left, sink.a, sink.hist, smem, lane);
    } else if constexpr (EPI == 4) {
        auto s_of = [&](int i, int j, int r) -> unsigned { return __float_as_uint(acc[i][j][r]); };
        gl_count::count_epilogue<NI, unsigned>(s_of, n_left, q0, qcol0, q_left, tile_q, sink.a, sink.counts, smem, lane);
    } else if constexpr (EPI == 5) {
        auto s_of = [&](int i, int j, int r) -> unsigned { return __float_as_uint(acc[i][j][r]); };
        gl_kde::kde_epilogue_f32<NI>(s_of, n_left, q0, qcol0, q_left, tile_q, sink.a, sink.sums, smem, lane);
    } else if constexpr (EPI == 2) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ql = qcol0 + j * 16 + frow;
            if (ql >= q_left) continue;
            unsigned *col = sink.pieces + ((nbase >> 2) * nq + q0 + ql) * 4;
#pragma unroll
            for (int i = 0; i < NI; ++i)
                if (i * 16 < n_left) *reinterpret_cast<v4f *>(col + (int64_t)i * 16 * nq) = acc[i][j];      // (i * 16 / 4) pieces rows further: 4 nq * 4 values
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ql = qcol0 + j * 16 + frow;
            if (ql >= q_left) continue;
            float *row = sink.dist + (q0 + ql) * sink.ld + nbase;
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (i * 16 + r < n_left) row[i * 16 + r] = acc[i][j][r];
        }
    }
}

// fp16 search rows, 256 x 256 tile.  CLUSTER: the schedule of feat_knn_h1c_kernel (a cluster of 32 workgroups takes a super-tile of 4 bank x 8
// query tiles and meets before every super-tile and K segment), else the one of feat_knn_h1s_kernel (tiles in strip order, nobody meets).
template <int EPI, bool CLUSTER>
__global__ void __launch_bounds__(512, 2)
feat_pairs_h1_kernel(const char *__restrict__ bank, const float *__restrict__ bank_norm, int64_t n_rows, const char *__restrict__ query,
                     const float *__restrict__ query_norm, int64_t nq, int64_t K1, int q_tiles, int n_tiles, char *__restrict__ scratch, int members,
                     float inv_s2, int blocked, const pair_sink<EPI> sink)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t kstep = blocked ? 32768 : 128;        // bytes between consecutive K slices of a tile's rows (K-blocked rows: gl_conv.h)
    v4f *totals = reinterpret_cast<v4f *>(scratch + 4096 + (size_t)blockIdx.x * kTotalsPerWg);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave >> 2, wq = wave & 3;
    const int fk = lane >> 4;
    const int64_t nk = K1 / 64;
    const int nseg = (int)((nk + kSegSlices - 1) / kSegSlices);
    v4f *my_tot = totals + (size_t)wave * 32 * 64 + lane;

    // one tile: `meet` runs before every K segment, also in workgroups without a tile (they still take part in the cluster's rendezvous)
    auto tile = [&](bool active, int nt, int qt, auto meet) {
        const int64_t n0 = (int64_t)nt * GT, q0 = (int64_t)qt * GT;
        gl_pair256::Source sa = {}, sb = {};
        if (active) {
            if (blocked) {
                sa = gl_pair256::make_source_blocked(bank, n0, nk, wave, lane);
                sb = gl_pair256::make_source_blocked(query, q0, nk, wave, lane);
            } else {
                sa = gl_pair256::make_source(bank, n0, n_rows, K1 * 2, wave, lane);
                sb = gl_pair256::make_source(query, q0, nq, K1 * 2, wave, lane);
            }
        }
        v4f acc[8][4];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = (v4f){0.f, 0.f, 0.f, 0.f};
        // The binning epilogue is the one with the most live values next to the accumulators (the kernel-density one, EPI = 5, likewise).  The lane's LDS offsets of the main loop are
        // invariants of the tile loop; kept across that epilogue they are spilled and reloaded inside the K loop.  Formed per tile from a
        // copy of `lane` the compiler cannot see through, they end with the K loop (a few VALU instructions per tile).
        int mlane = lane;
        if constexpr (EPI == 3 || EPI == 5) asm volatile("" : "+v"(mlane));
        for (int seg = 0; seg < nseg; ++seg) {
            meet();
            if (!active) continue;
            const int64_t k0 = (int64_t)seg * kSegSlices;
            const int64_t len = nk - k0 < kSegSlices ? nk - k0 : kSegSlices;
            gl_pair256::mainloop<v8h>(sa, sb, len, smem, acc, wave, mlane,
                                      [](const v8h &a, const v8h &b, const v4f &c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }, k0 * kstep, kstep);
            __syncthreads();                             // all fragment reads of the segment are done before its buffers are refilled
            if (nseg > 1) {
                // totals (+)= accumulators; the last segment leaves the sum in the accumulators (the order of feat_knn_h1c_kernel)
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        v4f *t = my_tot + (i * 4 + j) * 64;
                        if (seg > 0) acc[i][j] += *t;
                        if (seg + 1 < nseg) { *t = acc[i][j]; acc[i][j] = (v4f){0.f, 0.f, 0.f, 0.f}; }
                        __builtin_amdgcn_sched_barrier(0);       // one tile at a time: 32 loads in flight at once would not fit the register file
                    }
            }
        }
        if (!active) return;
        if constexpr (EPI == 3 || EPI == 5) {
            int elane = lane;                            // (as mlane: what the epilogue derives from the lane is formed after the K loop)
            asm volatile("" : "+v"(elane));
            finish_tile<EPI, 8>(acc, bank_norm, n_rows, n0 + wn * 128 + (elane >> 4) * 4, query_norm, nq, q0, wq * 64, GT, inv_s2, sink, smem, elane);
        } else {
            finish_tile<EPI, 8>(acc, bank_norm, n_rows, n0 + wn * 128 + fk * 4, query_norm, nq, q0, wq * 64, GT, inv_s2, sink, smem, lane);
        }
    };

    if constexpr (CLUSTER) {
        const int cluster = blockIdx.x & (kClusters - 1), member = blockIdx.x >> 3;
        unsigned *counter = reinterpret_cast<unsigned *>(scratch) + cluster * 32;           // 128 B apart
        const int sup_n = (n_tiles + kSuperN - 1) / kSuperN, sup_q = (q_tiles + kSuperQ - 1) / kSuperQ;
        unsigned episode = 0;
        for (int s = cluster; s < sup_n * sup_q; s += kClusters) {
            const int sq = s / sup_n, sn = s % sup_n;
            const int nt = sn * kSuperN + (member & (kSuperN - 1)), qt = sq * kSuperQ + (member >> 2);
            const bool active = member < kSuperN * kSuperQ && nt < n_tiles && qt < q_tiles;
            // (the rendezvous ends in a barrier: the epilogue's LDS table of the previous tile has been read by then)
            tile(active, nt, qt, [&]() { cluster_meet(counter, (unsigned)members * ++episode); });
        }
    } else {
        const unsigned tiles = (unsigned)q_tiles * (unsigned)n_tiles;
        for (unsigned t = blockIdx.x; t < tiles; t += gridDim.x) {
            int qt, nt;
            strip4_order(t, q_tiles, n_tiles, qt, nt);
            tile(true, nt, qt, []() {});
            __syncthreads();           // the next tile's prologue refills the slice buffers
        }
    }
}

// split rows (hi + lo halves of every value): feat_knn_kernel's tile, K loop and segments
template <int EPI>
__global__ void __launch_bounds__(256, 2)
feat_pairs_split_kernel(const char *__restrict__ bank, const float *__restrict__ bank_norm, int64_t n_rows, const char *__restrict__ query,
                        const float *__restrict__ query_norm, int64_t nq, int64_t K, int q_tiles, int n_tiles, float inv_s2, const pair_sink<EPI> sink)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const unsigned id = gl_xcd_remap(blockIdx.x, (unsigned)q_tiles * (unsigned)n_tiles);
    int qt, nt;
    gl_strip_order(id, q_tiles, n_tiles, qt, nt);
    const int64_t n0 = (int64_t)nt * FT, q0 = (int64_t)qt * FT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave >> 1, wq = wave & 1;
    const int rsub = lane >> 3, slot = lane & 7;
    const int64_t row_bytes = K * 4;

    const char *a_src[4], *b_src[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (wave * 4 + i) * 8 + rsub;
        int64_t gn = n0 + r, gq = q0 + r;
        if (gn >= n_rows) gn = n_rows - 1;      // clamped duplicates are masked in the epilogue
        if (gq >= nq) gq = nq - 1;
        a_src[i] = bank + gn * row_bytes + (slot ^ (r & 7)) * 16;
        b_src[i] = query + gq * row_bytes + (slot ^ (r & 7)) * 16;
    }
    auto stage = [&](int64_t kt, char *buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) gl_glds16(a_src[i] + kt * FROW, buf + (wave * 4 + i) * 1024);
#pragma unroll
        for (int i = 0; i < 4; ++i) gl_glds16(b_src[i] + kt * FROW, buf + FOPER + (wave * 4 + i) * 1024);
    };

    v4f acc[4][4], tot[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = tot[i][j] = (v4f){0.f, 0.f, 0.f, 0.f};

    const int64_t nk = K / 32;
    stage(0, smem);
    const int frow = lane & 15, fk = lane >> 4;
    for (int64_t kt = 0; kt < nk; ++kt) {
        __syncthreads();
        char *cur = smem + (kt & 1) * 2 * FOPER;
        if (kt + 1 < nk) stage(kt + 1, smem + ((kt + 1) & 1) * 2 * FOPER);
        const char *la = cur + (wn * 64) * FROW;
        const char *lb = cur + FOPER + (wq * 64) * FROW;
        v8h a_hi[4], a_lo[4], b_hi[4], b_lo[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = i * 16 + frow;
            a_hi[i] = *reinterpret_cast<const v8h *>(la + r * FROW + ((fk ^ (r & 7)) << 4));
            a_lo[i] = *reinterpret_cast<const v8h *>(la + r * FROW + (((4 + fk) ^ (r & 7)) << 4));
            b_hi[i] = *reinterpret_cast<const v8h *>(lb + r * FROW + ((fk ^ (r & 7)) << 4));
            b_lo[i] = *reinterpret_cast<const v8h *>(lb + r * FROW + (((4 + fk) ^ (r & 7)) << 4));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_lo[i], b_hi[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi[i], b_lo[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi[i], b_hi[j], acc[i][j], 0, 0, 0);
            }
        if ((kt & (kSplitSeg - 1)) == kSplitSeg - 1) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) { tot[i][j] += acc[i][j]; acc[i][j] = (v4f){0.f, 0.f, 0.f, 0.f}; }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += tot[i][j];

    finish_tile<EPI, 4>(acc, bank_norm, n_rows, n0 + wn * 64 + fk * 4, query_norm, nq, q0, wq * 64, FT, inv_s2, sink, smem, lane);
}

// ---- host side

int check_rows(const char *fn, gl_ctx *ctx, const void *bank, const float *bank_norm, int64_t n_rows, const void *query, const float *query_norm,
               int64_t nq, int64_t K, int k_multiple)
{
    GL_REQUIRE(ctx, "%s: NULL ctx", fn);
    GL_REQUIRE(n_rows >= 0 && nq >= 0 && K > 0 && K % k_multiple == 0, "%s: bad sizes n_rows=%lld nq=%lld K=%lld (K must be a multiple of %d)", fn,
               (long long)n_rows, (long long)nq, (long long)K, k_multiple);
    if (n_rows == 0 || nq == 0) return GL_OK;
    GL_REQUIRE(bank && bank_norm && query && query_norm, "%s: NULL device pointer", fn);
    GL_REQUIRE(((reinterpret_cast<uintptr_t>(bank) | reinterpret_cast<uintptr_t>(query)) & 15) == 0, "%s: rows must be 16-byte aligned", fn);
    GL_REQUIRE(((reinterpret_cast<uintptr_t>(bank_norm) | reinterpret_cast<uintptr_t>(query_norm)) & 3) == 0, "%s: norms must be 4-byte aligned", fn);
    GL_REQUIRE(gl_ceil_div(nq, FT) * gl_ceil_div(n_rows, FT) < (1ll << 31), "%s: grid too large", fn);
    return GL_OK;
}

int make_count_sink(const char *fn, const float *thr, int n_thr, int col0, int pitch, uint64_t *counts, bool need_counts, pair_sink<0> &s)
{
    GL_REQUIRE(n_thr >= 1 && n_thr <= GL_COUNT_MAX_T, "%s: n_thr=%d outside [1, %d]", fn, n_thr, GL_COUNT_MAX_T);
    GL_REQUIRE(thr, "%s: NULL thresholds", fn);
    GL_REQUIRE(col0 >= 0 && pitch <= GL_COUNT_MAX_T && col0 + n_thr <= pitch, "%s: columns [%d, %d) do not fit counters of %d columns (at most %d)", fn,
               col0, col0 + n_thr, pitch, GL_COUNT_MAX_T);
    for (int t = 0; t < n_thr; ++t) {
        GL_REQUIRE(!std::isnan(thr[t]), "%s: thr[%d] is NaN", fn, t);
        GL_REQUIRE(thr[t] >= 0.0f, "%s: thresholds must be non-negative (thr[%d]=%g); drop those columns, nothing meets them", fn, t, (double)thr[t]);
        GL_REQUIRE(t == 0 || thr[t - 1] <= thr[t], "%s: thresholds must be ascending (thr[%d]=%g > thr[%d]=%g)", fn, t - 1, (double)thr[t - 1], t, (double)thr[t]);
    }
    if (need_counts) {
        GL_REQUIRE(counts, "%s: NULL counters", fn);
        GL_REQUIRE((reinterpret_cast<uintptr_t>(counts) & 7) == 0, "%s: the counters must be 8-byte aligned", fn);
    }
    s.a.n = n_thr;
    s.a.col0 = col0;
    s.a.pitch = pitch;
    for (int t = 0; t < GL_COUNT_MAX_T; ++t) s.a.thr[t] = thr[t < n_thr ? t : n_thr - 1];
    s.counts = reinterpret_cast<unsigned long long *>(counts);
    return GL_OK;
}

int make_dist_sink(const char *fn, float *out, int64_t ld, int64_t n_rows, bool need_out, pair_sink<1> &s)
{
    GL_REQUIRE(ld >= n_rows, "%s: ld=%lld is shorter than a row of n_rows=%lld distances", fn, (long long)ld, (long long)n_rows);
    if (need_out) {
        GL_REQUIRE(out, "%s: NULL output", fn);
        GL_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "%s: the output must be 4-byte aligned", fn);
    }
    s.dist = out;
    s.ld = ld;
    return GL_OK;
}

// the window of gl_feat_hist* on the patterns of D32: 0 .. 0x7F800000 (+inf) is all there is (D32 >= +0 and never NaN after fmaxf), so a
// window is cut there.  `above`: the window lies beyond every pattern and the caller returns.
constexpr unsigned kMaxBits = 0x7F800000u;

int make_hist_sink(const char *fn, uint32_t lo, int shift, int n_bins, uint64_t *hist, bool need_hist, pair_sink<3> &s, bool &above)
{
    static_assert(GL_HIST_MAX_BINS * 4 <= 4 * FOPER && GL_HIST_MAX_BINS * 4 <= 4 * GOPER, "the bin table lives in the slice buffers");
    GL_REQUIRE(n_bins >= 1 && n_bins <= GL_HIST_MAX_BINS, "%s: n_bins=%d outside [1, %d]", fn, n_bins, GL_HIST_MAX_BINS);
    GL_REQUIRE(shift >= 0 && shift <= 31, "%s: shift=%d outside [0, 31]", fn, shift);
    if (need_hist) {
        GL_REQUIRE(hist, "%s: NULL histogram", fn);
        GL_REQUIRE((reinterpret_cast<uintptr_t>(hist) & 7) == 0, "%s: the histogram must be 8-byte aligned", fn);
    }
    above = lo > kMaxBits;
    const unsigned long long last = (unsigned long long)lo + ((unsigned long long)n_bins << shift) - 1ull;
    s.a.lo = lo;
    s.a.hi = (unsigned)(last < kMaxBits ? last : kMaxBits);
    s.a.shift = shift;
    s.a.n_bins = n_bins;
    s.hist = reinterpret_cast<unsigned long long *>(hist);
    return GL_OK;
}

// per-query thresholds of gl_feat_count_rows* on the patterns of D32: rows_bound<unsigned> gives at most kMaxBits + 1, which fits
int make_rows_sink(const char *fn, const int64_t *thr_dev, int n_thr, uint64_t *counts, bool need_ptrs, pair_sink<4> &s)
{
    static_assert(gl_count::ROWS_THR_OFFSET + GT * GL_COUNT_MAX_T * 4 <= 4 * GOPER && gl_count::ROWS_THR_OFFSET + FT * GL_COUNT_MAX_T * 4 <= 4 * FOPER,
                  "counters and bounds must fit the slice buffers");
    GL_REQUIRE(n_thr >= 1 && n_thr <= GL_COUNT_MAX_T, "%s: n_thr=%d outside [1, %d]", fn, n_thr, GL_COUNT_MAX_T);
    if (need_ptrs) {
        GL_REQUIRE(thr_dev, "%s: NULL thresholds", fn);
        GL_REQUIRE((reinterpret_cast<uintptr_t>(thr_dev) & 7) == 0, "%s: the thresholds must be 8-byte aligned", fn);
        GL_REQUIRE(counts, "%s: NULL counters", fn);
        GL_REQUIRE((reinterpret_cast<uintptr_t>(counts) & 7) == 0, "%s: the counters must be 8-byte aligned", fn);
    }
    s.a.thr = reinterpret_cast<const long long *>(thr_dev);
    s.a.s_max = (long long)kMaxBits;
    s.a.n = n_thr;
    s.counts = reinterpret_cast<unsigned long long *>(counts);
    return GL_OK;
}

// D0, bounds and coefficients of gl_feat_kde_rows*: the checks of gl_kde.hip's kde_rows_impl
int make_kde_sink(const char *fn, gl_ctx *ctx, const float *d0_dev, const uint32_t *bound_dev, const float *coef, int n_coef, uint64_t *sums,
                  bool need_ptrs, pair_sink<5> &s)
{
    static_assert(gl_kde::KDE_F32_LDS_BYTES <= 4 * GOPER && gl_kde::KDE_F32_LDS_BYTES <= 4 * FOPER, "sums, D0 and bounds must fit the slice buffers");
    static_assert(GT <= 256 && FT <= 256, "the LDS layout of kde_epilogue_f32 holds 256 queries");
    GL_REQUIRE(n_coef >= 1 && n_coef <= GL_COUNT_MAX_T, "%s: n_coef=%d outside [1, %d]", fn, n_coef, GL_COUNT_MAX_T);
    GL_REQUIRE(coef, "%s: NULL coefficients", fn);
    for (int t = 0; t < GL_COUNT_MAX_T; ++t) s.a.coef[t] = 0.0f;
    for (int t = 0; t < n_coef; ++t) {
        GL_REQUIRE(coef[t] >= 0.0f && coef[t] <= 3.402823466e38f, "%s: coef[%d] is not a finite value >= 0", fn, t);
        GL_REQUIRE(t == 0 || coef[t] <= coef[t - 1], "%s: the coefficients must be descending (coef[%d] > coef[%d])", fn, t, t - 1);
        s.a.coef[t] = coef[t];
    }
    if (need_ptrs) {
        GL_REQUIRE(d0_dev && bound_dev, "%s: NULL offsets or bounds", fn);
        GL_REQUIRE(((reinterpret_cast<uintptr_t>(d0_dev) | reinterpret_cast<uintptr_t>(bound_dev)) & 3) == 0, "%s: offsets and bounds must be 4-byte aligned", fn);
        GL_REQUIRE(sums, "%s: NULL sums", fn);
        GL_REQUIRE((reinterpret_cast<uintptr_t>(sums) & 7) == 0, "%s: the sums must be 8-byte aligned", fn);
    }
    s.a.d0 = d0_dev;
    s.a.bound = bound_dev;
    s.a.flag = ctx->kde_flag;
    s.a.n = n_coef;
    s.sums = reinterpret_cast<unsigned long long *>(sums);
    return GL_OK;
}

// the dispatch of gl_feat_knn_h1_scaled: clusters on a whole MI355X, the cluster-free persistent form on a device with fewer compute units
// (tuning builds: GL_PAIR_VARIANT=5 forces the latter).  Either way the same bits.
bool h1_clustered(const gl_ctx *ctx, int64_t K1)
{
    return (gl_vrow_blocked(K1) || gl_tuning_int("GL_PAIR_VARIANT", 3) != 5) && ctx->num_cu / kClusters >= kSuperN * kSuperQ;
}

template <int EPI>
int launch_h1(const char *fn, gl_ctx *ctx, const void *bank, const float *bank_norm, int64_t n_rows, const void *query, const float *query_norm, int64_t nq,
              int64_t K1, float row_scale, const pair_sink<EPI> &sink)
{
    GL_REQUIRE(row_scale > 0.0f && std::isfinite(row_scale), "%s: the row scale must be positive", fn);
    const float inv_s2 = 1.0f / (row_scale * row_scale);
    const int64_t q_tiles = gl_ceil_div(nq, GT), n_tiles = gl_ceil_div(n_rows, GT);
    const int lds = 4 * GOPER;
    const int blocked = gl_vrow_blocked(K1) ? 1 : 0;
    const int members = ctx->num_cu / kClusters;
    const bool clustered = h1_clustered(ctx, K1);
    const int grid = clustered ? kClusters * members : (ctx->num_cu > 0 ? ctx->num_cu : 256);
    if (const int rc = reserve_pair_scratch(ctx, grid)) return rc;
    GL_ONCE_PER_DEVICE(ctx, \
        GL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(feat_pairs_h1_kernel<EPI, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds)); \
        GL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(feat_pairs_h1_kernel<EPI, false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds)););
    gl_prof_scope prof_(ctx, GL_PROF_FEAT_COUNT);
    if (clustered) {
        GL_HIP(hipMemsetAsync(ctx->pair_scratch, 0, 4096, ctx->stream));         // the cluster counters
        hipLaunchKernelGGL((feat_pairs_h1_kernel<EPI, true>), dim3((unsigned)grid), dim3(512), lds, ctx->stream, reinterpret_cast<const char *>(bank), bank_norm,
                           n_rows, reinterpret_cast<const char *>(query), query_norm, nq, K1, (int)q_tiles, (int)n_tiles, ctx->pair_scratch, members, inv_s2,
                           blocked, sink);
    } else {
        hipLaunchKernelGGL((feat_pairs_h1_kernel<EPI, false>), dim3((unsigned)grid), dim3(512), lds, ctx->stream, reinterpret_cast<const char *>(bank), bank_norm,
                           n_rows, reinterpret_cast<const char *>(query), query_norm, nq, K1, (int)q_tiles, (int)n_tiles, ctx->pair_scratch, members, inv_s2,
                           blocked, sink);
    }
    GL_LAUNCH_CHECK();
    return GL_OK;
}

template <int EPI>
int launch_split(gl_ctx *ctx, const float *bank, const float *bank_norm, int64_t n_rows, const float *query, const float *query_norm, int64_t nq, int64_t K,
                 const pair_sink<EPI> &sink)
{
    const int64_t q_tiles = gl_ceil_div(nq, FT), n_tiles = gl_ceil_div(n_rows, FT);
    const int lds = 4 * FOPER;
    GL_ONCE_PER_DEVICE(ctx, \
        GL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(feat_pairs_split_kernel<EPI>), hipFuncAttributeMaxDynamicSharedMemorySize, lds)););
    gl_prof_scope prof_(ctx, GL_PROF_FEAT_COUNT);
    hipLaunchKernelGGL((feat_pairs_split_kernel<EPI>), dim3((unsigned)(q_tiles * n_tiles)), dim3(256), lds, ctx->stream, reinterpret_cast<const char *>(bank),
                       bank_norm, n_rows, reinterpret_cast<const char *>(query), query_norm, nq, K, (int)q_tiles, (int)n_tiles, 1.0f / (kVScale * kVScale), sink);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

// gl_feat_topk*: slices of queries x bank rows whose D32 pieces fit the top-K workspace, each a launch of the pair kernel (EPI = 2) followed
// by gl_topk.hip's selection and merge into the slice's rows of the lists.  H1: fp16 search rows (256 x 256 tile), else split rows (128 x 128).
template <bool H1>
int feat_topk_impl(const char *fn, gl_ctx *ctx, const void *bank, const float *bank_norm, int64_t n_rows, int64_t index_base, const void *query,
                   const float *query_norm, int64_t nq, int64_t K, float row_scale, int k, uint64_t *topk)
{
    gl_make_current(ctx);
    if (const int rc = check_rows(fn, ctx, bank, bank_norm, n_rows, query, query_norm, nq, K, H1 ? 64 : 32)) return rc;
    GL_REQUIRE(k >= 1 && k <= GL_TOPK_MAX, "%s: k=%d outside [1, %d]", fn, k, GL_TOPK_MAX);
    GL_REQUIRE(index_base >= 0 && index_base + n_rows <= (1ll << 32), "%s: global index does not fit the 32 index bits of a key", fn);
    if (H1) GL_REQUIRE(row_scale > 0.0f && std::isfinite(row_scale), "%s: the row scale must be positive", fn);
    if (n_rows == 0 || nq == 0) return GL_OK;
    GL_REQUIRE(topk, "%s: NULL key lists", fn);
    GL_REQUIRE((reinterpret_cast<uintptr_t>(topk) & 7) == 0, "%s: the key lists must be 8-byte aligned", fn);

    // slices: qs queries x rs bank rows of D32 within the budget, whole tiles (or the whole extent), never below one tile.  The clustered
    // kernel hands out super-tiles of 1024 bank rows x 2048 queries and every slice is a launch of its own: whole super-tiles when they fit.
    const int64_t tile = H1 ? GT : FT;
    const bool clustered = H1 && h1_clustered(ctx, K);
    const int64_t sup_q = (int64_t)kSuperQ * GT, sup_n = (int64_t)kSuperN * GT;
    const int64_t budget = (int64_t)gl_topk_workspace_budget(ctx);
    int64_t qs = budget / (tile * 4) / tile * tile;
    if (qs < tile) qs = tile;
    if (qs > GL_TOPK_MAX_QUERY_SLICE) qs = GL_TOPK_MAX_QUERY_SLICE;
    if (qs >= nq) qs = nq;
    else if (clustered && qs >= sup_q) qs = qs / sup_q * sup_q;
    int64_t rs = budget / (qs * 4) / tile * tile;
    if (clustered && rs >= sup_n) rs = rs / sup_n * sup_n;
    if (rs < tile) rs = tile;
    if (rs > n_rows) rs = n_rows;
    const int64_t groups = gl_ceil_div(rs, 4);
    const int64_t segs = gl_topk_segments(qs, rs);

    gl_scratch_guard mem{ctx};
    int rc = gl_malloc(ctx, (size_t)(groups * qs * 16), &mem.p[0]);
    if (rc != GL_OK) return rc;
    rc = gl_malloc(ctx, (size_t)(segs * qs * k * 8), &mem.p[1]);
    if (rc != GL_OK) return rc;
    pair_sink<2> sink;
    sink.pieces = static_cast<unsigned *>(mem.p[0]);
    unsigned long long *lists = static_cast<unsigned long long *>(mem.p[1]);
    unsigned long long *dst = reinterpret_cast<unsigned long long *>(topk);
    // a slice starts at a multiple of the tile; K-blocked rows are whole blocks of 256 rows x K halves, so that is row * K * 2 bytes for them too
    const int64_t row_bytes = H1 ? K * 2 : K * 4;

    for (int64_t q_lo = 0; q_lo < nq; q_lo += qs) {
        const int64_t nqs = nq - q_lo < qs ? nq - q_lo : qs;
        const char *qrows = static_cast<const char *>(query) + q_lo * row_bytes;
        for (int64_t r_lo = 0; r_lo < n_rows; r_lo += rs) {
            const int64_t nrs = n_rows - r_lo < rs ? n_rows - r_lo : rs;
            const char *brows = static_cast<const char *>(bank) + r_lo * row_bytes;
            if constexpr (H1)
                rc = launch_h1<2>(fn, ctx, brows, bank_norm + r_lo, nrs, qrows, query_norm + q_lo, nqs, K, row_scale, sink);
            else
                rc = launch_split<2>(ctx, reinterpret_cast<const float *>(brows), bank_norm + r_lo, nrs, reinterpret_cast<const float *>(qrows),
                                     query_norm + q_lo, nqs, K, sink);
            if (rc != GL_OK) return rc;
            rc = gl_topk_select_merge(ctx, mem.p[0], 4, nrs, nqs, k, 32, index_base + r_lo, dst + q_lo * k, lists, segs);
            if (rc != GL_OK) return rc;
        }
    }
    return GL_OK;
}

}  // namespace

extern "C" {

int gl_feat_count_h1_scaled(gl_ctx *ctx, const void *bank_V16_dev, const float *bank_norm_dev, int64_t n_rows, const void *query_V16_dev,
                            const float *query_norm_dev, int64_t nq, int64_t K1, float row_scale, const float *thr_host, int n_thr, int col0, int pitch,
                            uint64_t *counts_dev)
{
    static const char *fn = "gl_feat_count_h1_scaled";
    gl_make_current(ctx);
    pair_sink<0> sink;
    if (const int rc = check_rows(fn, ctx, bank_V16_dev, bank_norm_dev, n_rows, query_V16_dev, query_norm_dev, nq, K1, 64)) return rc;
    if (const int rc = make_count_sink(fn, thr_host, n_thr, col0, pitch, counts_dev, n_rows > 0 && nq > 0, sink)) return rc;
    if (n_rows == 0 || nq == 0) return GL_OK;
    return launch_h1<0>(fn, ctx, bank_V16_dev, bank_norm_dev, n_rows, query_V16_dev, query_norm_dev, nq, K1, row_scale, sink);
}

int gl_feat_count(gl_ctx *ctx, const float *bank_V_dev, const float *bank_norm_dev, int64_t n_rows, const float *query_V_dev, const float *query_norm_dev,
                  int64_t nq, int64_t K, const float *thr_host, int n_thr, int col0, int pitch, uint64_t *counts_dev)
{
    static const char *fn = "gl_feat_count";
    gl_make_current(ctx);
    pair_sink<0> sink;
    if (const int rc = check_rows(fn, ctx, bank_V_dev, bank_norm_dev, n_rows, query_V_dev, query_norm_dev, nq, K, 32)) return rc;
    if (const int rc = make_count_sink(fn, thr_host, n_thr, col0, pitch, counts_dev, n_rows > 0 && nq > 0, sink)) return rc;
    if (n_rows == 0 || nq == 0) return GL_OK;
    return launch_split<0>(ctx, bank_V_dev, bank_norm_dev, n_rows, query_V_dev, query_norm_dev, nq, K, sink);
}

int gl_feat_count_rows_h1_scaled(gl_ctx *ctx, const void *bank_V16_dev, const float *bank_norm_dev, int64_t n_rows, const void *query_V16_dev,
                                 const float *query_norm_dev, int64_t nq, int64_t K1, float row_scale, const int64_t *thr_dev, int n_thr,
                                 uint64_t *counts_dev)
{
    static const char *fn = "gl_feat_count_rows_h1_scaled";
    gl_make_current(ctx);
    pair_sink<4> sink;
    if (const int rc = check_rows(fn, ctx, bank_V16_dev, bank_norm_dev, n_rows, query_V16_dev, query_norm_dev, nq, K1, 64)) return rc;
    if (const int rc = make_rows_sink(fn, thr_dev, n_thr, counts_dev, n_rows > 0 && nq > 0, sink)) return rc;
    if (n_rows == 0 || nq == 0) return GL_OK;
    return launch_h1<4>(fn, ctx, bank_V16_dev, bank_norm_dev, n_rows, query_V16_dev, query_norm_dev, nq, K1, row_scale, sink);
}

int gl_feat_count_rows(gl_ctx *ctx, const float *bank_V_dev, const float *bank_norm_dev, int64_t n_rows, const float *query_V_dev,
                       const float *query_norm_dev, int64_t nq, int64_t K, const int64_t *thr_dev, int n_thr, uint64_t *counts_dev)
{
    static const char *fn = "gl_feat_count_rows";
    gl_make_current(ctx);
    pair_sink<4> sink;
    if (const int rc = check_rows(fn, ctx, bank_V_dev, bank_norm_dev, n_rows, query_V_dev, query_norm_dev, nq, K, 32)) return rc;
    if (const int rc = make_rows_sink(fn, thr_dev, n_thr, counts_dev, n_rows > 0 && nq > 0, sink)) return rc;
    if (n_rows == 0 || nq == 0) return GL_OK;
    return launch_split<4>(ctx, bank_V_dev, bank_norm_dev, n_rows, query_V_dev, query_norm_dev, nq, K, sink);
}

int gl_feat_kde_rows_h1_scaled(gl_ctx *ctx, const void *bank_V16_dev, const float *bank_norm_dev, int64_t n_rows, const void *query_V16_dev,
                               const float *query_norm_dev, int64_t nq, int64_t K1, float row_scale, const float *D0_dev, const uint32_t *bound_dev,
                               const float *coef_host, int n_coef, uint64_t *sums_dev)
{
    static const char *fn = "gl_feat_kde_rows_h1_scaled";
    gl_make_current(ctx);
    pair_sink<5> sink;
    if (const int rc = check_rows(fn, ctx, bank_V16_dev, bank_norm_dev, n_rows, query_V16_dev, query_norm_dev, nq, K1, 64)) return rc;
    if (const int rc = make_kde_sink(fn, ctx, D0_dev, bound_dev, coef_host, n_coef, sums_dev, n_rows > 0 && nq > 0, sink)) return rc;
    if (n_rows == 0 || nq == 0) return GL_OK;
    if (const int rc = launch_h1<5>(fn, ctx, bank_V16_dev, bank_norm_dev, n_rows, query_V16_dev, query_norm_dev, nq, K1, row_scale, sink)) return rc;
    return gl_kde_flag_check(fn, ctx);
}

int gl_feat_kde_rows(gl_ctx *ctx, const float *bank_V_dev, const float *bank_norm_dev, int64_t n_rows, const float *query_V_dev,
                     const float *query_norm_dev, int64_t nq, int64_t K, const float *D0_dev, const uint32_t *bound_dev, const float *coef_host,
                     int n_coef, uint64_t *sums_dev)
{
    static const char *fn = "gl_feat_kde_rows";
    gl_make_current(ctx);
    pair_sink<5> sink;
    if (const int rc = check_rows(fn, ctx, bank_V_dev, bank_norm_dev, n_rows, query_V_dev, query_norm_dev, nq, K, 32)) return rc;
    if (const int rc = make_kde_sink(fn, ctx, D0_dev, bound_dev, coef_host, n_coef, sums_dev, n_rows > 0 && nq > 0, sink)) return rc;
    if (n_rows == 0 || nq == 0) return GL_OK;
    if (const int rc = launch_split<5>(ctx, bank_V_dev, bank_norm_dev, n_rows, query_V_dev, query_norm_dev, nq, K, sink)) return rc;
    return gl_kde_flag_check(fn, ctx);
}

int gl_feat_hist_h1_scaled(gl_ctx *ctx, const void *bank_V16_dev, const float *bank_norm_dev, int64_t n_rows, const void *query_V16_dev,
                           const float *query_norm_dev, int64_t nq, int64_t K1, float row_scale, uint32_t lo, int shift, int n_bins, uint64_t *hist_dev)
{
    static const char *fn = "gl_feat_hist_h1_scaled";
    gl_make_current(ctx);
    pair_sink<3> sink;
    bool above = false;
    if (const int rc = check_rows(fn, ctx, bank_V16_dev, bank_norm_dev, n_rows, query_V16_dev, query_norm_dev, nq, K1, 64)) return rc;
    if (const int rc = make_hist_sink(fn, lo, shift, n_bins, hist_dev, n_rows > 0 && nq > 0, sink, above)) return rc;
    GL_REQUIRE(row_scale > 0.0f && std::isfinite(row_scale), "%s: the row scale must be positive", fn);
    if (n_rows == 0 || nq == 0 || above) return GL_OK;
    return launch_h1<3>(fn, ctx, bank_V16_dev, bank_norm_dev, n_rows, query_V16_dev, query_norm_dev, nq, K1, row_scale, sink);
}

int gl_feat_hist(gl_ctx *ctx, const float *bank_V_dev, const float *bank_norm_dev, int64_t n_rows, const float *query_V_dev, const float *query_norm_dev,
                 int64_t nq, int64_t K, uint32_t lo, int shift, int n_bins, uint64_t *hist_dev)
{
    static const char *fn = "gl_feat_hist";
    gl_make_current(ctx);
    pair_sink<3> sink;
    bool above = false;
    if (const int rc = check_rows(fn, ctx, bank_V_dev, bank_norm_dev, n_rows, query_V_dev, query_norm_dev, nq, K, 32)) return rc;
    if (const int rc = make_hist_sink(fn, lo, shift, n_bins, hist_dev, n_rows > 0 && nq > 0, sink, above)) return rc;
    if (n_rows == 0 || nq == 0 || above) return GL_OK;
    return launch_split<3>(ctx, bank_V_dev, bank_norm_dev, n_rows, query_V_dev, query_norm_dev, nq, K, sink);
}

int gl_feat_pair_dist_h1_scaled(gl_ctx *ctx, const void *bank_V16_dev, const float *bank_norm_dev, int64_t n_rows, const void *query_V16_dev,
                                const float *query_norm_dev, int64_t nq, int64_t K1, float row_scale, float *out_dev, int64_t ld)
{
    static const char *fn = "gl_feat_pair_dist_h1_scaled";
    gl_make_current(ctx);
    pair_sink<1> sink;
    if (const int rc = check_rows(fn, ctx, bank_V16_dev, bank_norm_dev, n_rows, query_V16_dev, query_norm_dev, nq, K1, 64)) return rc;
    if (const int rc = make_dist_sink(fn, out_dev, ld, n_rows, n_rows > 0 && nq > 0, sink)) return rc;
    if (n_rows == 0 || nq == 0) return GL_OK;
    return launch_h1<1>(fn, ctx, bank_V16_dev, bank_norm_dev, n_rows, query_V16_dev, query_norm_dev, nq, K1, row_scale, sink);
}

int gl_feat_pair_dist(gl_ctx *ctx, const float *bank_V_dev, const float *bank_norm_dev, int64_t n_rows, const float *query_V_dev,
                      const float *query_norm_dev, int64_t nq, int64_t K, float *out_dev, int64_t ld)
{
    static const char *fn = "gl_feat_pair_dist";
    gl_make_current(ctx);
    pair_sink<1> sink;
    if (const int rc = check_rows(fn, ctx, bank_V_dev, bank_norm_dev, n_rows, query_V_dev, query_norm_dev, nq, K, 32)) return rc;
    if (const int rc = make_dist_sink(fn, out_dev, ld, n_rows, n_rows > 0 && nq > 0, sink)) return rc;
    if (n_rows == 0 || nq == 0) return GL_OK;
    return launch_split<1>(ctx, bank_V_dev, bank_norm_dev, n_rows, query_V_dev, query_norm_dev, nq, K, sink);
}

int gl_feat_topk_h1_scaled(gl_ctx *ctx, const void *bank_V16_dev, const float *bank_norm_dev, int64_t n_rows, int64_t index_base,
                           const void *query_V16_dev, const float *query_norm_dev, int64_t nq, int64_t K1, float row_scale, int k, uint64_t *topk_keys_dev)
{
    return feat_topk_impl<true>("gl_feat_topk_h1_scaled", ctx, bank_V16_dev, bank_norm_dev, n_rows, index_base, query_V16_dev, query_norm_dev, nq, K1,
                                row_scale, k, topk_keys_dev);
}

int gl_feat_topk(gl_ctx *ctx, const float *bank_V_dev, const float *bank_norm_dev, int64_t n_rows, int64_t index_base, const float *query_V_dev,
                 const float *query_norm_dev, int64_t nq, int64_t K, int k, uint64_t *topk_keys_dev)
{
    return feat_topk_impl<false>("gl_feat_topk", ctx, bank_V_dev, bank_norm_dev, n_rows, index_base, query_V_dev, query_norm_dev, nq, K, 1.0f, k,
                                 topk_keys_dev);
}

}  // extern "C"
