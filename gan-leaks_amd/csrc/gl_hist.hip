// Histogram of the exact integer L2 distances of ALL pairs: hist[b] += #{ q < nq, n < n_rows : lo <= S(q, n) and (S(q, n) - lo) >> shift == b }
// for a window (lo, shift, n_bins) -- the primitive under attack.distance_quantiles, whose host radix-select zooms the window until the S at
// each requested rank is known exactly.
//
// The pairwise contraction is the one of the exact search and of the ball counts -- the K loops of gl_count.hip, repeated here as that file
// repeats gl_topk.hip's (128 x 128 tile, its 64-bit-total and wide forms, and the 256 x 256 tile on gl_pair256::mainloop), dispatched under
// the same rule -- with a different reduction: a bin per pair.  No pairwise value reaches HBM and there is no workspace.
//
// Epilogue: hist_epilogue (gl_hist_epi.h): every pair is binned, a per-workgroup table in LDS, one 64-bit atomicAdd per non-zero bin and
// workgroup; workgroups without a pair inside the window return early.
#include "gl_common.h"
#include "gl_hist_epi.h"
#include "gl_pair256.h"
#include <type_traits>

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int TILE_N = 128;   // bank rows per workgroup
constexpr int TILE_Q = 128;   // queries per workgroup
constexpr int TILE_K = 128;   // bytes of K per slice
constexpr int THREADS = 256;
constexpr int OPER_BYTES = TILE_N * TILE_K;
constexpr int BT = 256;       // rows per operand of the 256 x 256 tile

using gl_count::rows_left;
using gl_hist::hist_args;
using gl_hist::hist_epilogue;

// as in gl_count.hip / gl_topk.hip: 128 rows x 128 B per operand slice, 16-byte chunk c of row r at slot c ^ (r & 7)
__device__ __forceinline__ void stage_operand(const int8_t *__restrict__ base, int64_t row0, int64_t nrows_valid, int64_t stride, int64_t kbyte,
                                              char *lds_oper, int wave, int lane)
{
    const int rsub = lane >> 3, slot = lane & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int piece = wave * 4 + i;
        const int r = piece * 8 + rsub;
        int64_t gr = row0 + r;
        if (gr >= nrows_valid) gr = nrows_valid - 1;   // clamp: the epilogue masks rows beyond n_rows
        const int chunk = slot ^ (r & 7);
        gl_glds16(base + gr * stride + kbyte + chunk * 16, lds_oper + piece * 1024);
    }
}

__device__ __forceinline__ long long widen_norm(int32_t v) { return (long long)(unsigned)v; }   // int32 norms hold an unsigned value above d = 131071
__device__ __forceinline__ long long widen_norm(int64_t v) { return v; }

// The 128 x 128 tile (K loop of l2_count_i8_kernel).  BIG = false: d <= 66051, everything modulo 2^32 (S < 2^32).  BIG = true: int32 accumulators
// flushed into 64-bit totals every 64 KiB of K; NT = int32_t (d <= 262143) or int64_t (the wide form, d <= 2^24).
template <bool BIG, typename NT>
__global__ void __launch_bounds__(THREADS, 2)
l2_hist_i8_kernel(const int8_t *__restrict__ bank, const NT *__restrict__ bank_norm, int64_t n_rows, const int8_t *__restrict__ query,
                   const NT *__restrict__ query_norm, int64_t nq, int64_t stride,
                   const hist_args<typename std::conditional<BIG, unsigned long long, unsigned>::type> args, unsigned long long *__restrict__ hist,
                   int q_tiles, int n_tiles)
{
    typedef typename std::conditional<BIG, unsigned long long, unsigned>::type T;
    constexpr int FLUSH = 512;
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 buffers][bank 16 KiB | query 16 KiB]

    const unsigned nwg = (unsigned)q_tiles * (unsigned)n_tiles;
    const unsigned id = gl_xcd_remap(blockIdx.x, nwg);
    int qt, nt;
    gl_strip_order(id, q_tiles, n_tiles, qt, nt);
    const int64_t n0 = (int64_t)nt * TILE_N, q0 = (int64_t)qt * TILE_Q;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave >> 1, wq = wave & 1;
    const int frow = lane & 15, fk = lane >> 4;

    v4i acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (v4i){0, 0, 0, 0};
    long long tot[BIG ? 4 : 1][BIG ? 4 : 1][4] = {};
    auto flush = [&]() {
        if constexpr (BIG) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) { tot[i][j][r] += (long long)acc[i][j][r]; acc[i][j][r] = 0; }
        }
    };

    const int nk = (int)(stride / TILE_K);
    stage_operand(bank, n0, n_rows, stride, 0, smem, wave, lane);
    stage_operand(query, q0, nq, stride, 0, smem + OPER_BYTES, wave, lane);

    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();   // slice kt landed; everyone is done reading the other buffer
        char *cur = smem + (kt & 1) * 2 * OPER_BYTES;
        if (kt + 1 < nk) {
            char *nxt = smem + ((kt + 1) & 1) * 2 * OPER_BYTES;
            stage_operand(bank, n0, n_rows, stride, (int64_t)(kt + 1) * TILE_K, nxt, wave, lane);
            stage_operand(query, q0, nq, stride, (int64_t)(kt + 1) * TILE_K, nxt + OPER_BYTES, wave, lane);
        }
        const char *lb = cur + (wn * 64) * TILE_K;
        const char *lq = cur + OPER_BYTES + (wq * 64) * TILE_K;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int chunk = ks * 4 + fk;
            v4i a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = i * 16 + frow;
                a[i] = *reinterpret_cast<const v4i *>(lb + r * TILE_K + ((chunk ^ (r & 7)) << 4));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = j * 16 + frow;
                b[j] = *reinterpret_cast<const v4i *>(lq + r * TILE_K + ((chunk ^ (r & 7)) << 4));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (BIG && (kt % FLUSH) == FLUSH - 1) flush();
    }
    flush();

    // ---- epilogue.  C layout of the 16x16 tile: column (query) = lane & 15, row (bank) = (lane >> 4) * 4 + reg.  S replaces the dot products in
    // place (exactly as the count epilogue forms it), so that no norm stays live next to the accumulators.
    const int64_t nbase = n0 + wn * 64 + fk * 4;
    const int n_left = rows_left(n_rows, nbase), q_left = rows_left(nq, q0);
    const NT *bnp = bank_norm + nbase, *qnp = query_norm + q0;
    NT qn[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ql = wq * 64 + j * 16 + frow;
        qn[j] = ql < q_left ? qnp[ql] : (NT)0;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const NT bn = i * 16 + r < n_left ? bnp[i * 16 + r] : (NT)0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (BIG) tot[i][j][r] = widen_norm(bn) + widen_norm(qn[j]) - 2ll * tot[i][j][r];
                else acc[i][j][r] = (int)((unsigned)bn + (unsigned)qn[j] - 2u * (unsigned)acc[i][j][r]);       // exact modulo 2^32, and S < 2^32
            }
        }
    auto s_of = [&](int i, int j, int r) -> T {
        if constexpr (BIG) return (unsigned long long)tot[i][j][r];
        else return (unsigned)acc[i][j][r];
    };
    hist_epilogue<4, T>(s_of, n_left, wq * 64, q_left, args, hist, smem, lane);
}

// The 256 x 256 tile on the shared software-pipelined main loop (gl_pair256.h), d <= 66051.
__global__ void __launch_bounds__(512, 2)
l2_hist_i8_256p_kernel(const int8_t *__restrict__ bank, const int32_t *__restrict__ bank_norm, int64_t n_rows, const int8_t *__restrict__ query,
                        const int32_t *__restrict__ query_norm, int64_t nq, int64_t stride, const hist_args<unsigned> args,
                        unsigned long long *__restrict__ hist, int q_tiles, int n_tiles)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const unsigned id = gl_xcd_remap(blockIdx.x, (unsigned)q_tiles * (unsigned)n_tiles);
    int qt, nt;
    {
        constexpr int STRIP = 4;
        const unsigned per_strip = (unsigned)STRIP * (unsigned)q_tiles;
        const int strip = (int)(id / per_strip);
        const unsigned r = id % per_strip;
        const int width = n_tiles - strip * STRIP < STRIP ? n_tiles - strip * STRIP : STRIP;
        nt = strip * STRIP + (int)(r % (unsigned)width);
        qt = (int)(r / (unsigned)width);
    }
    const int64_t n0 = (int64_t)nt * BT, q0 = (int64_t)qt * BT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave >> 2, wq = wave & 3;
    const int frow = lane & 15, fk = lane >> 4;

    const gl_pair256::Source sa = gl_pair256::make_source(reinterpret_cast<const char *>(bank), n0, n_rows, stride, wave, lane);
    const gl_pair256::Source sb = gl_pair256::make_source(reinterpret_cast<const char *>(query), q0, nq, stride, wave, lane);
    v4i acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (v4i){0, 0, 0, 0};
    gl_pair256::mainloop<v4i, 0, 8>(sa, sb, stride / TILE_K, smem, acc, wave, lane,
                              [](const v4i &a, const v4i &b, const v4i &c) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0); });

    // S replaces the dot products in place (as above)
    const int64_t nbase = n0 + wn * 128 + fk * 4;
    const int n_left = rows_left(n_rows, nbase), q_left = rows_left(nq, q0);
    const int32_t *bnp = bank_norm + nbase, *qnp = query_norm + q0;
    unsigned qn[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ql = wq * 64 + j * 16 + frow;
        qn[j] = ql < q_left ? (unsigned)qnp[ql] : 0u;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned bn = i * 16 + r < n_left ? (unsigned)bnp[i * 16 + r] : 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j][r] = (int)(bn + qn[j] - 2u * (unsigned)acc[i][j][r]);   // exact modulo 2^32, and S < 2^32
        }
    auto s_of = [&](int i, int j, int r) -> unsigned { return (unsigned)acc[i][j][r]; };
    hist_epilogue<8, unsigned>(s_of, n_left, wq * 64, q_left, args, hist, smem, lane);
}

template <typename NT>
int hist_impl(const char *fn, gl_ctx *ctx, const int8_t *bank, const NT *bank_norm, int64_t n_rows, const int8_t *query, const NT *query_norm,
              int64_t nq, int64_t d, int64_t lo, int shift, int n_bins, uint64_t *hist)
{
    constexpr bool WIDE = sizeof(NT) == 8;
    const int64_t max_d = WIDE ? GL_L2_WIDE_MAX_D : GL_L2_MAX_D;
    gl_make_current(ctx);
    GL_REQUIRE(ctx, "%s: NULL ctx", fn);
    GL_REQUIRE(n_rows >= 0 && nq >= 0 && d > 0 && d <= max_d, "%s: bad sizes n_rows=%lld nq=%lld d=%lld (d <= %lld)", fn, (long long)n_rows,
               (long long)nq, (long long)d, (long long)max_d);
    GL_REQUIRE(n_bins >= 1 && n_bins <= GL_HIST_MAX_BINS, "%s: n_bins=%d outside [1, %d]", fn, n_bins, GL_HIST_MAX_BINS);
    GL_REQUIRE(shift >= 0 && shift <= 40, "%s: shift=%d outside [0, 40]", fn, shift);
    GL_REQUIRE(lo >= 0, "%s: lo=%lld is negative", fn, (long long)lo);
    if (n_rows == 0 || nq == 0) return GL_OK;
    GL_REQUIRE(bank && bank_norm && query && query_norm && hist, "%s: NULL device pointer", fn);
    GL_REQUIRE(((reinterpret_cast<uintptr_t>(bank) | reinterpret_cast<uintptr_t>(query)) & 15) == 0, "%s: prepared rows must be 16-byte aligned", fn);
    GL_REQUIRE((reinterpret_cast<uintptr_t>(hist) & 7) == 0, "%s: the histogram must be 8-byte aligned", fn);
    const int64_t stride = gl_l2_row_stride(d);
    const bool big = WIDE || d > 66051;                  // 65025 * 66051 < 2^32
    // the tile gl_l2_count_i8 would take
    const int force_tile = gl_tuning_int("GL_L2_TILE", 0);
    const bool t256 = !big && force_tile != 128 && (force_tile == 256 || gl_ceil_div(nq, BT) * gl_ceil_div(n_rows, BT) >= 1024);
    const int64_t tile = t256 ? BT : TILE_N;
    const int64_t qt = gl_ceil_div(nq, tile), nt = gl_ceil_div(n_rows, tile);
    GL_REQUIRE(qt * nt < (1ll << 31), "%s: grid too large", fn);
    unsigned long long *dst = reinterpret_cast<unsigned long long *>(hist);

    const int lds128 = 4 * OPER_BYTES;
    static_assert(GL_HIST_MAX_BINS * 4 <= 4 * OPER_BYTES && GL_HIST_MAX_BINS * 4 <= gl_pair256::LDS_BYTES, "the bin table lives in the slice buffers");
    GL_ONCE_PER_DEVICE(ctx, \
        GL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(l2_hist_i8_kernel<false, int32_t>), hipFuncAttributeMaxDynamicSharedMemorySize, lds128)); \
        GL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(l2_hist_i8_kernel<true, int32_t>), hipFuncAttributeMaxDynamicSharedMemorySize, lds128)); \
        GL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(l2_hist_i8_kernel<true, int64_t>), hipFuncAttributeMaxDynamicSharedMemorySize, lds128)); \
        GL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(l2_hist_i8_256p_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, gl_pair256::LDS_BYTES)););

    if ((unsigned long long)lo > 65025ull * (unsigned long long)d) return GL_OK;   // S <= 65025 d: the window lies above every pair
    const unsigned long long last = (unsigned long long)lo + ((unsigned long long)n_bins << shift) - 1ull;   // the largest S of the window; < 2^53
    gl_prof_scope prof_(ctx, GL_PROF_L2_HIST);
    const dim3 grid((unsigned)(qt * nt));
    if (!big) {
        const hist_args<unsigned> a = {(unsigned)lo, (unsigned)(last < 0xFFFFFFFFull ? last : 0xFFFFFFFFull), shift, n_bins};   // lo <= 65025 d < 2^32 here
        if constexpr (!WIDE) {
            if (t256)
                hipLaunchKernelGGL(l2_hist_i8_256p_kernel, grid, dim3(512), gl_pair256::LDS_BYTES, ctx->stream, bank, bank_norm, n_rows, query, query_norm, nq,
                                   stride, a, dst, (int)qt, (int)nt);
            else
                hipLaunchKernelGGL((l2_hist_i8_kernel<false, int32_t>), grid, dim3(THREADS), lds128, ctx->stream, bank, bank_norm, n_rows, query, query_norm,
                                   nq, stride, a, dst, (int)qt, (int)nt);
        }
    } else {
        const hist_args<unsigned long long> a = {(unsigned long long)lo, last, shift, n_bins};
        hipLaunchKernelGGL((l2_hist_i8_kernel<true, NT>), grid, dim3(THREADS), lds128, ctx->stream, bank, bank_norm, n_rows, query, query_norm, nq, stride,
                           a, dst, (int)qt, (int)nt);
    }
    GL_LAUNCH_CHECK();
    return GL_OK;
}

}  // namespace

extern "C" {

int gl_hist_init(gl_ctx *ctx, uint64_t *hist_dev, int n_bins)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx, "gl_hist_init: NULL ctx");
    GL_REQUIRE(n_bins >= 1 && n_bins <= GL_HIST_MAX_BINS, "gl_hist_init: n_bins=%d outside [1, %d]", n_bins, GL_HIST_MAX_BINS);
    GL_REQUIRE(hist_dev, "gl_hist_init: NULL histogram");
    GL_HIP(hipMemsetAsync(hist_dev, 0, (size_t)n_bins * 8, ctx->stream));
    return GL_OK;
}

int gl_l2_hist_i8(gl_ctx *ctx, const int8_t *bank_i8_dev, const int32_t *bank_norm_dev, int64_t n_rows, const int8_t *query_i8_dev,
                  const int32_t *query_norm_dev, int64_t nq, int64_t d, int64_t lo, int shift, int n_bins, uint64_t *hist_dev)
{
    return hist_impl<int32_t>("gl_l2_hist_i8", ctx, bank_i8_dev, bank_norm_dev, n_rows, query_i8_dev, query_norm_dev, nq, d, lo, shift, n_bins, hist_dev);
}

int gl_l2_hist_i8_wide(gl_ctx *ctx, const int8_t *bank_i8_dev, const int64_t *bank_norm_dev, int64_t n_rows, const int8_t *query_i8_dev,
                       const int64_t *query_norm_dev, int64_t nq, int64_t d, int64_t lo, int shift, int n_bins, uint64_t *hist_dev)
{
    return hist_impl<int64_t>("gl_l2_hist_i8_wide", ctx, bank_i8_dev, bank_norm_dev, n_rows, query_i8_dev, query_norm_dev, nq, d, lo, shift, n_bins,
                              hist_dev);
}

}  // extern "C"
