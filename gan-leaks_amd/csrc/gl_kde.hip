// Kernel-density (soft-min) sums under the exact integer L2 distance: sums[q][t] += sum over n < n_rows of
// gl_kde_weight(S(q, n) - S0[q], coef[t]), the fixed-point weight 2^(-(S - S0) coef) in units of 2^-40 (gl_kde_epi.h); S0_dev[nq] int64 in
// device memory, coef[T] fp32 descending in host memory (gl_l2_kde_rows_i8, gl_l2_kde_rows_i8_wide).
//
// The kernels are those of gl_count_rows.hip -- gl_rows::tile128 in its three forms and gl_rows::tile256, chosen by the same tile rule --
// with gl_kde::kde_epilogue: the K loops are shared, only what is reduced from the accumulators differs.  The sums are 64-bit integer adds of
// a pure function of (S - S0, coef): a function of the multiset of pair distances, whatever the tile, the chunking or the sharding.  No
// pairwise value reaches HBM and there is no workspace.
#include "gl_rows_tile.h"
#include "gl_kde_epi.h"

namespace {

using namespace gl_rows;
using gl_kde::kde_args;

struct kde_rows_epi {
    const kde_args &a;
    unsigned long long *__restrict__ sums;
    template <int NI, typename ST, typename SOf>
    __device__ __forceinline__ void run(SOf s_of, int n_left, int64_t q0, int qcol0, int q_left, int tile_q, char *smem, int lane) const
    {
        gl_kde::kde_epilogue<NI, ST>(s_of, n_left, q0, qcol0, q_left, tile_q, a, sums, smem, lane);
    }
};

// The 128 x 128 tile.  BIG = false: d <= 66051 (S < 2^32); BIG = true: 64-bit totals, NT = int32_t (d <= 262143) or int64_t (the wide form).
template <bool BIG, typename NT>
__global__ void __launch_bounds__(THREADS, 2)
l2_kde_rows_i8_kernel(const int8_t *__restrict__ bank, const NT *__restrict__ bank_norm, int64_t n_rows, const int8_t *__restrict__ query,
                      const NT *__restrict__ query_norm, int64_t nq, int64_t stride, const kde_args args, unsigned long long *__restrict__ sums,
                      int q_tiles, int n_tiles)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 buffers][bank 16 KiB | query 16 KiB]
    tile128<BIG, NT>(bank, bank_norm, n_rows, query, query_norm, nq, stride, q_tiles, n_tiles, smem, kde_rows_epi{args, sums});
}

// The 256 x 256 tile, d <= 66051.
__global__ void __launch_bounds__(512, 2)
l2_kde_rows_i8_256p_kernel(const int8_t *__restrict__ bank, const int32_t *__restrict__ bank_norm, int64_t n_rows, const int8_t *__restrict__ query,
                           const int32_t *__restrict__ query_norm, int64_t nq, int64_t stride, const kde_args args,
                           unsigned long long *__restrict__ sums, int q_tiles, int n_tiles)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    tile256(bank, bank_norm, n_rows, query, query_norm, nq, stride, q_tiles, n_tiles, smem, kde_rows_epi{args, sums});
}

template <typename NT>
int kde_rows_impl(const char *fn, gl_ctx *ctx, const int8_t *bank, const NT *bank_norm, int64_t n_rows, const int8_t *query, const NT *query_norm,
                  int64_t nq, int64_t d, const int64_t *s0_dev, const float *coef, int n_coef, uint64_t *sums)
{
    constexpr bool WIDE = sizeof(NT) == 8;
    const int64_t max_d = WIDE ? GL_L2_WIDE_MAX_D : GL_L2_MAX_D;
    gl_make_current(ctx);
    GL_REQUIRE(ctx, "%s: NULL ctx", fn);
    GL_REQUIRE(n_rows >= 0 && nq >= 0 && d > 0 && d <= max_d, "%s: bad sizes n_rows=%lld nq=%lld d=%lld (d <= %lld)", fn, (long long)n_rows,
               (long long)nq, (long long)d, (long long)max_d);
    GL_REQUIRE(n_coef >= 1 && n_coef <= GL_COUNT_MAX_T, "%s: n_coef=%d outside [1, %d]", fn, n_coef, GL_COUNT_MAX_T);
    GL_REQUIRE(coef, "%s: NULL coefficients", fn);
    kde_args a;
    for (int t = 0; t < GL_COUNT_MAX_T; ++t) a.coef[t] = 0.0f;
    for (int t = 0; t < n_coef; ++t) {
        GL_REQUIRE(coef[t] >= 0.0f && coef[t] <= 3.402823466e38f, "%s: coef[%d] is not a finite value >= 0", fn, t);
        GL_REQUIRE(t == 0 || coef[t] <= coef[t - 1], "%s: the coefficients must be descending (coef[%d] > coef[%d])", fn, t, t - 1);
        a.coef[t] = coef[t];
    }
    if (n_rows == 0 || nq == 0) return GL_OK;
    GL_REQUIRE(s0_dev, "%s: NULL offsets", fn);
    GL_REQUIRE((reinterpret_cast<uintptr_t>(s0_dev) & 7) == 0, "%s: the offsets must be 8-byte aligned", fn);
    GL_REQUIRE(bank && bank_norm && query && query_norm && sums, "%s: NULL device pointer", fn);
    GL_REQUIRE(((reinterpret_cast<uintptr_t>(bank) | reinterpret_cast<uintptr_t>(query)) & 15) == 0, "%s: prepared rows must be 16-byte aligned", fn);
    GL_REQUIRE((reinterpret_cast<uintptr_t>(sums) & 7) == 0, "%s: the sums must be 8-byte aligned", fn);
    const int64_t stride = gl_l2_row_stride(d);
    const bool big = WIDE || d > 66051;                  // 65025 * 66051 < 2^32
    // the tile gl_l2_count_rows_i8 would take
    const int force_tile = gl_tuning_int("GL_L2_TILE", 0);
    const bool t256 = !big && force_tile != 128 && (force_tile == 256 || gl_ceil_div(nq, BT) * gl_ceil_div(n_rows, BT) >= 1024);
    const int64_t tile = t256 ? BT : TILE_N;
    const int64_t qt = gl_ceil_div(nq, tile), nt = gl_ceil_div(n_rows, tile);
    GL_REQUIRE(qt * nt < (1ll << 31), "%s: grid too large", fn);
    unsigned long long *dst = reinterpret_cast<unsigned long long *>(sums);

    const int lds128 = 4 * OPER_BYTES;
    static_assert(gl_kde::KDE_LDS_BYTES <= 4 * OPER_BYTES, "sums, offsets and bounds must fit the slice buffers");
    static_assert(gl_kde::KDE_LDS_BYTES <= gl_pair256::LDS_BYTES, "sums, offsets and bounds must fit the slice buffers");
    GL_ONCE_PER_DEVICE(ctx, \
        GL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(l2_kde_rows_i8_kernel<false, int32_t>), hipFuncAttributeMaxDynamicSharedMemorySize, lds128)); \
        GL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(l2_kde_rows_i8_kernel<true, int32_t>), hipFuncAttributeMaxDynamicSharedMemorySize, lds128)); \
        GL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(l2_kde_rows_i8_kernel<true, int64_t>), hipFuncAttributeMaxDynamicSharedMemorySize, lds128)); \
        GL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(l2_kde_rows_i8_256p_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, gl_pair256::LDS_BYTES)););

    a.s0 = reinterpret_cast<const long long *>(s0_dev);
    a.cut = gl_kde_cut(a.coef[n_coef - 1]);
    a.s_max = (long long)(65025ull * (unsigned long long)d);
    a.flag = ctx->kde_flag;
    a.n = n_coef;
    {
        gl_prof_scope prof_(ctx, GL_PROF_L2_COUNT);
        const dim3 grid((unsigned)(qt * nt));
        if (!big) {
            if constexpr (!WIDE) {
                if (t256)
                    hipLaunchKernelGGL(l2_kde_rows_i8_256p_kernel, grid, dim3(512), gl_pair256::LDS_BYTES, ctx->stream, bank, bank_norm, n_rows, query,
                                       query_norm, nq, stride, a, dst, (int)qt, (int)nt);
                else
                    hipLaunchKernelGGL((l2_kde_rows_i8_kernel<false, int32_t>), grid, dim3(THREADS), lds128, ctx->stream, bank, bank_norm, n_rows, query,
                                       query_norm, nq, stride, a, dst, (int)qt, (int)nt);
            }
        } else {
            hipLaunchKernelGGL((l2_kde_rows_i8_kernel<true, NT>), grid, dim3(THREADS), lds128, ctx->stream, bank, bank_norm, n_rows, query, query_norm, nq,
                               stride, a, dst, (int)qt, (int)nt);
        }
        GL_LAUNCH_CHECK();
    }
    // the flag of pairs below their query's S0: read back and cleared, so the call waits for its kernel
    int below = 0;
    GL_HIP(hipMemcpyAsync(&below, ctx->kde_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    GL_HIP(hipMemsetAsync(ctx->kde_flag, 0, sizeof(int), ctx->stream));
    GL_HIP(hipStreamSynchronize(ctx->stream));
    GL_REQUIRE(!below, "%s: a pair lies below the offset S0 of its query (its weight would exceed 2^40); the sums of this call are unspecified", fn);
    return GL_OK;
}

}  // namespace

extern "C" {

int gl_l2_kde_rows_i8(gl_ctx *ctx, const int8_t *bank_i8_dev, const int32_t *bank_norm_dev, int64_t n_rows, const int8_t *query_i8_dev,
                      const int32_t *query_norm_dev, int64_t nq, int64_t d, const int64_t *S0_dev, const float *coef_host, int n_coef,
                      uint64_t *sums_dev)
{
    return kde_rows_impl<int32_t>("gl_l2_kde_rows_i8", ctx, bank_i8_dev, bank_norm_dev, n_rows, query_i8_dev, query_norm_dev, nq, d, S0_dev, coef_host,
                                  n_coef, sums_dev);
}

int gl_l2_kde_rows_i8_wide(gl_ctx *ctx, const int8_t *bank_i8_dev, const int64_t *bank_norm_dev, int64_t n_rows, const int8_t *query_i8_dev,
                           const int64_t *query_norm_dev, int64_t nq, int64_t d, const int64_t *S0_dev, const float *coef_host, int n_coef,
                           uint64_t *sums_dev)
{
    return kde_rows_impl<int64_t>("gl_l2_kde_rows_i8_wide", ctx, bank_i8_dev, bank_norm_dev, n_rows, query_i8_dev, query_norm_dev, nq, d, S0_dev,
                                  coef_host, n_coef, sums_dev);
}

int gl_kde_cut_bits_rows(const float *D0, int64_t n, float c, uint32_t *out)
{
    GL_REQUIRE(n >= 0 && (n == 0 || (D0 && out)), "gl_kde_cut_bits_rows: bad arguments");
    GL_REQUIRE(c >= 0.0f && c <= 3.402823466e38f, "gl_kde_cut_bits_rows: the coefficient is not a finite value >= 0");
    for (int64_t i = 0; i < n; ++i) {
        GL_REQUIRE(D0[i] >= 0.0f && D0[i] <= 3.402823466e38f, "gl_kde_cut_bits_rows: D0[%lld] is not a finite value >= 0", (long long)i);
        out[i] = gl_kde_cut_bits(D0[i], c);
    }
    return GL_OK;
}

}  // extern "C"
