// Epsilon-ball counts under the exact integer L2 distance with thresholds PER QUERY: counts[q][t] += #{ n < n_rows : S(q, n) <= thr[q][t] },
// thr_dev[nq][T] int64 in device memory, ascending within each row (gl_l2_count_rows_i8, gl_l2_count_rows_i8_wide).
//
// The kernels are those of gl_count.hip -- the 128 x 128 tile, its 64-bit-total and wide forms, the 256 x 256 tile on gl_pair256::mainloop, chosen
// by the same tile rule -- with the second form of count_epilogue (gl_count_epi.h): the lane's query columns bring their own thresholds.  The
// primitive under counts with one radius per query and under the exact k-th smallest S per query (attack.select_kth_rows: a host search over
// these counts, 16 thresholds per query and pass).  No pairwise value reaches HBM and there is no workspace.
#include "gl_rows_tile.h"

namespace {

using namespace gl_rows;
using gl_count::rows_args;
using gl_count::count_epilogue;

// the epilogue of these kernels: gl_count::count_epilogue with the thresholds of every query
struct count_rows_epi {
    const rows_args &a;
    unsigned long long *__restrict__ counts;
    template <int NI, typename ST, typename SOf>
    __device__ __forceinline__ void run(SOf s_of, int n_left, int64_t q0, int qcol0, int q_left, int tile_q, char *smem, int lane) const
    {
        count_epilogue<NI, ST>(s_of, n_left, q0, qcol0, q_left, tile_q, a, counts, smem, lane);
    }
};

// The 128 x 128 tile (gl_rows::tile128) with the per-query epilogue.  BIG = false: d <= 66051, everything modulo 2^32 (S < 2^32).  BIG = true: int32 accumulators
// flushed into 64-bit totals every 64 KiB of K; NT = int32_t (d <= 262143) or int64_t (the wide form, d <= 2^24).
template <bool BIG, typename NT>
__global__ void __launch_bounds__(THREADS, 2)
l2_count_rows_i8_kernel(const int8_t *__restrict__ bank, const NT *__restrict__ bank_norm, int64_t n_rows, const int8_t *__restrict__ query,
                        const NT *__restrict__ query_norm, int64_t nq, int64_t stride, const rows_args args, unsigned long long *__restrict__ counts,
                        int q_tiles, int n_tiles)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 buffers][bank 16 KiB | query 16 KiB]
    tile128<BIG, NT>(bank, bank_norm, n_rows, query, query_norm, nq, stride, q_tiles, n_tiles, smem, count_rows_epi{args, counts});
}

// The 256 x 256 tile on the shared software-pipelined main loop (gl_rows::tile256), d <= 66051.
__global__ void __launch_bounds__(512, 2)
l2_count_rows_i8_256p_kernel(const int8_t *__restrict__ bank, const int32_t *__restrict__ bank_norm, int64_t n_rows, const int8_t *__restrict__ query,
                        const int32_t *__restrict__ query_norm, int64_t nq, int64_t stride, const rows_args args,
                        unsigned long long *__restrict__ counts, int q_tiles, int n_tiles)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    tile256(bank, bank_norm, n_rows, query, query_norm, nq, stride, q_tiles, n_tiles, smem, count_rows_epi{args, counts});
}

template <typename NT>
int count_rows_impl(const char *fn, gl_ctx *ctx, const int8_t *bank, const NT *bank_norm, int64_t n_rows, const int8_t *query, const NT *query_norm,
                    int64_t nq, int64_t d, const int64_t *thr_dev, int n_thr, uint64_t *counts)
{
    constexpr bool WIDE = sizeof(NT) == 8;
    const int64_t max_d = WIDE ? GL_L2_WIDE_MAX_D : GL_L2_MAX_D;
    gl_make_current(ctx);
    GL_REQUIRE(ctx, "%s: NULL ctx", fn);
    GL_REQUIRE(n_rows >= 0 && nq >= 0 && d > 0 && d <= max_d, "%s: bad sizes n_rows=%lld nq=%lld d=%lld (d <= %lld)", fn, (long long)n_rows,
               (long long)nq, (long long)d, (long long)max_d);
    GL_REQUIRE(n_thr >= 1 && n_thr <= GL_COUNT_MAX_T, "%s: n_thr=%d outside [1, %d]", fn, n_thr, GL_COUNT_MAX_T);
    if (n_rows == 0 || nq == 0) return GL_OK;
    GL_REQUIRE(thr_dev, "%s: NULL thresholds", fn);
    GL_REQUIRE((reinterpret_cast<uintptr_t>(thr_dev) & 7) == 0, "%s: the thresholds must be 8-byte aligned", fn);
    GL_REQUIRE(bank && bank_norm && query && query_norm && counts, "%s: NULL device pointer", fn);
    GL_REQUIRE(((reinterpret_cast<uintptr_t>(bank) | reinterpret_cast<uintptr_t>(query)) & 15) == 0, "%s: prepared rows must be 16-byte aligned", fn);
    GL_REQUIRE((reinterpret_cast<uintptr_t>(counts) & 7) == 0, "%s: the counters must be 8-byte aligned", fn);
    const int64_t stride = gl_l2_row_stride(d);
    const bool big = WIDE || d > 66051;                  // 65025 * 66051 < 2^32
    // the tile gl_l2_count_i8 would take
    const int force_tile = gl_tuning_int("GL_L2_TILE", 0);
    const bool t256 = !big && force_tile != 128 && (force_tile == 256 || gl_ceil_div(nq, BT) * gl_ceil_div(n_rows, BT) >= 1024);
    const int64_t tile = t256 ? BT : TILE_N;
    const int64_t qt = gl_ceil_div(nq, tile), nt = gl_ceil_div(n_rows, tile);
    GL_REQUIRE(qt * nt < (1ll << 31), "%s: grid too large", fn);
    unsigned long long *dst = reinterpret_cast<unsigned long long *>(counts);

    const int lds128 = 4 * OPER_BYTES;
    static_assert(gl_count::ROWS_THR_OFFSET + TILE_Q * GL_COUNT_MAX_T * 8 <= 4 * OPER_BYTES, "counters and bounds must fit the slice buffers");
    static_assert(gl_count::ROWS_THR_OFFSET + BT * GL_COUNT_MAX_T * 4 <= gl_pair256::LDS_BYTES, "counters and bounds must fit the slice buffers");
    GL_ONCE_PER_DEVICE(ctx, \
        GL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(l2_count_rows_i8_kernel<false, int32_t>), hipFuncAttributeMaxDynamicSharedMemorySize, lds128)); \
        GL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(l2_count_rows_i8_kernel<true, int32_t>), hipFuncAttributeMaxDynamicSharedMemorySize, lds128)); \
        GL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(l2_count_rows_i8_kernel<true, int64_t>), hipFuncAttributeMaxDynamicSharedMemorySize, lds128)); \
        GL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(l2_count_rows_i8_256p_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, gl_pair256::LDS_BYTES)););

    gl_prof_scope prof_(ctx, GL_PROF_L2_COUNT);
    const dim3 grid((unsigned)(qt * nt));
    const rows_args a = {reinterpret_cast<const long long *>(thr_dev), (long long)(65025ull * (unsigned long long)d), n_thr};
    if (!big) {
        if constexpr (!WIDE) {
            if (t256)
                hipLaunchKernelGGL(l2_count_rows_i8_256p_kernel, grid, dim3(512), gl_pair256::LDS_BYTES, ctx->stream, bank, bank_norm, n_rows, query, query_norm,
                                   nq, stride, a, dst, (int)qt, (int)nt);
            else
                hipLaunchKernelGGL((l2_count_rows_i8_kernel<false, int32_t>), grid, dim3(THREADS), lds128, ctx->stream, bank, bank_norm, n_rows, query,
                                   query_norm, nq, stride, a, dst, (int)qt, (int)nt);
        }
    } else {
        hipLaunchKernelGGL((l2_count_rows_i8_kernel<true, NT>), grid, dim3(THREADS), lds128, ctx->stream, bank, bank_norm, n_rows, query, query_norm, nq,
                           stride, a, dst, (int)qt, (int)nt);
    }
    GL_LAUNCH_CHECK();
    return GL_OK;
}

}  // namespace

extern "C" {

int gl_l2_count_rows_i8(gl_ctx *ctx, const int8_t *bank_i8_dev, const int32_t *bank_norm_dev, int64_t n_rows, const int8_t *query_i8_dev,
                        const int32_t *query_norm_dev, int64_t nq, int64_t d, const int64_t *thr_dev, int n_thr, uint64_t *counts_dev)
{
    return count_rows_impl<int32_t>("gl_l2_count_rows_i8", ctx, bank_i8_dev, bank_norm_dev, n_rows, query_i8_dev, query_norm_dev, nq, d, thr_dev, n_thr,
                                    counts_dev);
}

int gl_l2_count_rows_i8_wide(gl_ctx *ctx, const int8_t *bank_i8_dev, const int64_t *bank_norm_dev, int64_t n_rows, const int8_t *query_i8_dev,
                             const int64_t *query_norm_dev, int64_t nq, int64_t d, const int64_t *thr_dev, int n_thr, uint64_t *counts_dev)
{
    return count_rows_impl<int64_t>("gl_l2_count_rows_i8_wide", ctx, bank_i8_dev, bank_norm_dev, n_rows, query_i8_dev, query_norm_dev, nq, d, thr_dev,
                                    n_thr, counts_dev);
}

}  // extern "C"
