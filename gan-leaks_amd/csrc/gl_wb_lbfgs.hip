// L-BFGS for the white-box attack (GAN-Leaks, section 5.4 minimises over z with L-BFGS), for all queries of a block at once.  The line search
// is parallel: every query scores a ladder of L step widths along its direction in one batched forward, with the kernels the
// partial-black-box attack scores its population with (gl_pbb_group_min / gl_pbb_group_min_keys, gl_pbb_accept).  This file holds what is
// left, per-query vector arithmetic on [m][nz] histories that never leave the device.  One step is
//     the gradient g at z                (gl_dcgan_l2_grad_z, gl_pggan_l2_grad_z, ... : not touched here)
//     gl_wb_lbfgs_push        the pair (z - z_prev, g - g_prev) of a query that moved goes into its ring iff s.y > 0 and 1 / s.y is finite
//     gl_wb_lbfgs_direction   p = -H g by the two-loop recursion over the ring, -g where the ring is empty or H g is no descent direction
//     gl_wb_lbfgs_candidates  z + (t 2^-j) p, j < L, clamped to [-z_max, z_max]
//     scoring and gl_pbb_accept          (gl_pbb.hip)
//     gl_wb_lbfgs_advance     the trial width t and the ring after the ladder was accepted or rejected
// Nothing reads a tuning variable, nothing synchronises, nothing uses atomics.
#include "gl_common.h"

// every fp32 product, sum and quotient below is rounded on its own (see gl_wb.hip), and every dot product has ONE order -- lane l adds
// elements l, l + 64, ... in ascending order into a sum that starts at +0, then the lanes' sums go through the xor butterfly 32, 16, 8, 4,
// 2, 1 (a + b is commutative, so all lanes end with the same bits) -- so a numpy float32 restatement reproduces p, the ring and t bit for bit
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxM = GL_WB_LBFGS_MAX_M;

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int wave_or(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ bool finite_d(float x) { return fabsf(x) <= 3.402823466e38f; }        // false for NaN
// a trial width a query still works with; 0, negative and non-finite ones mark a finished query
__device__ __forceinline__ bool live_t(float t) { return t > 0.0f && t <= 3.402823466e38f; }
// 2^-j, 0 <= j <= 32, exactly
__device__ __forceinline__ float pow2_neg(int j) { return __uint_as_float((unsigned)(127 - j) << 23); }

// count and head as the kernels use them: whatever the caller uploaded, no row outside the query's own m is touched
__device__ __forceinline__ int ring_count(int k, int m) { return k < 0 ? 0 : (k > m ? m : k); }
__device__ __forceinline__ int ring_head(int h, int m) { return h >= 0 && h < m ? h : 0; }

// ---------------------------------------------------------------------------------------------------------------- push
// one wave per query
__global__ void __launch_bounds__(64) lbfgs_push_kernel(const float *__restrict__ z, const float *__restrict__ g, float *__restrict__ z_prev,
                                                        float *__restrict__ g_prev, float *__restrict__ S_hist, float *__restrict__ Y_hist,
                                                        int *__restrict__ count, int *__restrict__ head, const uint8_t *__restrict__ moved, int nz, int m)
{
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const float *zq = z + q * nz, *gq = g + q * nz;
    float *zp = z_prev + q * nz, *gp = g_prev + q * nz;
    if (moved[q]) {                                                      // wave-uniform
        float sy = 0.0f;
        for (int c = lane; c < nz; c += 64) {
            const float s = zq[c] - zp[c], y = gq[c] - gp[c];
            sy = sy + s * y;
        }
        sy = wave_sum(sy);
        const float rho = 1.0f / sy;
        if (sy > 0.0f && finite_d(rho)) {                                // the cautious update
            const int h = ring_head(head[q], m), k = ring_count(count[q], m);
            float *S = S_hist + (q * m + h) * nz, *Y = Y_hist + (q * m + h) * nz;
            for (int c = lane; c < nz; c += 64) {
                S[c] = zq[c] - zp[c];
                Y[c] = gq[c] - gp[c];
            }
            if (lane == 0) {
                head[q] = h + 1 == m ? 0 : h + 1;
                count[q] = k < m ? k + 1 : m;
            }
        }
    }
    for (int c = lane; c < nz; c += 64) {
        zp[c] = zq[c];
        gp[c] = gq[c];
    }
}

// ---------------------------------------------------------------------------------------------------------------- direction
// One wave per query.  The vector of the recursion lives in p (lane l owns elements l, l + 64, ...: a lane reads back only what it wrote),
// the ring rows are read once per loop, rho and alpha of the up to 16 pairs stay in registers (the loops are unrolled over the slot
// counter; every condition is wave-uniform).
__global__ void __launch_bounds__(64) lbfgs_direction_kernel(const float *__restrict__ g, const float *__restrict__ S_hist, const float *__restrict__ Y_hist,
                                                             int *__restrict__ count, int *__restrict__ head, float *__restrict__ t,
                                                             uint8_t *__restrict__ flag, int nz, int m, float step0, float *__restrict__ p)
{
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const float *gq = g + q * nz;
    float *pq = p + q * nz;
    const float t_in = t[q];
    if (!live_t(t_in)) {                                                 // finished: no direction, state as it is
        for (int c = lane; c < nz; c += 64) pq[c] = 0.0f;
        return;
    }
    const int k = ring_count(count[q], m), h = ring_head(head[q], m);
    const bool was_steepest = (flag[q] & GL_WB_LBFGS_STEEPEST) != 0;
    bool two_loop = k > 0, dropped = false;
    if (two_loop) {
        float rho[kMaxM], alpha[kMaxM];
        float gamma = 0.0f;
        for (int c = lane; c < nz; c += 64) pq[c] = gq[c];
#pragma unroll
        for (int i = 0; i < kMaxM; ++i) {                                // newest to oldest
            if (i < k) {
                int slot = h - 1 - i;
                if (slot < 0) slot += m;
                const float *S = S_hist + (q * m + slot) * nz, *Y = Y_hist + (q * m + slot) * nz;
                float sy = 0.0f, sq = 0.0f, yy = 0.0f;
                for (int c = lane; c < nz; c += 64) {
                    const float s = S[c], y = Y[c];
                    sy = sy + s * y;
                    sq = sq + s * pq[c];
                    yy = yy + y * y;
                }
                sy = wave_sum(sy);
                sq = wave_sum(sq);
                if (i == 0) gamma = sy / wave_sum(yy);
                rho[i] = 1.0f / sy;
                alpha[i] = rho[i] * sq;
                const float a = alpha[i];
                for (int c = lane; c < nz; c += 64) pq[c] = pq[c] - a * Y[c];
            }
        }
        for (int c = lane; c < nz; c += 64) pq[c] = gamma * pq[c];
#pragma unroll
        for (int i = kMaxM - 1; i >= 0; --i) {                           // oldest to newest
            if (i < k) {
                int slot = h - 1 - i;
                if (slot < 0) slot += m;
                const float *S = S_hist + (q * m + slot) * nz, *Y = Y_hist + (q * m + slot) * nz;
                float yr = 0.0f;
                for (int c = lane; c < nz; c += 64) yr = yr + Y[c] * pq[c];
                yr = wave_sum(yr);
                const float beta = rho[i] * yr;
                const float w = alpha[i] - beta;
                for (int c = lane; c < nz; c += 64) pq[c] = pq[c] + S[c] * w;
            }
        }
        float gp = 0.0f;
        int bad = 0;
        for (int c = lane; c < nz; c += 64) {
            const float v = -pq[c];
            pq[c] = v;
            gp = gp + gq[c] * v;
            bad |= finite_d(v) ? 0 : 1;
        }
        gp = wave_sum(gp);
        bad = wave_or(bad);
        if (bad || !(gp < 0.0f) || !finite_d(gp)) {                      // no descent direction: the ring goes, steepest descent runs
            two_loop = false;
            dropped = true;
        }
    }
    float t_out = 1.0f;
    if (!two_loop) {
        float gg = 0.0f;
        for (int c = lane; c < nz; c += 64) {
            const float v = gq[c];
            pq[c] = -v;
            gg = gg + v * v;
        }
        gg = wave_sum(gg);
        // consecutive steepest-descent steps carry their width on (gl_wb_lbfgs_advance); a first one starts at length step0
        t_out = was_steepest ? t_in : step0 / sqrtf(gg);
    }
    if (lane == 0) {
        t[q] = t_out;
        flag[q] = two_loop ? 0 : (dropped ? (GL_WB_LBFGS_STEEPEST | GL_WB_LBFGS_DROPPED) : GL_WB_LBFGS_STEEPEST);
        if (dropped) {
            count[q] = 0;
            head[q] = 0;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- candidates
// one thread per candidate value
__global__ void __launch_bounds__(kThreads) lbfgs_candidates_kernel(const float *__restrict__ z, const float *__restrict__ p, const float *__restrict__ t,
                                                                    int64_t nq, int nz, int L, float z_max, float *__restrict__ out)
{
    const int64_t total = nq * (int64_t)L * nz;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t row = i / nz;
        const int c = (int)(i - row * nz);
        const int64_t q = row / L;
        const int j = (int)(row - q * L);
        const float tq = t[q], zc = z[q * nz + c];
        if (!live_t(tq)) {                                               // finished: the iterate itself, which is never strictly closer
            out[i] = zc;
            continue;
        }
        const float w = tq * pow2_neg(j);
        const float step = w * p[q * nz + c];
        const float v = zc + step;
        out[i] = fminf(fmaxf(v, -z_max), z_max);
    }
}

// ---------------------------------------------------------------------------------------------------------------- advance
// one thread per query
__global__ void __launch_bounds__(kThreads) lbfgs_advance_kernel(float *__restrict__ t, int *__restrict__ count, int *__restrict__ head,
                                                                 const uint8_t *__restrict__ flag, const uint8_t *__restrict__ accepted,
                                                                 const int *__restrict__ j_new, int64_t nq, int L)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const float tq = t[q];
    if (!live_t(tq)) return;
    const bool steepest = (flag[q] & GL_WB_LBFGS_STEEPEST) != 0;
    if (accepted[q]) {
        const int j = j_new[q];
        if (steepest && j >= 0 && j < L) {
            const float twice = 2.0f * tq;
            t[q] = twice * pow2_neg(j);                                  // the next ladder starts one rung above the one that won
        }
    } else if (steepest) {
        t[q] = tq * pow2_neg(L);                                         // the next ladder goes on below where this one ended
    } else {
        count[q] = 0;                                                    // the quasi-Newton step did not improve: the ring goes
        head[q] = 0;
    }
}

static inline bool finite_f(float x) { return x == x && x <= 3.402823466e38f && x >= -3.402823466e38f; }

}  // namespace

extern "C" {

int gl_wb_lbfgs_push(gl_ctx *ctx, const float *z_dev, const float *grad_dev, float *z_prev_dev, float *g_prev_dev, float *S_hist_dev, float *Y_hist_dev,
                     int32_t *count_dev, int32_t *head_dev, const uint8_t *moved_dev, int64_t nq, int64_t nz, int64_t m)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx, "gl_wb_lbfgs_push: NULL ctx");
    GL_REQUIRE(nq >= 0 && nq < (1ll << 31) && nz >= 1 && nz < (1ll << 31), "gl_wb_lbfgs_push: bad sizes nq=%lld nz=%lld", (long long)nq, (long long)nz);
    GL_REQUIRE(m >= 1 && m <= kMaxM, "gl_wb_lbfgs_push: the memory m=%lld must lie in 1..%d", (long long)m, kMaxM);
    if (nq == 0) return GL_OK;
    GL_REQUIRE(nq <= INT64_MAX / 4 / m / nz, "gl_wb_lbfgs_push: nq * m * nz overflows");
    GL_REQUIRE(z_dev && grad_dev && z_prev_dev && g_prev_dev && S_hist_dev && Y_hist_dev && count_dev && head_dev && moved_dev,
               "gl_wb_lbfgs_push: NULL device pointer");
    hipLaunchKernelGGL(lbfgs_push_kernel, dim3((unsigned)nq), dim3(64), 0, ctx->stream, z_dev, grad_dev, z_prev_dev, g_prev_dev, S_hist_dev, Y_hist_dev,
                       count_dev, head_dev, moved_dev, (int)nz, (int)m);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int gl_wb_lbfgs_direction(gl_ctx *ctx, const float *grad_dev, const float *S_hist_dev, const float *Y_hist_dev, int32_t *count_dev, int32_t *head_dev,
                          float *t_dev, uint8_t *flag_dev, int64_t nq, int64_t nz, int64_t m, float step0, float *p_dev)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx, "gl_wb_lbfgs_direction: NULL ctx");
    GL_REQUIRE(nq >= 0 && nq < (1ll << 31) && nz >= 1 && nz < (1ll << 31), "gl_wb_lbfgs_direction: bad sizes nq=%lld nz=%lld", (long long)nq,
               (long long)nz);
    GL_REQUIRE(m >= 1 && m <= kMaxM, "gl_wb_lbfgs_direction: the memory m=%lld must lie in 1..%d", (long long)m, kMaxM);
    GL_REQUIRE(finite_f(step0) && step0 > 0.0f, "gl_wb_lbfgs_direction: step0 must be finite and positive");
    if (nq == 0) return GL_OK;
    GL_REQUIRE(nq <= INT64_MAX / 4 / m / nz, "gl_wb_lbfgs_direction: nq * m * nz overflows");
    GL_REQUIRE(grad_dev && S_hist_dev && Y_hist_dev && count_dev && head_dev && t_dev && flag_dev && p_dev, "gl_wb_lbfgs_direction: NULL device pointer");
    hipLaunchKernelGGL(lbfgs_direction_kernel, dim3((unsigned)nq), dim3(64), 0, ctx->stream, grad_dev, S_hist_dev, Y_hist_dev, count_dev, head_dev, t_dev,
                       flag_dev, (int)nz, (int)m, step0, p_dev);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int gl_wb_lbfgs_candidates(gl_ctx *ctx, const float *z_dev, const float *p_dev, const float *t_dev, int64_t nq, int64_t nz, int64_t ladder, float z_max,
                           float *out_dev)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx, "gl_wb_lbfgs_candidates: NULL ctx");
    GL_REQUIRE(nq >= 0 && nq < (1ll << 31) && nz >= 1 && nz < (1ll << 31), "gl_wb_lbfgs_candidates: bad sizes nq=%lld nz=%lld", (long long)nq,
               (long long)nz);
    GL_REQUIRE(ladder >= 1 && ladder <= GL_WB_LBFGS_MAX_LADDER, "gl_wb_lbfgs_candidates: the ladder L=%lld must lie in 1..%d", (long long)ladder,
               GL_WB_LBFGS_MAX_LADDER);
    GL_REQUIRE(finite_f(z_max) && z_max > 0.0f, "gl_wb_lbfgs_candidates: z_max must be finite and positive");
    if (nq == 0) return GL_OK;
    GL_REQUIRE(nq <= INT64_MAX / 4 / ladder / nz, "gl_wb_lbfgs_candidates: nq * L * nz overflows");
    GL_REQUIRE(z_dev && p_dev && t_dev && out_dev, "gl_wb_lbfgs_candidates: NULL device pointer");
    const int64_t total = nq * ladder * nz;
    int64_t blocks = gl_ceil_div(total, kThreads);
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(lbfgs_candidates_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, ctx->stream, z_dev, p_dev, t_dev, nq, (int)nz, (int)ladder, z_max,
                       out_dev);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int gl_wb_lbfgs_advance(gl_ctx *ctx, float *t_dev, int32_t *count_dev, int32_t *head_dev, const uint8_t *flag_dev, const uint8_t *accepted_dev,
                        const int32_t *j_new_dev, int64_t nq, int64_t ladder)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx, "gl_wb_lbfgs_advance: NULL ctx");
    GL_REQUIRE(nq >= 0 && nq < (1ll << 31), "gl_wb_lbfgs_advance: bad size nq=%lld", (long long)nq);
    GL_REQUIRE(ladder >= 1 && ladder <= GL_WB_LBFGS_MAX_LADDER, "gl_wb_lbfgs_advance: the ladder L=%lld must lie in 1..%d", (long long)ladder,
               GL_WB_LBFGS_MAX_LADDER);
    if (nq == 0) return GL_OK;
    GL_REQUIRE(t_dev && count_dev && head_dev && flag_dev && accepted_dev && j_new_dev, "gl_wb_lbfgs_advance: NULL device pointer");
    hipLaunchKernelGGL(lbfgs_advance_kernel, dim3((unsigned)gl_ceil_div(nq, kThreads)), dim3(kThreads), 0, ctx->stream, t_dev, count_dev, head_dev, flag_dev,
                       accepted_dev, j_new_dev, nq, (int)ladder);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

}  // extern "C"
