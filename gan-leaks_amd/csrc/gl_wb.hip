// The white-box attack (GAN-Leaks, section 5.4: the attacker holds the generator's weights and finds z* = argmin_z L(x, G(z)) by gradient
// descent).  The gradient is gl_dcgan_l2_grad_z (gl_dcgan_grad.hip), the scoring and the best-so-far bookkeeping are gl_pbb_group_min and
// gl_pbb_accept with lambda = 1 (gl_pbb.hip); this file holds the optimiser step.
#include "gl_common.h"

// every fp32 product, sum, quotient and square root below is rounded on its own (see gl_pbb.hip): a numpy float32 restatement reproduces
// z, m and v bit for bit
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;

__global__ void __launch_bounds__(kThreads) wb_adam_kernel(float *__restrict__ z, float *__restrict__ m, float *__restrict__ v, const float *__restrict__ grad,
                                                           int64_t total, float lr, float beta1, float beta2, float eps, float c1, float c2, float z_max)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const float omb1 = 1.0f - beta1, omb2 = 1.0f - beta2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const float gi = grad[i];
        const float mi = beta1 * m[i] + omb1 * gi;
        const float vi = beta2 * v[i] + (omb2 * gi) * gi;
        const float mh = mi * c1, vh = vi * c2;
        const float den = sqrtf(vh) + eps;
        const float step = (lr * mh) / den;
        const float zi = z[i] - step;
        m[i] = mi;
        v[i] = vi;
        z[i] = fminf(fmaxf(zi, -z_max), z_max);
    }
}

// keys[i] = the uint32 pattern of M[i][i], zero-extended: the score of query i against its own image out of a block's pair distances
__global__ void __launch_bounds__(kThreads) wb_diag_keys_kernel(const float *__restrict__ M, int64_t n, int64_t ld, uint64_t *__restrict__ keys)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = (uint64_t)__float_as_uint(M[i * ld + i]);
}

static inline bool finite_f(float x) { return x == x && x <= 3.402823466e38f && x >= -3.402823466e38f; }

}  // namespace

extern "C" {

int gl_wb_adam_step(gl_ctx *ctx, float *z_dev, float *m_dev, float *v_dev, const float *grad_dev, int64_t nq, int64_t nz, float lr, float beta1,
                    float beta2, float eps, float c1, float c2, float z_max)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx, "gl_wb_adam_step: NULL ctx");
    GL_REQUIRE(nq >= 0 && nz >= 1 && nz < (1ll << 31) && nq <= INT64_MAX / nz, "gl_wb_adam_step: bad sizes nq=%lld nz=%lld", (long long)nq, (long long)nz);
    GL_REQUIRE(finite_f(lr) && lr > 0.0f && beta1 >= 0.0f && beta1 < 1.0f && beta2 >= 0.0f && beta2 < 1.0f && finite_f(eps) && eps > 0.0f,
               "gl_wb_adam_step: need lr > 0, 0 <= beta1, beta2 < 1 and eps > 0, all finite");
    GL_REQUIRE(finite_f(c1) && finite_f(c2) && c1 > 0.0f && c2 > 0.0f, "gl_wb_adam_step: the bias corrections c1, c2 must be finite and positive");
    GL_REQUIRE(finite_f(z_max) && z_max > 0.0f, "gl_wb_adam_step: z_max must be finite and positive");
    if (nq == 0) return GL_OK;
    GL_REQUIRE(z_dev && m_dev && v_dev && grad_dev, "gl_wb_adam_step: NULL device pointer");
    const int64_t total = nq * nz;
    int64_t blocks = gl_ceil_div(total, kThreads);
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(wb_adam_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, ctx->stream, z_dev, m_dev, v_dev, grad_dev, total, lr, beta1, beta2, eps,
                       c1, c2, z_max);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int gl_wb_diag_keys(gl_ctx *ctx, const float *M_dev, int64_t n, int64_t ld, uint64_t *keys_dev)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx, "gl_wb_diag_keys: NULL ctx");
    GL_REQUIRE(n >= 0 && ld >= n && (n == 0 || ld <= INT64_MAX / n), "gl_wb_diag_keys: bad sizes n=%lld ld=%lld", (long long)n, (long long)ld);
    if (n == 0) return GL_OK;
    GL_REQUIRE(M_dev && keys_dev, "gl_wb_diag_keys: NULL device pointer");
    hipLaunchKernelGGL(wb_diag_keys_kernel, dim3((unsigned)gl_ceil_div(n, kThreads)), dim3(kThreads), 0, ctx->stream, M_dev, n, ld, keys_dev);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

}  // extern "C"
