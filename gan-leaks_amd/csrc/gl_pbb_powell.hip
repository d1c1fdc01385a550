// Powell's conjugate-direction method for the partial-black-box attack (GAN-Leaks, section 5.3 runs it per query), for all queries of a block
// in lock-step.  Every line search is a two-sided ladder of L step widths scored in one batched generator forward with the kernels the
// evolution strategy scores its population with (gl_pbb_group_min / gl_pbb_group_min_keys, gl_pbb_accept: gl_pbb.hip, not touched here).
// This file holds what is left, per-query arithmetic on the direction set U [nz + 1][nz] and its trial widths t [nz + 1], which never leave
// the device.  One sweep is
//     gl_pbb_powell_begin        z0 = z, f0 = S_prev = S_cur, the largest decrease so far = 0
//     for line i = 0 .. nz - 1 (the same i for every query):
//         gl_pbb_powell_candidates   z + (+-2^-(r >> 1) t[i]) U[i], r < L, clamped to [-z_max, z_max]
//         scoring and gl_pbb_accept  (gl_pbb.hip)
//         gl_pbb_powell_advance      the width of line i after the ladder was accepted or rejected, the largest decrease and its line
//     gl_pbb_powell_extrapolate  row nz = z - z0, z_e = z + (z - z0), scored by the caller
//     gl_pbb_powell_decide       Numerical Recipes' test on (f0, fN, fE, the largest decrease): flag, t[nz] = 2 or 0
//     line nz as above (a width of 0 makes every candidate z itself: never strictly closer, so the block stays in lock-step)
//     gl_pbb_powell_replace      where flag: row i_best <- row nz - 1, row nz - 1 <- row nz, widths with their rows
// gl_pbb_powell_init writes the identity and the first widths.  Nothing reads a tuning variable, nothing synchronises, nothing uses atomics.
#include "gl_common.h"

// every fp32 and fp64 product, sum and difference below is rounded on its own (see gl_pbb.hip): a numpy restatement reproduces U, t, z,
// flag and i_best bit for bit
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;

// 2^-j, 0 <= j <= 32, exactly
__device__ __forceinline__ float pow2_neg(int j) { return __uint_as_float((unsigned)(127 - j) << 23); }

__device__ __forceinline__ int wave_or(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    return v;
}

// the exact value of a key as a double: kind 0 the integer S (exact below 2^53), kind 1 the float32 whose pattern the low word holds
__device__ __forceinline__ double key_value(unsigned long long key, int kind)
{
    return kind ? (double)__uint_as_float((unsigned)key) : (double)key;
}

// ---------------------------------------------------------------------------------------------------------------- init
// one thread per element of U; the threads of column 0 also write the row's width
__global__ void __launch_bounds__(kThreads) powell_init_kernel(float *__restrict__ U, float *__restrict__ t, int64_t nq, int nz, float step0)
{
    const int64_t total = nq * ((int64_t)nz + 1) * nz;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t row = i / nz;                                      // q * (nz + 1) + line
        const int c = (int)(i - row * nz);
        const int64_t q = row / ((int64_t)nz + 1);
        const int64_t line = row - q * ((int64_t)nz + 1);
        U[i] = line == c ? 1.0f : 0.0f;                                  // line == nz matches no column: row nz is 0
        if (c == 0) t[row] = line < nz ? step0 : 0.0f;
    }
}

// ---------------------------------------------------------------------------------------------------------------- begin
// one thread per latent value; the threads of column 0 also write the query's scalars
__global__ void __launch_bounds__(kThreads) powell_begin_kernel(const float *__restrict__ z, const unsigned long long *__restrict__ S_cur,
                                                                float *__restrict__ z0, unsigned long long *__restrict__ f0,
                                                                unsigned long long *__restrict__ S_prev, double *__restrict__ drop_best,
                                                                int *__restrict__ i_best, int64_t nq, int nz)
{
    const int64_t total = nq * nz;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t q = i / nz;
        z0[i] = z[i];
        if (i - q * nz == 0) {
            const unsigned long long s = S_cur[q];
            f0[q] = s;
            S_prev[q] = s;
            drop_best[q] = 0.0;
            i_best[q] = 0;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- candidates
// one thread per candidate value
__global__ void __launch_bounds__(kThreads) powell_candidates_kernel(const float *__restrict__ z, const float *__restrict__ U, const float *__restrict__ t,
                                                                     int64_t nq, int nz, int line, int L, float z_max, float *__restrict__ out)
{
    const int64_t total = nq * (int64_t)L * nz;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t row = i / nz;
        const int c = (int)(i - row * nz);
        const int64_t q = row / L;
        const int r = (int)(row - q * L);
        const int64_t urow = q * ((int64_t)nz + 1) + line;
        const float mag = pow2_neg(r >> 1);
        const float w = (r & 1) ? -mag : mag;
        const float a = w * t[urow];
        const float step = a * U[urow * nz + c];
        const float v = z[q * nz + c] + step;
        out[i] = fminf(fmaxf(v, -z_max), z_max);
    }
}

// ---------------------------------------------------------------------------------------------------------------- advance
// one thread per query
__global__ void __launch_bounds__(kThreads) powell_advance_kernel(float *__restrict__ t, const uint8_t *__restrict__ accepted, const int *__restrict__ j_new,
                                                                  const unsigned long long *__restrict__ S_cur, unsigned long long *__restrict__ S_prev,
                                                                  double *__restrict__ drop_best, int *__restrict__ i_best, int64_t nq, int nz, int line,
                                                                  int L, int kind, float t_min, float t_max)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    float *tq = t + q * ((int64_t)nz + 1) + line;
    const float w = *tq;
    if (accepted[q]) {
        const int r = j_new[q];
        if (r >= 0 && r < L) {
            const float twice = 2.0f * w;
            *tq = fminf(t_max, twice * pow2_neg(r >> 1));                // the next ladder starts one rung above the one that won
        }
    } else {
        *tq = fmaxf(t_min, w * pow2_neg(L >> 1));                        // the next ladder goes on below where this one ended
    }
    if (line < nz) {
        const unsigned long long s = S_cur[q];
        const double drop = key_value(S_prev[q], kind) - key_value(s, kind);
        if (drop > drop_best[q]) {
            drop_best[q] = drop;
            i_best[q] = line;
        }
        S_prev[q] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------- extrapolate
// one thread per latent value
__global__ void __launch_bounds__(kThreads) powell_extrapolate_kernel(const float *__restrict__ z, const float *__restrict__ z0, float *__restrict__ U,
                                                                      int64_t nq, int nz, float z_max, float *__restrict__ z_e)
{
    const int64_t total = nq * nz;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t q = i / nz;
        const int c = (int)(i - q * nz);
        const float zc = z[i];
        const float dz = zc - z0[i];
        U[(q * ((int64_t)nz + 1) + nz) * nz + c] = dz;
        const float v = zc + dz;
        z_e[i] = fminf(fmaxf(v, -z_max), z_max);
    }
}

// ---------------------------------------------------------------------------------------------------------------- decide
// one wave per query: the lanes look for a non-zero element of row nz, lane 0 evaluates the test
__global__ void __launch_bounds__(64) powell_decide_kernel(const float *__restrict__ U, float *__restrict__ t, const unsigned long long *__restrict__ f0_key,
                                                           const unsigned long long *__restrict__ S_cur, const unsigned long long *__restrict__ S_e,
                                                           const double *__restrict__ drop_best, uint8_t *__restrict__ flag, int nz, int kind)
{
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const float *dz = U + (q * ((int64_t)nz + 1) + nz) * nz;
    int moved = 0;
    for (int c = lane; c < nz; c += 64) moved |= dz[c] != 0.0f ? 1 : 0;
    moved = wave_or(moved);
    if (lane == 0) {
        const double f0 = key_value(f0_key[q], kind), fN = key_value(S_cur[q], kind), fE = key_value(S_e[q], kind), delta = drop_best[q];
        bool set = false;
        if (moved && fE < f0) {
            const double twoN = 2.0 * fN;
            const double a0 = f0 - twoN;
            const double a = a0 + fE;                                    // f0 - 2 fN + fE
            const double b0 = f0 - fN;
            const double b = b0 - delta;                                 // f0 - fN - delta
            const double bb = b * b;
            const double a2 = 2.0 * a;
            const double lhs = a2 * bb;
            const double c0 = f0 - fE;
            const double cc = c0 * c0;
            const double rhs = delta * cc;
            set = lhs < rhs;
        }
        flag[q] = set ? 1 : 0;
        t[q * ((int64_t)nz + 1) + nz] = set ? 2.0f : 0.0f;
    }
}

// ---------------------------------------------------------------------------------------------------------------- replace
// one wave per query, lane l owning elements l, l + 64, ...: a lane reads and writes only its own columns, so the two moves need no barrier
__global__ void __launch_bounds__(64) powell_replace_kernel(float *__restrict__ U, float *__restrict__ t, const uint8_t *__restrict__ flag,
                                                            const int *__restrict__ i_best, int nz)
{
    const int64_t q = blockIdx.x;
    if (!flag[q]) return;                                                // wave-uniform
    const int lane = threadIdx.x;
    int ib = i_best[q];
    ib = ib < 0 ? 0 : (ib > nz - 1 ? nz - 1 : ib);                       // whatever the caller uploaded, no row outside the query's own is touched
    float *Uq = U + q * ((int64_t)nz + 1) * nz;
    float *tq = t + q * ((int64_t)nz + 1);
    float *dst = Uq + (int64_t)ib * nz, *last = Uq + (int64_t)(nz - 1) * nz;
    const float *extra = Uq + (int64_t)nz * nz;
    for (int c = lane; c < nz; c += 64) {
        dst[c] = last[c];
        last[c] = extra[c];
    }
    if (lane == 0) {
        tq[ib] = tq[nz - 1];
        tq[nz - 1] = tq[nz];
    }
}

static inline bool finite_f(float x) { return x == x && x <= 3.402823466e38f && x >= -3.402823466e38f; }
static inline bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
static inline unsigned grid_for(int64_t total)
{
    int64_t blocks = gl_ceil_div(total, kThreads);
    if (blocks > 65536) blocks = 65536;
    return (unsigned)blocks;
}

}  // namespace

// sizes every entry shares: nq queries of nz latent values, and the direction rows nq * (nz + 1) * nz floats must be addressable
#define POWELL_SIZES(name)                                                                                                                     \
    GL_REQUIRE(ctx, name ": NULL ctx");                                                                                                        \
    GL_REQUIRE(nq >= 0 && nq < (1ll << 31) && nz >= 1 && nz < (1ll << 31) - 1, name ": bad sizes nq=%lld nz=%lld", (long long)nq, (long long)nz); \
    GL_REQUIRE(nq == 0 || nq <= INT64_MAX / 4 / (nz + 1) / nz, name ": nq * (nz + 1) * nz overflows")
#define POWELL_LADDER(name)                                                                                                                    \
    GL_REQUIRE(ladder >= 2 && ladder <= GL_PBB_POWELL_MAX_LADDER && (ladder & 1) == 0, name ": the ladder L=%lld must be even and lie in 2..%d", \
               (long long)ladder, GL_PBB_POWELL_MAX_LADDER);                                                                                   \
    GL_REQUIRE(line >= 0 && line <= nz, name ": line=%lld must lie in 0..nz=%lld", (long long)line, (long long)nz)

extern "C" {

int gl_pbb_powell_init(gl_ctx *ctx, float *U_dev, float *t_dev, int64_t nq, int64_t nz, float step0)
{
    gl_make_current(ctx);
    POWELL_SIZES("gl_pbb_powell_init");
    GL_REQUIRE(finite_f(step0) && step0 > 0.0f, "gl_pbb_powell_init: step0 must be finite and positive");
    if (nq == 0) return GL_OK;
    GL_REQUIRE(U_dev && t_dev, "gl_pbb_powell_init: NULL device pointer");
    GL_REQUIRE(aligned_to(U_dev, 4) && aligned_to(t_dev, 4), "gl_pbb_powell_init: U_dev and t_dev must be 4-byte aligned");
    hipLaunchKernelGGL(powell_init_kernel, dim3(grid_for(nq * (nz + 1) * nz)), dim3(kThreads), 0, ctx->stream, U_dev, t_dev, nq, (int)nz, step0);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int gl_pbb_powell_begin(gl_ctx *ctx, const float *z_dev, const uint64_t *S_cur_dev, float *z0_dev, uint64_t *f0_dev, uint64_t *S_prev_dev,
                        double *drop_best_dev, int32_t *i_best_dev, int64_t nq, int64_t nz)
{
    gl_make_current(ctx);
    POWELL_SIZES("gl_pbb_powell_begin");
    if (nq == 0) return GL_OK;
    GL_REQUIRE(z_dev && S_cur_dev && z0_dev && f0_dev && S_prev_dev && drop_best_dev && i_best_dev, "gl_pbb_powell_begin: NULL device pointer");
    GL_REQUIRE(aligned_to(z_dev, 4) && aligned_to(z0_dev, 4) && aligned_to(i_best_dev, 4) && aligned_to(S_cur_dev, 8) && aligned_to(f0_dev, 8) &&
                   aligned_to(S_prev_dev, 8) && aligned_to(drop_best_dev, 8),
               "gl_pbb_powell_begin: z_dev, z0_dev, i_best_dev must be 4-byte and S_cur_dev, f0_dev, S_prev_dev, drop_best_dev 8-byte aligned");
    hipLaunchKernelGGL(powell_begin_kernel, dim3(grid_for(nq * nz)), dim3(kThreads), 0, ctx->stream, z_dev,
                       reinterpret_cast<const unsigned long long *>(S_cur_dev), z0_dev, reinterpret_cast<unsigned long long *>(f0_dev),
                       reinterpret_cast<unsigned long long *>(S_prev_dev), drop_best_dev, i_best_dev, nq, (int)nz);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int gl_pbb_powell_candidates(gl_ctx *ctx, const float *z_dev, const float *U_dev, const float *t_dev, int64_t nq, int64_t nz, int64_t line,
                             int64_t ladder, float z_max, float *out_dev)
{
    gl_make_current(ctx);
    POWELL_SIZES("gl_pbb_powell_candidates");
    POWELL_LADDER("gl_pbb_powell_candidates");
    GL_REQUIRE(finite_f(z_max) && z_max > 0.0f, "gl_pbb_powell_candidates: z_max must be finite and positive");
    if (nq == 0) return GL_OK;
    GL_REQUIRE(nq <= INT64_MAX / 4 / ladder / nz, "gl_pbb_powell_candidates: nq * L * nz overflows");
    GL_REQUIRE(z_dev && U_dev && t_dev && out_dev, "gl_pbb_powell_candidates: NULL device pointer");
    GL_REQUIRE(aligned_to(z_dev, 4) && aligned_to(U_dev, 4) && aligned_to(t_dev, 4) && aligned_to(out_dev, 4),
               "gl_pbb_powell_candidates: z_dev, U_dev, t_dev and out_dev must be 4-byte aligned");
    hipLaunchKernelGGL(powell_candidates_kernel, dim3(grid_for(nq * ladder * nz)), dim3(kThreads), 0, ctx->stream, z_dev, U_dev, t_dev, nq, (int)nz,
                       (int)line, (int)ladder, z_max, out_dev);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int gl_pbb_powell_advance(gl_ctx *ctx, float *t_dev, const uint8_t *accepted_dev, const int32_t *j_new_dev, const uint64_t *S_cur_dev,
                          uint64_t *S_prev_dev, double *drop_best_dev, int32_t *i_best_dev, int64_t nq, int64_t nz, int64_t line, int64_t ladder,
                          int kind, float t_min, float t_max)
{
    gl_make_current(ctx);
    POWELL_SIZES("gl_pbb_powell_advance");
    POWELL_LADDER("gl_pbb_powell_advance");
    GL_REQUIRE(kind == 0 || kind == 1, "gl_pbb_powell_advance: kind=%d must be 0 (integer keys) or 1 (float32 patterns)", kind);
    GL_REQUIRE(finite_f(t_min) && finite_f(t_max) && t_min > 0.0f && t_min <= t_max, "gl_pbb_powell_advance: need 0 < t_min <= t_max, both finite");
    if (nq == 0) return GL_OK;
    GL_REQUIRE(t_dev && accepted_dev && j_new_dev && S_cur_dev && S_prev_dev && drop_best_dev && i_best_dev, "gl_pbb_powell_advance: NULL device pointer");
    GL_REQUIRE(aligned_to(t_dev, 4) && aligned_to(j_new_dev, 4) && aligned_to(i_best_dev, 4) && aligned_to(S_cur_dev, 8) && aligned_to(S_prev_dev, 8) &&
                   aligned_to(drop_best_dev, 8),
               "gl_pbb_powell_advance: t_dev, j_new_dev, i_best_dev must be 4-byte and S_cur_dev, S_prev_dev, drop_best_dev 8-byte aligned");
    hipLaunchKernelGGL(powell_advance_kernel, dim3((unsigned)gl_ceil_div(nq, kThreads)), dim3(kThreads), 0, ctx->stream, t_dev, accepted_dev, j_new_dev,
                       reinterpret_cast<const unsigned long long *>(S_cur_dev), reinterpret_cast<unsigned long long *>(S_prev_dev), drop_best_dev,
                       i_best_dev, nq, (int)nz, (int)line, (int)ladder, kind, t_min, t_max);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int gl_pbb_powell_extrapolate(gl_ctx *ctx, const float *z_dev, const float *z0_dev, float *U_dev, int64_t nq, int64_t nz, float z_max, float *z_e_dev)
{
    gl_make_current(ctx);
    POWELL_SIZES("gl_pbb_powell_extrapolate");
    GL_REQUIRE(finite_f(z_max) && z_max > 0.0f, "gl_pbb_powell_extrapolate: z_max must be finite and positive");
    if (nq == 0) return GL_OK;
    GL_REQUIRE(z_dev && z0_dev && U_dev && z_e_dev, "gl_pbb_powell_extrapolate: NULL device pointer");
    GL_REQUIRE(aligned_to(z_dev, 4) && aligned_to(z0_dev, 4) && aligned_to(U_dev, 4) && aligned_to(z_e_dev, 4),
               "gl_pbb_powell_extrapolate: z_dev, z0_dev, U_dev and z_e_dev must be 4-byte aligned");
    hipLaunchKernelGGL(powell_extrapolate_kernel, dim3(grid_for(nq * nz)), dim3(kThreads), 0, ctx->stream, z_dev, z0_dev, U_dev, nq, (int)nz, z_max,
                       z_e_dev);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int gl_pbb_powell_decide(gl_ctx *ctx, const float *U_dev, float *t_dev, const uint64_t *f0_dev, const uint64_t *S_cur_dev, const uint64_t *S_e_dev,
                         const double *drop_best_dev, uint8_t *flag_dev, int64_t nq, int64_t nz, int kind)
{
    gl_make_current(ctx);
    POWELL_SIZES("gl_pbb_powell_decide");
    GL_REQUIRE(kind == 0 || kind == 1, "gl_pbb_powell_decide: kind=%d must be 0 (integer keys) or 1 (float32 patterns)", kind);
    if (nq == 0) return GL_OK;
    GL_REQUIRE(U_dev && t_dev && f0_dev && S_cur_dev && S_e_dev && drop_best_dev && flag_dev, "gl_pbb_powell_decide: NULL device pointer");
    GL_REQUIRE(aligned_to(U_dev, 4) && aligned_to(t_dev, 4) && aligned_to(f0_dev, 8) && aligned_to(S_cur_dev, 8) && aligned_to(S_e_dev, 8) &&
                   aligned_to(drop_best_dev, 8),
               "gl_pbb_powell_decide: U_dev, t_dev must be 4-byte and f0_dev, S_cur_dev, S_e_dev, drop_best_dev 8-byte aligned");
    hipLaunchKernelGGL(powell_decide_kernel, dim3((unsigned)nq), dim3(64), 0, ctx->stream, U_dev, t_dev, reinterpret_cast<const unsigned long long *>(f0_dev),
                       reinterpret_cast<const unsigned long long *>(S_cur_dev), reinterpret_cast<const unsigned long long *>(S_e_dev), drop_best_dev,
                       flag_dev, (int)nz, kind);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int gl_pbb_powell_replace(gl_ctx *ctx, float *U_dev, float *t_dev, const uint8_t *flag_dev, const int32_t *i_best_dev, int64_t nq, int64_t nz)
{
    gl_make_current(ctx);
    POWELL_SIZES("gl_pbb_powell_replace");
    if (nq == 0) return GL_OK;
    GL_REQUIRE(U_dev && t_dev && flag_dev && i_best_dev, "gl_pbb_powell_replace: NULL device pointer");
    GL_REQUIRE(aligned_to(U_dev, 4) && aligned_to(t_dev, 4) && aligned_to(i_best_dev, 4), "gl_pbb_powell_replace: U_dev, t_dev and i_best_dev must be 4-byte aligned");
    hipLaunchKernelGGL(powell_replace_kernel, dim3((unsigned)nq), dim3(64), 0, ctx->stream, U_dev, t_dev, flag_dev, i_best_dev, (int)nz);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

}  // extern "C"
