// The partial-black-box attack (GAN-Leaks, section 5.3: the attacker holds the generator and searches its latent space for
// z* = argmin_z L(x, G(z)) without gradients), as a population-based (1 + lambda) evolution strategy per query.  One round is
//     gl_pbb_candidates : lambda latents around every query's incumbent, z + sigma * eps with a counter-based noise eps
//     the generator     : all nq * lambda candidates in one pass (gl_dcgan_forward / gl_pggan_forward, not touched here)
//     gl_pbb_group_min  : every query against its OWN lambda images only -- exact S = sum (a - b)^2 and the minimum of (S, j)
//     gl_pbb_accept     : the winner replaces the incumbent where it is strictly closer; sigma grows on success and shrinks otherwise.
// Under 0.2 LPIPS + L2 the third step is gl_feat_pair_dist* on the candidates' search rows and gl_pbb_group_min_keys over the stored block
// of pair distances: the minimum of the uint32 patterns of every query's own lambda columns.
// Everything is a pure function of (seed, round, global query index, j, c) and of exact integers, so the result does not depend on how
// the queries are blocked or sharded.  No tuning variables are read.
#include "gl_common.h"

// every fp32 product and sum in this file is rounded on its own: a host restatement reproduces the candidates and the step widths bit for
// bit.  Plain * and + under this pragma: the header's __fmul_rn / __fadd_rn are compiled under the default (contract) and hipcc fuses
// __fadd_rn(z, __fmul_rn(sigma, eps)) into one fma all the same.
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;

// ---------------------------------------------------------------------------------------------------------------- noise
// Philox4x32-10 (Salmon et al., SC'11): 10 rounds of two 32 x 32 -> 64 multiplies and a word permutation; the key is bumped by the Weyl
// constants between rounds.  Integer operations only.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// eps(seed, round, query, j, c): Irwin-Hall with n = 8 on the eight 16-bit halves of one Philox call.  t = 2 sum h - 8 * 65535 is an exact
// int32 with |t| <= 524280 < 2^24, so float(t) is exact and eps is ONE rounded product: unit variance, support +-4.9.
__device__ __forceinline__ float pbb_noise(uint32_t k0, uint32_t k1, uint32_t round, uint32_t query, uint32_t j, uint32_t c)
{
    uint32_t w[4];
    philox4x32_10(c, j, query, round, k0, k1, w);
    int sum = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) sum += (int)(w[i] & 0xFFFFu) + (int)(w[i] >> 16);
    return (float)(2 * sum - 524280) * __uint_as_float(GL_PBB_NOISE_SCALE_BITS);
}

// one thread per candidate value: out[(q * lambda + j) * nz + c] = clamp(fl32(z[q][c] + fl32(sigma[q] * eps)), -z_max, z_max)
__global__ void __launch_bounds__(kThreads) pbb_candidates_kernel(const float *__restrict__ z, const float *__restrict__ sigma, int64_t nq, int nz,
                                                                  int lambda, uint32_t k0, uint32_t k1, uint32_t round, uint64_t query_base,
                                                                  float z_max, float *__restrict__ out)
{
    const int64_t total = nq * (int64_t)lambda * nz;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t row = i / nz;
        const int c = (int)(i - row * nz);
        const int64_t q = row / lambda;
        const int j = (int)(row - q * lambda);
        const float eps = pbb_noise(k0, k1, round, (uint32_t)(query_base + (uint64_t)q), (uint32_t)j, (uint32_t)c);
        const float step = sigma[q] * eps;
        const float v = z[q * nz + c] + step;
        out[i] = fminf(fmaxf(v, -z_max), z_max);
    }
}

// the reconstruction attack's posterior draws: gl_pbb_candidates with a width per coordinate, round 0 of the same noise, and draw 0 the mean
// itself.  out[(q * lambda + j) * nz + c] = clamp(fl32(mu[q][c] + fl32(std[q][c] * eps)), -z_max, z_max), eps = 0 for j = 0
__global__ void __launch_bounds__(kThreads) recon_latents_kernel(const float *__restrict__ mu, const float *__restrict__ sd, int64_t nq, int nz, int lambda,
                                                                 uint32_t k0, uint32_t k1, uint64_t query_base, float z_max, float *__restrict__ out)
{
    const int64_t total = nq * (int64_t)lambda * nz;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t row = i / nz;
        const int c = (int)(i - row * nz);
        const int64_t q = row / lambda;
        const int j = (int)(row - q * lambda);
        const float eps = j ? pbb_noise(k0, k1, 0u, (uint32_t)(query_base + (uint64_t)q), (uint32_t)j, (uint32_t)c) : 0.0f;
        const float step = sd[q * nz + c] * eps;
        const float v = mu[q * nz + c] + step;
        out[i] = fminf(fmaxf(v, -z_max), z_max);
    }
}

// ---------------------------------------------------------------------------------------------------------------- grouped distance
// Block (q, g): query q against candidates [g * GROUP, min(lambda, (g + 1) * GROUP)) of ITS lambda rows.  The query row goes through LDS in
// chunks of KC bytes; each of the four waves owns PER_WAVE whole candidates and streams them with 16-byte loads, so one LDS read of the
// query serves PER_WAVE candidate loads and every candidate byte is read once.  Per dword: sum b^2 and sum a b (v_dot4_u32_u8), plus
// sum a^2 once per query dword; S = sum a^2 + sum b^2 - 2 sum a b.  A lane adds at most KC / 1024 * 4 dot4 values of <= 4 * 255^2 into a
// uint32 per chunk (16.6 M at KC = 16384) and flushes into 64-bit totals after every chunk: exact for any d.
constexpr int GROUP = GL_PBB_GROUP;
constexpr int WAVES = kThreads / 64;
constexpr int PER_WAVE = GROUP / WAVES;
constexpr int KC = 16384;
static_assert(GROUP % WAVES == 0 && PER_WAVE == 4, "the wave loop below is written for four candidates per wave");

struct pbb_partial {
    unsigned long long S;
    int j;
    int pad;
};
static_assert(sizeof(pbb_partial) == GL_PBB_PARTIAL_BYTES, "workspace layout");

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// VEC: d % 16 == 0 and both base pointers 16-byte aligned, so every row starts on a 16-byte boundary.  Otherwise bytes, one per lane.
// ALL (gl_pbb_group_S): the same sums, every S(q, j) stored to all_S[q * lambda + j] instead of the minimum; part is not touched.
template <bool VEC, bool ALL = false>
__global__ void __launch_bounds__(kThreads) pbb_group_min_kernel(const uint8_t *__restrict__ queries, const uint8_t *__restrict__ cand, int lambda,
                                                                 int64_t d, pbb_partial *__restrict__ part, int64_t nq,
                                                                 unsigned long long *__restrict__ all_S = nullptr)
{
    __shared__ __attribute__((aligned(16))) uint8_t qs[KC];
    __shared__ pbb_partial wave_best[WAVES];
    const int64_t q = blockIdx.x;
    const int g = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j0 = g * GROUP + wave * PER_WAVE;
    const int n_valid = lambda - j0 < PER_WAVE ? (lambda - j0 < 0 ? 0 : lambda - j0) : PER_WAVE;
    const uint8_t *qrow = queries + q * d;
    // rows past lambda are not read: their slots alias the wave's last valid row and their results are dropped
    const uint8_t *crow[PER_WAVE];
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) {
        const int j = n_valid ? j0 + (i < n_valid ? i : n_valid - 1) : 0;
        crow[i] = cand + (q * (int64_t)lambda + j) * d;
    }
    unsigned long long aa = 0, bb[PER_WAVE] = {0, 0, 0, 0}, ab[PER_WAVE] = {0, 0, 0, 0};

    for (int64_t k0 = 0; k0 < d; k0 += KC) {
        const int kc = d - k0 < KC ? (int)(d - k0) : KC;
        if (k0) __syncthreads();                       // the previous chunk has been read by every wave
        if constexpr (VEC) {
            for (int o = threadIdx.x * 16; o < kc; o += kThreads * 16) *reinterpret_cast<uint4 *>(qs + o) = *reinterpret_cast<const uint4 *>(qrow + k0 + o);
        } else {
            for (int o = threadIdx.x; o < kc; o += kThreads) qs[o] = qrow[k0 + o];
        }
        __syncthreads();
        if (n_valid == 0) continue;                    // wave-uniform; the barriers above are still reached
        unsigned saa = 0, sbb[PER_WAVE] = {0, 0, 0, 0}, sab[PER_WAVE] = {0, 0, 0, 0};
        if constexpr (VEC) {
            for (int o = lane * 16; o < kc; o += 64 * 16) {
                const uint4 a = *reinterpret_cast<const uint4 *>(qs + o);
                uint4 b[PER_WAVE];
#pragma unroll
                for (int i = 0; i < PER_WAVE; ++i) b[i] = *reinterpret_cast<const uint4 *>(crow[i] + k0 + o);
                saa = __builtin_amdgcn_udot4(a.x, a.x, saa, false);
                saa = __builtin_amdgcn_udot4(a.y, a.y, saa, false);
                saa = __builtin_amdgcn_udot4(a.z, a.z, saa, false);
                saa = __builtin_amdgcn_udot4(a.w, a.w, saa, false);
#pragma unroll
                for (int i = 0; i < PER_WAVE; ++i) {
                    sbb[i] = __builtin_amdgcn_udot4(b[i].x, b[i].x, sbb[i], false);
                    sbb[i] = __builtin_amdgcn_udot4(b[i].y, b[i].y, sbb[i], false);
                    sbb[i] = __builtin_amdgcn_udot4(b[i].z, b[i].z, sbb[i], false);
                    sbb[i] = __builtin_amdgcn_udot4(b[i].w, b[i].w, sbb[i], false);
                    sab[i] = __builtin_amdgcn_udot4(a.x, b[i].x, sab[i], false);
                    sab[i] = __builtin_amdgcn_udot4(a.y, b[i].y, sab[i], false);
                    sab[i] = __builtin_amdgcn_udot4(a.z, b[i].z, sab[i], false);
                    sab[i] = __builtin_amdgcn_udot4(a.w, b[i].w, sab[i], false);
                }
            }
        } else {
            for (int o = lane; o < kc; o += 64) {
                const unsigned a = qs[o];
                saa += a * a;
#pragma unroll
                for (int i = 0; i < PER_WAVE; ++i) {
                    const unsigned b = crow[i][k0 + o];
                    sbb[i] += b * b;
                    sab[i] += a * b;
                }
            }
        }
        aa += saa;
#pragma unroll
        for (int i = 0; i < PER_WAVE; ++i) { bb[i] += sbb[i]; ab[i] += sab[i]; }
    }

    // (S, j) of the wave's best candidate: all lanes hold the same totals after the butterfly
    pbb_partial best;
    best.S = ~0ull; best.j = 0x7fffffff; best.pad = 0;
    if (n_valid) {
        const unsigned long long AA = wave_sum(aa);
#pragma unroll
        for (int i = 0; i < PER_WAVE; ++i) {
            const unsigned long long S = AA + wave_sum(bb[i]) - 2ull * wave_sum(ab[i]);
            if constexpr (ALL) {
                if (i < n_valid && lane == 0) all_S[q * (int64_t)lambda + j0 + i] = S;
            }
            if (i < n_valid && S < best.S) { best.S = S; best.j = j0 + i; }      // ascending j: strict < keeps the lower index on a tie
        }
    }
    if constexpr (ALL) return;                         // no barrier below is needed: every S has been stored by its own wave
    if (lane == 0) wave_best[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < WAVES; ++w)
            if (wave_best[w].S < best.S) best = wave_best[w];                     // waves in ascending j as well
        part[(int64_t)g * nq + q] = best;
    }
}

// one thread per query over its groups, in ascending j
__global__ void __launch_bounds__(kThreads) pbb_combine_kernel(const pbb_partial *__restrict__ part, int64_t nq, int groups,
                                                               unsigned long long *__restrict__ out_S, int *__restrict__ out_j)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    pbb_partial best = part[q];
    for (int g = 1; g < groups; ++g) {
        const pbb_partial p = part[(int64_t)g * nq + q];
        if (p.S < best.S) best = p;
    }
    out_S[q] = best.S;
    out_j[q] = best.j;
}

// ---------------------------------------------------------------------------------------------------------------- grouped minimum of keys
// The same reduction over a stored block of pair distances M (gl_feat_pair_dist*): one wave per query, four queries per workgroup.  The
// lanes stride over the query's own lambda columns (coalesced), each keeps the minimum of (pattern << 32) | j, and a butterfly leaves the
// wave's minimum in every lane: the smallest pattern, and among equal patterns the smallest j.  D32 >= +0, so the unsigned order of the
// patterns is the order of the floats.
__global__ void __launch_bounds__(kThreads) pbb_group_min_keys_kernel(const float *__restrict__ M, int64_t nq, int64_t lambda, int64_t ld,
                                                                      unsigned long long *__restrict__ keys, int *__restrict__ out_j)
{
    const int64_t q = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (q >= nq) return;                               // wave-uniform; no barrier below
    const int lane = threadIdx.x & 63;
    const float *row = M + q * ld + q * lambda;
    unsigned long long best = ~0ull;
    for (int64_t j = lane; j < lambda; j += 64) {
        const unsigned long long v = ((unsigned long long)__float_as_uint(row[j]) << 32) | (unsigned long long)j;
        best = v < best ? v : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = other < best ? other : best;
    }
    if (lane == 0) {
        keys[q] = best >> 32;
        out_j[q] = (int)(best & 0xffffffffull);
    }
}

// ---------------------------------------------------------------------------------------------------------------- accept
// one wave per query.  Every lane reads the decision before lane 0 overwrites S_cur.
__global__ void __launch_bounds__(64) pbb_accept_kernel(float *__restrict__ z, float *__restrict__ sigma, unsigned long long *__restrict__ S_cur,
                                                        const float *__restrict__ cand_z, const unsigned long long *__restrict__ S_new,
                                                        const int *__restrict__ j_new, int nz, int lambda, float up, float down, float sigma_min,
                                                        float sigma_max, uint8_t *__restrict__ accepted)
{
    const int64_t q = blockIdx.x;
    const unsigned long long s_new = S_new[q], s_cur = S_cur[q];
    const int j = j_new[q];
    const bool take = s_new < s_cur && j >= 0 && j < lambda;
    __syncthreads();
    if (take) {
        const float *src = cand_z + (q * (int64_t)lambda + j) * nz;
        for (int c = threadIdx.x; c < nz; c += 64) z[q * nz + c] = src[c];
    }
    if (threadIdx.x == 0) {
        if (take) S_cur[q] = s_new;
        const float s = sigma[q] * (take ? up : down);
        sigma[q] = fminf(fmaxf(s, sigma_min), sigma_max);
        accepted[q] = take ? 1 : 0;
    }
}

static inline bool finite_f(float v) { return v == v && v <= 3.402823466e38f && v >= -3.402823466e38f; }

}  // namespace

extern "C" {

int gl_pbb_candidates(gl_ctx *ctx, const float *z_dev, const float *sigma_dev, int64_t nq, int64_t nz, int64_t lambda, uint64_t seed, uint32_t round,
                      int64_t query_base, float z_max, float *out_dev)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx, "gl_pbb_candidates: NULL ctx");
    GL_REQUIRE(nq >= 0 && nz >= 1 && nz < (1ll << 31) && lambda >= 1 && lambda < (1ll << 31), "gl_pbb_candidates: bad sizes nq=%lld nz=%lld lambda=%lld",
               (long long)nq, (long long)nz, (long long)lambda);
    GL_REQUIRE(query_base >= 0 && nq <= (1ll << 32) && query_base <= (1ll << 32) - nq,
               "gl_pbb_candidates: query_base + nq = %lld + %lld exceeds 2^32 (the noise counter holds 32 bits of the query index)", (long long)query_base,
               (long long)nq);
    GL_REQUIRE(finite_f(z_max) && z_max > 0.0f, "gl_pbb_candidates: z_max must be finite and positive");
    if (nq == 0) return GL_OK;
    GL_REQUIRE(nq <= INT64_MAX / lambda / nz, "gl_pbb_candidates: nq * lambda * nz overflows");
    GL_REQUIRE(z_dev && sigma_dev && out_dev, "gl_pbb_candidates: NULL device pointer");
    const int64_t total = nq * lambda * nz;
    int64_t blocks = gl_ceil_div(total, kThreads);
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(pbb_candidates_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, ctx->stream, z_dev, sigma_dev, nq, (int)nz, (int)lambda,
                       (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), round, (uint64_t)query_base, z_max, out_dev);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int gl_pbb_group_min(gl_ctx *ctx, const uint8_t *queries_u8_dev, const uint8_t *cand_u8_dev, int64_t nq, int64_t lambda, int64_t d, uint64_t *out_S_dev,
                     int32_t *out_j_dev, void *workspace_dev)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx, "gl_pbb_group_min: NULL ctx");
    GL_REQUIRE(nq >= 0 && nq < (1ll << 31) && lambda >= 1 && d > 0 && d <= GL_L2_WIDE_MAX_D, "gl_pbb_group_min: bad sizes nq=%lld lambda=%lld d=%lld (d <= %lld)",
               (long long)nq, (long long)lambda, (long long)d, (long long)GL_L2_WIDE_MAX_D);
    const int64_t groups = gl_ceil_div(lambda, GROUP);
    GL_REQUIRE(groups <= 65535, "gl_pbb_group_min: lambda=%lld exceeds %d candidates per query", (long long)lambda, 65535 * GROUP);
    if (nq == 0) return GL_OK;
    GL_REQUIRE(nq <= INT64_MAX / lambda / d, "gl_pbb_group_min: nq * lambda * d overflows");
    GL_REQUIRE(queries_u8_dev && cand_u8_dev && out_S_dev && out_j_dev && workspace_dev, "gl_pbb_group_min: NULL device pointer");
    GL_REQUIRE((reinterpret_cast<uintptr_t>(out_S_dev) & 7) == 0 && (reinterpret_cast<uintptr_t>(out_j_dev) & 3) == 0 &&
               (reinterpret_cast<uintptr_t>(workspace_dev) & 15) == 0,
               "gl_pbb_group_min: out_S_dev must be 8-byte, out_j_dev 4-byte and the workspace 16-byte aligned");
    const bool vec = (d & 15) == 0 && ((reinterpret_cast<uintptr_t>(queries_u8_dev) | reinterpret_cast<uintptr_t>(cand_u8_dev)) & 15) == 0;
    pbb_partial *part = reinterpret_cast<pbb_partial *>(workspace_dev);
    const dim3 grid((unsigned)nq, (unsigned)groups);
    if (vec)
        hipLaunchKernelGGL((pbb_group_min_kernel<true, false>), grid, dim3(kThreads), 0, ctx->stream, queries_u8_dev, cand_u8_dev, (int)lambda, d, part, nq,
                           (unsigned long long *)nullptr);
    else
        hipLaunchKernelGGL((pbb_group_min_kernel<false, false>), grid, dim3(kThreads), 0, ctx->stream, queries_u8_dev, cand_u8_dev, (int)lambda, d, part, nq,
                           (unsigned long long *)nullptr);
    GL_LAUNCH_CHECK();
    hipLaunchKernelGGL(pbb_combine_kernel, dim3((unsigned)gl_ceil_div(nq, kThreads)), dim3(kThreads), 0, ctx->stream, part, nq, (int)groups,
                       reinterpret_cast<unsigned long long *>(out_S_dev), out_j_dev);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int gl_pbb_group_S(gl_ctx *ctx, const uint8_t *queries_u8_dev, const uint8_t *cand_u8_dev, int64_t nq, int64_t lambda, int64_t d, uint64_t *out_S_dev)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx, "gl_pbb_group_S: NULL ctx");
    GL_REQUIRE(nq >= 0 && nq < (1ll << 31) && lambda >= 1 && d > 0 && d <= GL_L2_WIDE_MAX_D, "gl_pbb_group_S: bad sizes nq=%lld lambda=%lld d=%lld (d <= %lld)",
               (long long)nq, (long long)lambda, (long long)d, (long long)GL_L2_WIDE_MAX_D);
    const int64_t groups = gl_ceil_div(lambda, GROUP);
    GL_REQUIRE(groups <= 65535, "gl_pbb_group_S: lambda=%lld exceeds %d candidates per query", (long long)lambda, 65535 * GROUP);
    if (nq == 0) return GL_OK;
    GL_REQUIRE(nq <= INT64_MAX / lambda / d, "gl_pbb_group_S: nq * lambda * d overflows");
    GL_REQUIRE(queries_u8_dev && cand_u8_dev && out_S_dev, "gl_pbb_group_S: NULL device pointer");
    GL_REQUIRE((reinterpret_cast<uintptr_t>(out_S_dev) & 7) == 0, "gl_pbb_group_S: out_S_dev must be 8-byte aligned");
    const bool vec = (d & 15) == 0 && ((reinterpret_cast<uintptr_t>(queries_u8_dev) | reinterpret_cast<uintptr_t>(cand_u8_dev)) & 15) == 0;
    unsigned long long *out = reinterpret_cast<unsigned long long *>(out_S_dev);
    const dim3 grid((unsigned)nq, (unsigned)groups);
    if (vec)
        hipLaunchKernelGGL((pbb_group_min_kernel<true, true>), grid, dim3(kThreads), 0, ctx->stream, queries_u8_dev, cand_u8_dev, (int)lambda, d,
                           (pbb_partial *)nullptr, nq, out);
    else
        hipLaunchKernelGGL((pbb_group_min_kernel<false, true>), grid, dim3(kThreads), 0, ctx->stream, queries_u8_dev, cand_u8_dev, (int)lambda, d,
                           (pbb_partial *)nullptr, nq, out);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int gl_recon_latents(gl_ctx *ctx, const float *mu_dev, const float *std_dev, int64_t nq, int64_t nz, int64_t lambda, uint64_t seed, int64_t query_base,
                     float z_max, float *out_dev)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx, "gl_recon_latents: NULL ctx");
    GL_REQUIRE(nq >= 0 && nz >= 1 && nz < (1ll << 31) && lambda >= 1 && lambda < (1ll << 31), "gl_recon_latents: bad sizes nq=%lld nz=%lld lambda=%lld",
               (long long)nq, (long long)nz, (long long)lambda);
    GL_REQUIRE(query_base >= 0 && nq <= (1ll << 32) && query_base <= (1ll << 32) - nq,
               "gl_recon_latents: query_base + nq = %lld + %lld exceeds 2^32 (the noise counter holds 32 bits of the query index)", (long long)query_base,
               (long long)nq);
    GL_REQUIRE(finite_f(z_max) && z_max > 0.0f, "gl_recon_latents: z_max must be finite and positive");
    if (nq == 0) return GL_OK;
    GL_REQUIRE(nq <= INT64_MAX / lambda / nz, "gl_recon_latents: nq * lambda * nz overflows");
    GL_REQUIRE(mu_dev && std_dev && out_dev, "gl_recon_latents: NULL device pointer");
    const int64_t total = nq * lambda * nz;
    int64_t blocks = gl_ceil_div(total, kThreads);
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(recon_latents_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, ctx->stream, mu_dev, std_dev, nq, (int)nz, (int)lambda,
                       (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), (uint64_t)query_base, z_max, out_dev);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int gl_pbb_group_min_keys(gl_ctx *ctx, const float *M_dev, int64_t nq, int64_t lambda, int64_t ld, uint64_t *keys_dev, int32_t *j_dev)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx, "gl_pbb_group_min_keys: NULL ctx");
    GL_REQUIRE(nq >= 0 && nq < (1ll << 31) && lambda >= 1 && lambda < (1ll << 31), "gl_pbb_group_min_keys: bad sizes nq=%lld lambda=%lld", (long long)nq,
               (long long)lambda);
    // nq * lambda < 2^62 after the check above; the last element read is M[(nq - 1) * ld + nq * lambda - 1], below nq * ld
    GL_REQUIRE(ld >= nq * lambda && (nq == 0 || ld <= INT64_MAX / 4 / nq), "gl_pbb_group_min_keys: ld=%lld must hold nq * lambda = %lld * %lld columns",
               (long long)ld, (long long)nq, (long long)lambda);
    if (nq == 0) return GL_OK;
    GL_REQUIRE(M_dev && keys_dev && j_dev, "gl_pbb_group_min_keys: NULL device pointer");
    GL_REQUIRE((reinterpret_cast<uintptr_t>(M_dev) & 3) == 0 && (reinterpret_cast<uintptr_t>(keys_dev) & 7) == 0 &&
               (reinterpret_cast<uintptr_t>(j_dev) & 3) == 0, "gl_pbb_group_min_keys: M_dev, j_dev must be 4-byte and keys_dev 8-byte aligned");
    hipLaunchKernelGGL(pbb_group_min_keys_kernel, dim3((unsigned)gl_ceil_div(nq, WAVES)), dim3(kThreads), 0, ctx->stream, M_dev, nq, lambda, ld,
                       reinterpret_cast<unsigned long long *>(keys_dev), j_dev);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int gl_pbb_accept(gl_ctx *ctx, float *z_dev, float *sigma_dev, uint64_t *S_cur_dev, const float *cand_z_dev, const uint64_t *S_new_dev,
                  const int32_t *j_new_dev, int64_t nq, int64_t nz, int64_t lambda, float up, float down, float sigma_min, float sigma_max,
                  uint8_t *accepted_dev)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx, "gl_pbb_accept: NULL ctx");
    GL_REQUIRE(nq >= 0 && nq < (1ll << 31) && nz >= 1 && nz < (1ll << 31) && lambda >= 1 && lambda < (1ll << 31),
               "gl_pbb_accept: bad sizes nq=%lld nz=%lld lambda=%lld", (long long)nq, (long long)nz, (long long)lambda);
    GL_REQUIRE(finite_f(up) && finite_f(down) && up > 0.0f && down > 0.0f, "gl_pbb_accept: up and down must be finite and positive");
    GL_REQUIRE(finite_f(sigma_min) && finite_f(sigma_max) && sigma_min > 0.0f && sigma_min <= sigma_max,
               "gl_pbb_accept: need 0 < sigma_min <= sigma_max, both finite");
    if (nq == 0) return GL_OK;
    GL_REQUIRE(nq <= INT64_MAX / lambda / nz, "gl_pbb_accept: nq * lambda * nz overflows");
    GL_REQUIRE(z_dev && sigma_dev && S_cur_dev && cand_z_dev && S_new_dev && j_new_dev && accepted_dev, "gl_pbb_accept: NULL device pointer");
    GL_REQUIRE(((reinterpret_cast<uintptr_t>(S_cur_dev) | reinterpret_cast<uintptr_t>(S_new_dev)) & 7) == 0 &&
               (reinterpret_cast<uintptr_t>(j_new_dev) & 3) == 0, "gl_pbb_accept: S_cur_dev, S_new_dev must be 8-byte and j_new_dev 4-byte aligned");
    hipLaunchKernelGGL(pbb_accept_kernel, dim3((unsigned)nq), dim3(64), 0, ctx->stream, z_dev, sigma_dev,
                       reinterpret_cast<unsigned long long *>(S_cur_dev), cand_z_dev, reinterpret_cast<const unsigned long long *>(S_new_dev), j_new_dev,
                       (int)nz, (int)lambda, up, down, sigma_min, sigma_max, accepted_dev);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

}  // extern "C"
