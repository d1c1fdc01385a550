// The kernel-density (soft-min) epilogue of the exact-integer pair kernels (gl_kde.hip): sums[q][t] += sum over bank rows of
// kde_weight(S(q, n) - S0[q], coef[t]), a fixed-point stand-in for 2^(-(S - S0) coef) in units of 2^-40.
//
// The first part of this header is the arithmetic contract and compiles for the host as well (tests/test_kde_cpu.py builds it with a plain
// C++ compiler; define GL_KDE_HOST_ONLY to leave the device epilogues out): gl_kde_weight and gl_kde_cut for the exact-integer path,
// gl_kde_weight_f32 and gl_kde_cut_bits for the float paths (0.2 LPIPS + L2 and fp32 rows), both on gl_kde_weight_x.  Every float operation in it is
// one individually rounded fp32 multiply or add -- no fma contraction, no exponential instruction, no ldexp -- so that host and device
// agree bit for bit and the integer sums are a function of the multiset of pair distances alone.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define GL_KDE_FN __host__ __device__ __forceinline__
#else
#define GL_KDE_FN inline
#endif
// One rounded product / sum, MATERIALISED: without it the compiler is free to fuse the product into the add that follows it (fma
// contraction, which __fmul_rn / __fadd_rn do not prevent: they are plain operators), and device and host would stop agreeing bit for bit.
// On the device the empty asm pins the value in a register (the idiom of gl_tap_value); on the host a volatile store does the same.
GL_KDE_FN float gl_kde_mul(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    float r = a * b;
    asm volatile("" : "+v"(r));
    return r;
#else
    volatile float r = a * b;
    return r;
#endif
}
GL_KDE_FN float gl_kde_add(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    float r = a + b;
    asm volatile("" : "+v"(r));
    return r;
#else
    volatile float r = a + b;
    return r;
#endif
}

// weights are in units of 2^-GL_KDE_FRAC_BITS: gl_kde_weight(0, c) == 2^40, and nothing is larger
#define GL_KDE_FRAC_BITS 40
// x = fl32(fl32(delta) * c) at or beyond this gives the weight 0 (2^-41 is below half a unit)
#define GL_KDE_X_CUT 41.0f

// 2^-f on [0, 1) = 1 + f q(f): q interpolates (2^-f - 1) / f at six Chebyshev nodes.  Evaluated by Horner with every product and sum rounded
// to fp32 the relative error of p is 1.9e-7 (measured on 2 x 10^6 points); q < 0 on [0, 1), so p <= 1, and p >= 0.5.
#define GL_KDE_C1 (-0x1.62e430p-1f)
#define GL_KDE_C2 (0x1.ebfba8p-3f)
#define GL_KDE_C3 (-0x1.c6a652p-5f)
#define GL_KDE_C4 (0x1.3a79c4p-7f)
#define GL_KDE_C5 (-0x1.529848p-10f)
#define GL_KDE_C6 (0x1.e2025cp-14f)

// The weight at x >= 0 (or NaN): trunc(p(f) 2^(40 - n)) with n = floor(x), f = x - n (exact); 0 when x is not below 41, NaN included.
GL_KDE_FN unsigned long long gl_kde_weight_x(float x)
{
    if (!(x < GL_KDE_X_CUT)) return 0ull;
    const int n = (int)x;                                 // 0 <= x < 41: truncation is floor
    const float f = gl_kde_add(x, -(float)n);             // exact: both lie in [n, n + 1)
    float q = GL_KDE_C6;
    q = gl_kde_add(gl_kde_mul(q, f), GL_KDE_C5);
    q = gl_kde_add(gl_kde_mul(q, f), GL_KDE_C4);
    q = gl_kde_add(gl_kde_mul(q, f), GL_KDE_C3);
    q = gl_kde_add(gl_kde_mul(q, f), GL_KDE_C2);
    q = gl_kde_add(gl_kde_mul(q, f), GL_KDE_C1);
    const float p = gl_kde_add(1.0f, gl_kde_mul(q, f));   // in [0.5, 1]
    // p = m 2^(e - 150) with the 24-bit significand m and the biased exponent e: p 2^(40 - n) = m 2^(e - 110 - n), truncated by the shift
    unsigned bits;
    memcpy(&bits, &p, 4);
    const unsigned long long m = (unsigned long long)((bits & 0x7FFFFFu) | 0x800000u);
    const int sh = (int)(bits >> 23) - 110 - n;           // e is 126 or 127: -24 <= sh <= 17
    return sh >= 0 ? m << sh : m >> (-sh);
}

// The weight of a pair at delta = S - S0 >= 0 under the coefficient c (finite, >= 0): gl_kde_weight_x of x = fl32(fl32(delta) c).
// delta < 0 is the caller's error (the weight would exceed 2^40); the kernels raise a flag instead of calling this.
GL_KDE_FN unsigned long long gl_kde_weight(long long delta, float c)
{
    return gl_kde_weight_x(gl_kde_mul((float)delta, c));  // int64 -> fp32 rounds to nearest even on host and device
}

// The weight of a pair on the float paths (0.2 LPIPS + L2, fp32 rows): D its float32 distance, D0 the float32 distance of its query's
// nearest sample, c the coefficient: gl_kde_weight_x of x = fl32(fl32(D - D0) c) -- one rounded subtraction and one rounded product, each
// materialised, no fma.  Preconditions: D >= D0 >= 0, D0 finite, D not NaN, c finite and >= 0; D < D0 and NaN are the caller's errors (the
// kernels raise flag bits instead of calling this).  D = +inf gives x = inf (NaN for c = 0), hence the weight 0 by the first test of
// gl_kde_weight_x: a row at infinite distance weighs nothing, under c = 0 as well.
// Measured on 1.1 x 10^6 (D, D0, c) triples (tests/test_pair_kde_cpu.py) against float64 2^(-(D - D0) c): the largest relative error where
// the true weight is >= 2^-30 is 9.71e-4 (the truncation to units of 2^-40: 2^-10 at a weight of 2^-30, as for gl_kde_weight); for x <= 8
// it is 5.3e-7: the fp32 rounding of D - D0 and of the product (2 x 8 x 2^-24 ln 2 at most) plus the polynomial's.
GL_KDE_FN unsigned long long gl_kde_weight_f32(float D, float D0, float c)
{
    return gl_kde_weight_x(gl_kde_mul(gl_kde_add(D, -D0), c));
}

// The smallest delta from which on every weight under c is 0, or 2^62 when there is none below that (no S reaches it: S < 2^40).  The
// kernels test each pair once against S0 + gl_kde_cut(smallest coefficient) before anything else.  It never excludes a pair whose weight
// is not 0: fl32(delta) is non-decreasing in delta (round to nearest is monotone), and so is its rounded product with c >= 0, so
// x(delta) >= x(cut) >= 41 for every delta >= cut, where gl_kde_weight returns 0 by its first test.  Host only.
#if defined(__HIPCC__)
__host__
#endif
inline long long gl_kde_cut(float c)
{
    long long lo = 0, hi = 1ll << 62;                     // x(lo) = 0 < 41
    if (gl_kde_mul((float)hi, c) < GL_KDE_X_CUT) return hi;
    while (hi - lo > 1) {
        const long long mid = lo + (hi - lo) / 2;
        if (gl_kde_mul((float)mid, c) < GL_KDE_X_CUT) lo = mid;
        else hi = mid;
    }
    return hi;
}

// The float sibling of gl_kde_cut: the smallest uint32 pattern b in [bits(D0), 0x7F800000] for which x(b) = fl32(fl32(float(b) - D0) c) is
// not below 41, so that gl_kde_weight_f32 gives 0.  It always exists: x(+inf) is inf, or NaN for c = 0.  The kernels test each pair's
// pattern once against the bound of its query under the SMALLEST coefficient before anything else.  It never excludes a pair whose weight
// is not 0: on D >= D0 >= +0 the order of the patterns is the order of the floats, a rounded subtraction of the fixed D0 is non-decreasing
// in D (round to nearest is monotone) and so is the rounded product of a value >= 0 with c >= 0, with one exception that only helps:
// for c = 0 the product is 0 at every finite D and NaN at +inf, where the weight is 0.  So "!(x(b) < 41)" is monotone in b, the bisection
// below finds its first pattern, and every pair at or above it has the weight 0 under the smallest coefficient -- hence under every larger
// one (x grows with c).  D0 finite and >= 0, c finite and >= 0.  Host only.
#if defined(__HIPCC__)
__host__
#endif
inline uint32_t gl_kde_cut_bits(float D0, float c)
{
    auto beyond = [&](uint32_t b) {
        float D;
        memcpy(&D, &b, 4);
        return !(gl_kde_mul(gl_kde_add(D, -D0), c) < GL_KDE_X_CUT);
    };
    uint32_t lo, hi = 0x7F800000u;                        // beyond(hi) holds
    memcpy(&lo, &D0, 4);
    if (lo >= hi || beyond(lo)) return lo < hi ? lo : hi; // (x(bits(D0)) = 0: only a D0 outside the preconditions comes here)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (beyond(mid)) hi = mid;
        else lo = mid;
    }
    return hi;
}

#if defined(__HIPCC__) && !defined(GL_KDE_HOST_ONLY)
#include "gl_count_epi.h"

namespace gl_kde {

using gl_count::rows_left;

// one launch: S0 per query in device memory, the coefficients descending (coef[n - 1] the smallest), cut = gl_kde_cut(coef[n - 1]),
// s_max = 65025 d (the largest S), flag: a device int that is set when a pair lies below its query's S0
struct kde_args {
    const long long *s0;
    float coef[GL_COUNT_MAX_T];
    long long cut, s_max;
    int *flag;
    int n;
};

// "S - S0 < cut" as "S < bound" in the unsigned type of S: bound = clamp(S0 + cut, 0, s_max + 1) (s_max + 1 fits, see gl_count::rows_bound)
template <typename ST> __device__ __forceinline__ ST kde_bound(long long s0, long long cut, long long s_max)
{
    const long long b = s0 + cut;                         // |S0| < 2^62 is checked by nobody: S0 is an S, below 2^40
    return (ST)(b < 0 ? 0ll : (b > s_max + 1 ? s_max + 1 : b));
}

constexpr int KDE_S0_OFFSET = 256 * GL_COUNT_MAX_T * 8;        // S0 and the bounds follow the largest table of sums (256 queries x 16 x 8 bytes)
constexpr int KDE_LDS_BYTES = KDE_S0_OFFSET + 2 * 256 * 8;     // what the epilogue needs of the slice buffers

// The shape of gl_count::count_epilogue with thresholds per query (same arguments, same steps):
//   1. one compare per pair against the bound of its query's LARGEST ball, S0 + cut (four bounds per lane, read from global memory once the
//      accumulators hold S); workgroups (__syncthreads_or) and waves (__any) without a pair inside leave.
//   2. the others stage S0 and the bound of the tile's queries into the slice buffers; per coefficient t and query column j a lane sums the
//      weights of its pairs inside the bound, the four lane groups of a column are folded with __shfl_xor and group 0 adds the wave's sum
//      into a 64-bit LDS table [queries of the tile][n] (a tile's entry reaches 256 x 2^40).
//   3. the workgroup adds one value per non-zero entry to sums[q][t] (64-bit atomicAdd).
// A pair below S0 sets *a.flag (its weight would exceed 2^40); the sums of such a launch are unspecified.
// smem must hold KDE_LDS_BYTES and be free after the first barrier; every thread of the workgroup must call this.
template <int NI, typename ST, typename SOf>
__device__ __forceinline__ void kde_epilogue(SOf s_of, int n_left, int64_t q0, int qcol0, int q_left, int tile_q, const kde_args &a,
                                             unsigned long long *__restrict__ sums, char *smem, int lane)
{
    const int frow = lane & 15, fk = lane >> 4;
    unsigned rvalid = 0;                                  // bit i * 4 + r: the bank row is a real one
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) rvalid |= (i * 16 + r < n_left ? 1u : 0u) << (i * 4 + r);
    const long long *s0_tile = a.s0 + q0;
    int hit = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ql = qcol0 + j * 16 + frow;
        const ST top = ql < q_left ? kde_bound<ST>(s0_tile[ql], a.cut, a.s_max) : (ST)0;
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) hit |= (((rvalid >> (i * 4 + r)) & 1u) && s_of(i, j, r) < top) ? 1 : 0;
    }
    // (also the barrier after which the slice buffers may be overwritten)
    if (!__syncthreads_or(hit)) return;

    unsigned long long *tab = reinterpret_cast<unsigned long long *>(smem);          // [tile_q][a.n]
    long long *s0_lds = reinterpret_cast<long long *>(smem + KDE_S0_OFFSET);         // [tile_q]
    unsigned long long *bound = reinterpret_cast<unsigned long long *>(smem + KDE_S0_OFFSET + 256 * 8);   // [tile_q]
    const int entries = tile_q * a.n;
    for (int e = threadIdx.x; e < entries; e += blockDim.x) tab[e] = 0ull;
    for (int ql = threadIdx.x; ql < tile_q; ql += blockDim.x) {
        const long long s0 = ql < q_left ? s0_tile[ql] : 0ll;
        s0_lds[ql] = s0;
        bound[ql] = ql < q_left ? (unsigned long long)kde_bound<ST>(s0, a.cut, a.s_max) : 0ull;     // queries beyond nq: nothing is inside
    }
    __syncthreads();
    if (__any(hit)) {
        int below = 0;
        for (int t = 0; t < a.n; ++t) {
            const float c = a.coef[t];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ql = qcol0 + j * 16 + frow;
                const long long s0 = s0_lds[ql];
                const ST top = (ST)bound[ql];
                unsigned long long w = 0ull;
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const ST s = s_of(i, j, r);
                        if (((rvalid >> (i * 4 + r)) & 1u) && s < top) {
                            const long long delta = (long long)s - s0;
                            if (delta < 0) below = 1;
                            else w += gl_kde_weight(delta, c);
                        }
                    }
                w += __shfl_xor(w, 16, 64);
                w += __shfl_xor(w, 32, 64);
                if (fk == 0 && w != 0ull) atomicAdd(&tab[ql * a.n + t], w);
            }
        }
        if (below) *a.flag = 1;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < entries; e += blockDim.x) {
        const unsigned long long w = tab[e];
        if (w != 0ull) atomicAdd(&sums[q0 * a.n + e], w);
    }
}

// ---- the float paths: the pairs carry the uint32 pattern of their float32 distance D32 >= +0 (gl_feat_count.hip; gl_l2f32.hip has the same
// steps in its own thread layout)

// ctx->kde_flag as bits
constexpr int KDE_FLAG_BELOW = 1;            // a real pair has bits(D32) < bits(D0): its weight would exceed 2^40
constexpr int KDE_FLAG_NAN = 2;              // a real pair's D32 is NaN (pattern above 0x7F800000); only fp32 rows can produce one

// one launch: D0 per query (float32, the distance of its nearest sample) and bound per query (gl_kde_cut_bits(D0, coef[n - 1])) in device
// memory, the coefficients descending, flag: a device int that takes the bits above
struct kde_f32_args {
    const float *d0;
    const unsigned *bound;
    float coef[GL_COUNT_MAX_T];
    int *flag;
    int n;
};

constexpr int KDE_F32_LDS_BYTES = KDE_S0_OFFSET + 2 * 256 * 4;     // the table of sums, then D0 and the bounds of the tile's queries

// kde_epilogue on patterns: s_of gives bits(D32), a pair takes part when its pattern lies below its query's bound (one compare; the bound
// is at most 0x7F800000, so +inf and NaN patterns never do), its weight is gl_kde_weight_f32(D32, D0, coef[t]).  Same three steps, same
// LDS table, same atomics.  A pair below D0 sets KDE_FLAG_BELOW in *a.flag; the sums of such a launch are unspecified.
// smem must hold KDE_F32_LDS_BYTES and be free after the first barrier; every thread of the workgroup must call this.
template <int NI, typename SOf>
__device__ __forceinline__ void kde_epilogue_f32(SOf s_of, int n_left, int64_t q0, int qcol0, int q_left, int tile_q, const kde_f32_args &a,
                                                 unsigned long long *__restrict__ sums, char *smem, int lane)
{
    const int frow = lane & 15, fk = lane >> 4;
    unsigned rvalid = 0;                                  // bit i * 4 + r: the bank row is a real one
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) rvalid |= (i * 16 + r < n_left ? 1u : 0u) << (i * 4 + r);
    const unsigned *bound_tile = a.bound + q0;
    int hit = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ql = qcol0 + j * 16 + frow;
        const unsigned top = ql < q_left ? bound_tile[ql] : 0u;
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) hit |= (((rvalid >> (i * 4 + r)) & 1u) && s_of(i, j, r) < top) ? 1 : 0;
    }
    // (also the barrier after which the slice buffers may be overwritten)
    if (!__syncthreads_or(hit)) return;

    unsigned long long *tab = reinterpret_cast<unsigned long long *>(smem);          // [tile_q][a.n]
    float *d0_lds = reinterpret_cast<float *>(smem + KDE_S0_OFFSET);                 // [tile_q]
    unsigned *bound = reinterpret_cast<unsigned *>(smem + KDE_S0_OFFSET + 256 * 4);  // [tile_q]
    const int entries = tile_q * a.n;
    for (int e = threadIdx.x; e < entries; e += blockDim.x) tab[e] = 0ull;
    for (int ql = threadIdx.x; ql < tile_q; ql += blockDim.x) {
        d0_lds[ql] = ql < q_left ? a.d0[q0 + ql] : 0.0f;
        bound[ql] = ql < q_left ? bound_tile[ql] : 0u;    // queries beyond nq: nothing is inside
    }
    __syncthreads();
    if (__any(hit)) {
        int below = 0;
        for (int t = 0; t < a.n; ++t) {
            const float c = a.coef[t];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ql = qcol0 + j * 16 + frow;
                const float d0 = d0_lds[ql];
                const unsigned top = bound[ql];
                unsigned long long w = 0ull;
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const unsigned s = s_of(i, j, r);
                        if (((rvalid >> (i * 4 + r)) & 1u) && s < top) {
                            if (s < __float_as_uint(d0)) below = 1;
                            else w += gl_kde_weight_f32(__uint_as_float(s), d0, c);
                        }
                    }
                w += __shfl_xor(w, 16, 64);
                w += __shfl_xor(w, 32, 64);
                if (fk == 0 && w != 0ull) atomicAdd(&tab[ql * a.n + t], w);
            }
        }
        if (below) atomicOr(a.flag, KDE_FLAG_BELOW);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < entries; e += blockDim.x) {
        const unsigned long long w = tab[e];
        if (w != 0ull) atomicAdd(&sums[q0 * a.n + e], w);
    }
}

}  // namespace gl_kde

// What the launchers of the float paths do behind their kernel, as gl_kde.hip's kde_rows_impl does: the flag is read back and cleared (so
// the call waits for its kernel, and the next call on the context starts clean) and a set bit fails the call.
inline int gl_kde_flag_check(const char *fn, gl_ctx *ctx)
{
    int flag = 0;
    GL_HIP(hipMemcpyAsync(&flag, ctx->kde_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    GL_HIP(hipMemsetAsync(ctx->kde_flag, 0, sizeof(int), ctx->stream));
    GL_HIP(hipStreamSynchronize(ctx->stream));
    GL_REQUIRE(!(flag & gl_kde::KDE_FLAG_NAN), "%s: the distance of a pair is NaN (rows with NaN, or with +inf and -inf, or differences that overflow to "
               "inf - inf); the sums of this call are unspecified", fn);
    GL_REQUIRE(!(flag & gl_kde::KDE_FLAG_BELOW), "%s: a pair lies below the offset D0 of its query (its weight would exceed 2^40); the sums of this call "
               "are unspecified", fn);
    return GL_OK;
}
#endif
