// Backward pass of the self-attention block of gl_dcgan.hip (attention_core_kernel), the part of VAEGAN's latent gradient that is not the DCGAN
// ConvTranspose stack.  Per image of T = 256 positions, with the rows [q | k | v] the forward left in ws_qkv (DK = C / 8, C in {64, 128}),
// dY the gradient with respect to y = gamma * out + x, and P = softmax_j(q_i . k_j):
//   dO = gamma dY,  dV_j = sum_i P_ij dO_i,  dP_ij = dO_i . v_j,  D_i = sum_j P_ij dP_ij,  dE_ij = P_ij (dP_ij - D_i),
//   dq_i = sum_j dE_ij k_j,  dk_j = sum_i dE_ij q_i
// and dX = dY + [dq | dk | dv] . [Wq; Wk; Wv] is one GEMM of the caller (gl_dcgan_grad.hip); the biases get no gradient.  The T x T matrices
// are never stored: P is rebuilt from q and k with the forward's own instructions (the same fp32 MFMA chain for the energies, the same
// __expf(e - m) and row sum), so the probabilities differentiated are the ones the forward used.  Two kernels, one workgroup of 8 waves per
// image each, every GEMM on v_mfma_f32_32x32x2_f32 (exact fp32 products, a k-ordered fma chain):
//   rows     wave w owns the 32 query rows i of block w, a lane one i (lane & 31) and -- as in the forward -- the 16 key positions
//            j = 32 jb + 4 fh + 8 g + r of every key block jb that the accumulator layout hands its lane half fh.  v [T][C] and k [T][DK] sit in
//            LDS.  Three sweeps over the key blocks: the row maximum m_i; then l_i and sum_j p_ij dP_ij (D_i needs every j), dP^T = v dO^T; then dP^T
//            again for dE, which is at once the B operand of dq^T += k^T dE^T.  Every sweep forms the energies of its block again (DK / 2 MFMAs
//            against the C / 2 of dP): P and dP do not both fit the register file at C = 128, and keeping the forward's 8 x 16 energies spills at
//            two waves per SIMD.  D_i = dO_i . out_i would need the forward's output, which y = gamma out + x does not give back at gamma = 0.
//            Writes dq, the zero columns of the caller's GEMM and the row statistics (m_i, 1 / l_i, D_i).
//   columns  wave w owns the 32 key rows j of block w, a lane one j, and walks the query blocks ib in ascending order.  dO = gamma dY [T][C] and
//            q [T][DK] sit in LDS with the statistics.  Per block: E = q k^T (the forward's chain with A and B exchanged: the same products in
//            the same order), P from the stored statistics, dP = dO v^T, then dV^T += dO^T P and dk^T += q^T dE with P and dE as B operands straight
//            from the accumulator registers.  Writes dk and dv.
// Every sum is in-wave and in a fixed order (blocks ascending, then the MFMA's k order): no atomics, no split sums, and a row depends on its own
// image alone.  Both LDS images are row-major with a row stride of C + 1 (DK + 1) floats: an A operand is read with the lanes along the rows
// (stride C + 1: 32 banks) or along the columns (consecutive), both without bank conflicts, so one image serves both products that need it.
// LDS at C = 128: 149 504 B (rows) / 152 576 B (columns) of the 163 840 B of a CU, one workgroup per CU, 2 waves per SIMD: up to 256 registers per lane.
#include "gl_dcgan.h"

namespace {

typedef float v16f __attribute__((ext_vector_type(16)));

template <int C>
struct AttGrad {
    static constexpr int T = 256, DK = C / 8, QKV = 2 * DK + C, QKVP = (QKV + 31) / 32 * 32, LD = C + 1, LDK = DK + 1, CB = C / 32;
    static constexpr int lds_rows = (T * LD + T * LDK) * 4;
    static constexpr int lds_cols = (T * LD + T * LDK + 3 * T) * 4;
};

// big [T][C] -> LDS [T][C + 1] (times scale), small [T][DK] -> LDS [T][DK + 1]; rows of `ld_src` floats
template <int C>
__device__ __forceinline__ void stage_rows(const float *__restrict__ big, int64_t ld_big, float scale, const float *__restrict__ small, int64_t ld_small,
                                           float *__restrict__ bs, float *__restrict__ ss)
{
    using G = AttGrad<C>;
    const int tid = threadIdx.x;
    for (int idx = tid; idx < G::T * C / 4; idx += 512) {
        const int j = idx / (C / 4), c4 = idx % (C / 4);
        const float4 t = *reinterpret_cast<const float4 *>(big + (int64_t)j * ld_big + c4 * 4);
        float *dst = bs + j * G::LD + c4 * 4;
        dst[0] = t.x * scale; dst[1] = t.y * scale; dst[2] = t.z * scale; dst[3] = t.w * scale;
    }
    for (int idx = tid; idx < G::T * G::DK; idx += 512) {
        const int j = idx / G::DK, d = idx % G::DK;
        ss[j * G::LDK + d] = small[(int64_t)j * ld_small + d];
    }
}

// the C / 2 values row[2 s + fh] (times scale): what a lane holds of a B operand whose k index is the channel
template <int C>
__device__ __forceinline__ void load_parity(const float *__restrict__ row, int fh, float scale, float (&out)[C / 2])
{
#pragma unroll
    for (int t = 0; t < C / 4; ++t) {
        const float4 v = *reinterpret_cast<const float4 *>(row + 4 * t);
        out[2 * t] = (fh ? v.y : v.x) * scale;
        out[2 * t + 1] = (fh ? v.w : v.z) * scale;
    }
}

template <int C>
__global__ void __launch_bounds__(512) attention_grad_rows_kernel(const float *__restrict__ qkv, const float *__restrict__ dY, float gamma,
                                                                  float *__restrict__ dqkv, float *__restrict__ stats)
{
    using G = AttGrad<C>;
    constexpr int T = G::T, DK = G::DK, QKV = G::QKV, QKVP = G::QKVP, LD = G::LD, LDK = G::LDK;
    extern __shared__ __attribute__((aligned(16))) float ag_smem[];
    float *vs = ag_smem;                  // [T][C + 1]
    float *ks = ag_smem + T * LD;         // [T][DK + 1]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 31, fh = lane >> 5;
    const float *base = qkv + (int64_t)blockIdx.x * T * QKV;
    stage_rows<C>(base + 2 * DK, QKV, 1.0f, base + DK, QKV, vs, ks);
    __syncthreads();

    const int i = wave * 32 + frow;
    const int64_t pos = (int64_t)blockIdx.x * T + i;
    float qreg[DK / 2];
#pragma unroll
    for (int s = 0; s < DK / 2; ++s) qreg[s] = base[(int64_t)i * QKV + 2 * s + fh];
    // energies, transposed, as the forward forms them: e[r] = energy(i, j = jb * 32 + 4 fh + 8 (r >> 2) + (r & 3)).  A block costs DK / 2 MFMAs
    // against the C / 2 of dP, so every sweep forms them again and the 8 x 16 registers of the forward are not kept
    auto energies = [&](int jb) {
        v16f e;
#pragma unroll
        for (int r = 0; r < 16; ++r) e[r] = 0.0f;
#pragma unroll
        for (int s = 0; s < DK / 2; ++s) e = __builtin_amdgcn_mfma_f32_32x32x2f32(ks[(jb * 32 + frow) * LDK + 2 * s + fh], qreg[s], e, 0, 0, 0);
        return e;
    };
    float dO[C / 2];                      // dO[s] = gamma dY[i][2 s + fh]
    load_parity<C>(dY + pos * C, fh, gamma, dO);
    auto dprobs = [&](int jb) {           // dp[r] = dP(i, the same j) = dO_i . v_j
        v16f dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) dp[r] = 0.0f;
#pragma unroll
        for (int s = 0; s < C / 2; ++s) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vs[(jb * 32 + frow) * LD + 2 * s + fh], dO[s], dp, 0, 0, 0);
        return dp;
    };
    float m = -__builtin_inff();
#pragma unroll 1
    for (int jb = 0; jb < T / 32; ++jb) {
        const v16f e = energies(jb);
#pragma unroll
        for (int r = 0; r < 16; ++r) m = fmaxf(m, e[r]);
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    // first sweep: l_i = sum_j p_ij (the forward's order of additions) and sum_j p_ij dP_ij, p = exp(e - m) the unnormalised weights
    float ssum = 0.0f, dsum = 0.0f;
#pragma unroll 1
    for (int jb = 0; jb < T / 32; ++jb) {
        const v16f e = energies(jb), dp = dprobs(jb);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = __expf(e[r] - m);
            ssum += p;
            dsum = fmaf(p, dp[r], dsum);
        }
    }
    ssum += __shfl_xor(ssum, 32, 64);
    dsum += __shfl_xor(dsum, 32, 64);
    const float inv = 1.0f / ssum;
    const float D = dsum * inv;
    // second sweep: dE_ij = P_ij (dP_ij - D_i), dq^T[d][i] += k[j][d] dE_ij (rows d >= DK of the 32 x 32 tile are fed zeros)
    v16f dq;
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[r] = 0.0f;
    const int kcol = frow < DK ? frow : 0;
#pragma unroll 1
    for (int jb = 0; jb < T / 32; ++jb) {
        const v16f e = energies(jb), dp = dprobs(jb);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float de = (__expf(e[r] - m) * inv) * (dp[r] - D);
            const float kv = ks[(jb * 32 + 4 * fh + 8 * (r >> 2) + (r & 3)) * LDK + kcol];
            dq = __builtin_amdgcn_mfma_f32_32x32x2f32(frow < DK ? kv : 0.0f, de, dq, 0, 0, 0);
        }
    }
    // dq[r] = dq^T[d = 4 fh + 8 (r >> 2) + (r & 3)][i]
    float *drow = dqkv + pos * QKVP;
#pragma unroll
    for (int g = 0; g < DK / 8; ++g)
        *reinterpret_cast<float4 *>(drow + 8 * g + 4 * fh) = make_float4(dq[4 * g], dq[4 * g + 1], dq[4 * g + 2], dq[4 * g + 3]);
    for (int c = QKV + 4 * fh; c < QKVP; c += 8) *reinterpret_cast<float4 *>(drow + c) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // the GEMM's zero columns
    if (fh == 0) {
        float *st = stats + (int64_t)blockIdx.x * 3 * T;
        st[i] = m;
        st[T + i] = inv;
        st[2 * T + i] = D;
    }
}

template <int C>
__global__ void __launch_bounds__(512) attention_grad_cols_kernel(const float *__restrict__ qkv, const float *__restrict__ dY, float gamma,
                                                                  const float *__restrict__ stats, float *__restrict__ dqkv)
{
    using G = AttGrad<C>;
    constexpr int T = G::T, DK = G::DK, QKV = G::QKV, QKVP = G::QKVP, LD = G::LD, LDK = G::LDK, CB = G::CB;
    extern __shared__ __attribute__((aligned(16))) float ag_smem[];
    float *dOs = ag_smem;                 // [T][C + 1], gamma dY
    float *qs = ag_smem + T * LD;         // [T][DK + 1]
    float *st = qs + T * LDK;             // [3][T]: m, 1 / l, D
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 31, fh = lane >> 5;
    const float *base = qkv + (int64_t)blockIdx.x * T * QKV;
    stage_rows<C>(dY + (int64_t)blockIdx.x * T * C, C, gamma, base, QKV, dOs, qs);
    for (int idx = tid; idx < 3 * T; idx += 512) st[idx] = stats[(int64_t)blockIdx.x * 3 * T + idx];
    __syncthreads();

    const int j = wave * 32 + frow;
    float kreg[DK / 2], vreg[C / 2];
#pragma unroll
    for (int s = 0; s < DK / 2; ++s) kreg[s] = base[(int64_t)j * QKV + DK + 2 * s + fh];
    load_parity<C>(base + (int64_t)j * QKV + 2 * DK, fh, 1.0f, vreg);
    v16f dv[CB], dk;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        dk[r] = 0.0f;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) dv[cb][r] = 0.0f;
    }
    const int qcol = frow < DK ? frow : 0;
#pragma unroll 1
    for (int ib = 0; ib < T / 32; ++ib) {
        // e[r] = energy(i = ib * 32 + 4 fh + 8 (r >> 2) + (r & 3), j), dp[r] = dP of the same pair
        v16f e, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { e[r] = 0.0f; dp[r] = 0.0f; }
#pragma unroll
        for (int s = 0; s < DK / 2; ++s) e = __builtin_amdgcn_mfma_f32_32x32x2f32(qs[(ib * 32 + frow) * LDK + 2 * s + fh], kreg[s], e, 0, 0, 0);
#pragma unroll
        for (int s = 0; s < C / 2; ++s) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(dOs[(ib * 32 + frow) * LD + 2 * s + fh], vreg[s], dp, 0, 0, 0);
        float p[16], de[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int i4 = ib * 32 + 8 * g + 4 * fh;
            const float4 mm = *reinterpret_cast<const float4 *>(st + i4), il = *reinterpret_cast<const float4 *>(st + T + i4),
                         dd = *reinterpret_cast<const float4 *>(st + 2 * T + i4);
            const float mr[4] = {mm.x, mm.y, mm.z, mm.w}, ir[4] = {il.x, il.y, il.z, il.w}, dr[4] = {dd.x, dd.y, dd.z, dd.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                p[4 * g + r] = __expf(e[4 * g + r] - mr[r]) * ir[r];
                de[4 * g + r] = p[4 * g + r] * (dp[4 * g + r] - dr[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int irow = ib * 32 + 4 * fh + 8 * (r >> 2) + (r & 3);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) dv[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(dOs[irow * LD + cb * 32 + frow], p[r], dv[cb], 0, 0, 0);
            const float qv = qs[irow * LDK + qcol];
            dk = __builtin_amdgcn_mfma_f32_32x32x2f32(frow < DK ? qv : 0.0f, de[r], dk, 0, 0, 0);
        }
    }
    // dk[r] = dk^T[d = 4 fh + 8 (r >> 2) + (r & 3)][j], dv[cb][r] = dV^T[c = cb * 32 + the same][j]
    float *drow = dqkv + ((int64_t)blockIdx.x * T + j) * QKVP;
#pragma unroll
    for (int g = 0; g < DK / 8; ++g)
        *reinterpret_cast<float4 *>(drow + DK + 8 * g + 4 * fh) = make_float4(dk[4 * g], dk[4 * g + 1], dk[4 * g + 2], dk[4 * g + 3]);
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4 *>(drow + 2 * DK + cb * 32 + 8 * g + 4 * fh) =
                make_float4(dv[cb][4 * g], dv[cb][4 * g + 1], dv[cb][4 * g + 2], dv[cb][4 * g + 3]);
}

template <int C>
int launch_attention_grad(gl_ctx *ctx, const float *qkv, const float *dY, float gamma, int64_t images, float *dqkv, float *stats)
{
    using G = AttGrad<C>;
    GL_ONCE_PER_DEVICE(ctx, \
        GL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(attention_grad_rows_kernel<C>), hipFuncAttributeMaxDynamicSharedMemorySize, G::lds_rows)); \
        GL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(attention_grad_cols_kernel<C>), hipFuncAttributeMaxDynamicSharedMemorySize, G::lds_cols)););
    hipLaunchKernelGGL((attention_grad_rows_kernel<C>), dim3((unsigned)images), dim3(512), G::lds_rows, ctx->stream, qkv, dY, gamma, dqkv, stats);
    GL_LAUNCH_CHECK();
    hipLaunchKernelGGL((attention_grad_cols_kernel<C>), dim3((unsigned)images), dim3(512), G::lds_cols, ctx->stream, qkv, dY, gamma,
                       (const float *)stats, dqkv);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

}  // namespace

int gl_attention_grad_cols(int C) { return C == 128 ? AttGrad<128>::QKVP : AttGrad<64>::QKVP; }

int gl_launch_attention_grad(gl_ctx *ctx, int C, const float *qkv, const float *dY, float gamma, int64_t images, float *dqkv, float *stats)
{
    GL_REQUIRE(C == 64 || C == 128, "attention backward: width %d unsupported (64 or 128)", C);
    GL_REQUIRE(qkv && dY && dqkv && stats && images >= 0 && images < (1ll << 31), "attention backward: bad argument");
    GL_REQUIRE(((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(dY) | reinterpret_cast<uintptr_t>(dqkv)) & 15) == 0,
               "attention backward: unaligned operand");
    if (images == 0) return GL_OK;
    return C == 128 ? launch_attention_grad<128>(ctx, qkv, dY, gamma, images, dqkv, stats) : launch_attention_grad<64>(ctx, qkv, dY, gamma, images, dqkv, stats);
}
