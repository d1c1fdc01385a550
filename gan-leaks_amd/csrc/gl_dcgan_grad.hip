// Gradient of the DCGAN / WGAN-GP generator with respect to its latent input: grad_z = (dG/dz)^T cot, the white-box attack's hot path.
//
// A pass of m images first runs the forward with fp32 products (gl_dcgan_forward, precision 0), which leaves the post-ReLU activations
// a_0..a_3 (NHWC) in g->ws_a and the output y.  Backwards, with BatchNorm an eval-mode affine of scale s_l[c]:
//   g4                = cot * (1 - y^2)                                                                  (tanh')
//   dA_3[n,y,x,ci]    = sum_{ky,kx,co} g4[n,co,2y+ky-1,2x+kx-1] W4[ci,co,ky,kx]       the data gradient of ConvTranspose2d(k4 s2 p1) is Conv2d(k4 s2 p1)
//   gpre_l            = dA_l * [a_l > 0] * s_l[c],   dA_{l-1} = the same stride-2 convolution of gpre_l with W_l          (l = 3, 2, 1)
//   dz[n,ci]          = sum_{ky,kx,co} gpre_0[n,ky,kx,co] W0[ci,co,ky,kx]
// Everything that multiplies weights runs on the forward's fp32 tap-gather GEMM (gl_launch_gather_conv), untouched:
//   * ky - 1 = 2 dy + py, i.e. ky = 0,1,2,3 -> (dy,py) = (-1,1), (0,0), (0,1), (1,0).  relu_bn_grad_kernel stores gpre_l phase-planar,
//     [py*2+px][n][H][W][C] (space-to-depth of the 2H x 2W grid), so that per input phase the stride-2 convolution is a stride-1 gather with
//     2 x 2 taps, offsets in {-1,0,1}, Cin = C_l and C_{l-1} columns.  The four phases are four launches; phases 1..3 add the running sum
//     through GlGatherConv::residual (in place: a thread reads the element it then writes), so every output is ((p0 + p1) + p2) + p3 with
//     each p a fixed-order GEMM row: no atomics, no split K, and a row does not depend on which images share the launch.
//   * the 3-channel layer: patch_rgb_kernel gathers the 4 x 4 x 3 window of g4 behind every 32 x 32 position into [pos][48 -> 64] rows
//     (the mirror of col2im_rgb_tanh_kernel), then a one-tap GEMM with K = 64 gives the C_3 columns.
//   * layer 0 is a plain GEMM [m][16 C1] x [16 C1][z_dim] written straight into grad_z (rows of z_dim, no padding), its K in chunks of 4096.
//   * VAEGAN's stack with its spectral-norm state held: s_l = bn_scale / sigma is what g->scale[l] holds, and layer 3 reads y = gamma out + x of the
//     self-attention block, so its data gradient is dY.  gl_attention_grad.hip turns dY and the forward's rows [q | k | v] into rows
//     [dq | dk | dv | 0], and one one-tap GEMM with the transposed 1x1 weights adds them to dY in place (residual): dX = dA_2.
// The FLOP count equals the forward's.  Transposed weight packs and workspaces are built on the first gradient call only.
#include "gl_dcgan.h"
#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int IMG = 3 * 64 * 64;
constexpr int kGradK0 = 4096;   // K chunk of the last GEMM; 16 C1 = 256 features_g is a multiple of it (features_g % 16 == 0)

// ky -> (dy, py) with ky - 1 = 2 dy + py; per input phase py the two taps ty = 0, 1
const int kBwdKy[2][2] = {{1, 3}, {0, 2}};
const int kBwdDy[2][2] = {{0, 1}, {-1, 0}};

// one workgroup per image.  L2: cot = 2 (y - x), x = 2 u / 255 - 1 the target's value, and loss = sum (y - x)^2 -- the squares are added in
// double, per thread over its strided share and then down a fixed tree, so the float result is that of the exact sum of the fp32 differences.
template <bool L2>
__global__ void __launch_bounds__(kThreads) tanh_grad_kernel(const float *__restrict__ y, const float *__restrict__ cot, const uint8_t *__restrict__ target,
                                                             float *__restrict__ g4, float *__restrict__ loss)
{
    __shared__ double red[kThreads];
    const int64_t base = (int64_t)blockIdx.x * IMG;
    double acc = 0.0;
    for (int i = threadIdx.x * 4; i < IMG; i += kThreads * 4) {
        const float4 yv = *reinterpret_cast<const float4 *>(y + base + i);
        float c[4];
        const float yy[4] = {yv.x, yv.y, yv.z, yv.w};
        if constexpr (L2) {
            const uchar4 t = *reinterpret_cast<const uchar4 *>(target + base + i);
            const float u[4] = {(float)t.x, (float)t.y, (float)t.z, (float)t.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float diff = yy[e] - (2.0f * (u[e] / 255.0f) - 1.0f);
                acc += (double)diff * (double)diff;
                c[e] = 2.0f * diff;
            }
        } else {
            const float4 cv = *reinterpret_cast<const float4 *>(cot + base + i);
            c[0] = cv.x; c[1] = cv.y; c[2] = cv.z; c[3] = cv.w;
        }
        float4 o;
        o.x = c[0] * (1.0f - yy[0] * yy[0]);
        o.y = c[1] * (1.0f - yy[1] * yy[1]);
        o.z = c[2] * (1.0f - yy[2] * yy[2]);
        o.w = c[3] * (1.0f - yy[3] * yy[3]);
        *reinterpret_cast<float4 *>(g4 + base + i) = o;
    }
    if constexpr (L2) {
        red[threadIdx.x] = acc;
        __syncthreads();
        for (int o = kThreads / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) loss[blockIdx.x] = (float)red[0];
    }
}

// patch[pos][(ky*4+kx)*3 + co] = g4[n][co][2y+ky-1][2x+kx-1] (0 outside the image; columns 48..63 are 0), pos = (n, y, x) on the 32 x 32 grid.
// One thread per four columns.
__global__ void __launch_bounds__(kThreads) patch_rgb_kernel(const float *__restrict__ g4, int64_t n_img, float *__restrict__ patch)
{
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n_img * 1024 * 16) return;
    const int k4 = (int)(gid & 15);
    const int64_t pos = gid >> 4;
    const int64_t img = pos >> 10;
    const int y = (int)(pos >> 5) & 31, x = (int)pos & 31;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int k = k4 * 4 + e;
        const int t = k / 3, co = k - t * 3;
        const int yy = 2 * y + (t >> 2) - 1, xx = 2 * x + (t & 3) - 1;
        v[e] = 0.0f;
        if (k < 48 && yy >= 0 && yy < 64 && xx >= 0 && xx < 64) v[e] = g4[((img * 3 + co) * 64 + yy) * 64 + xx];
    }
    *reinterpret_cast<float4 *>(patch + gid * 4) = make_float4(v[0], v[1], v[2], v[3]);
}

// gpre = dA * [a > 0] * scale[c] for a pass of n_img images of Ho x Wo x C (NHWC), one thread per four channels.
// PLANAR: stored as [py*2+px][n][Ho/2][Wo/2][C]; otherwise (layer 0: the rows [n][Ho * Wo * C] of the final GEMM) cut into K chunks of kc
// floats, [chunk][n][kc].
template <bool PLANAR>
__global__ void __launch_bounds__(kThreads) relu_bn_grad_kernel(const float *__restrict__ dA, const float *__restrict__ a, const float *__restrict__ scale,
                                                                int64_t n_img, int Ho, int Wo, int C, int kc, float *__restrict__ out)
{
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int c4n = C >> 2;
    const int64_t total = n_img * Ho * Wo * c4n;
    if (gid >= total) return;
    const int c = (int)(gid % c4n) * 4;
    const int64_t pix = gid / c4n;
    const float4 d = *reinterpret_cast<const float4 *>(dA + gid * 4);
    const float4 av = *reinterpret_cast<const float4 *>(a + gid * 4);
    const float4 s = *reinterpret_cast<const float4 *>(scale + c);
    float4 o;
    o.x = av.x > 0.0f ? d.x * s.x : 0.0f;
    o.y = av.y > 0.0f ? d.y * s.y : 0.0f;
    o.z = av.z > 0.0f ? d.z * s.z : 0.0f;
    o.w = av.w > 0.0f ? d.w * s.w : 0.0f;
    int64_t dst;
    if constexpr (PLANAR) {
        const int xo = (int)(pix % Wo);
        const int64_t r = pix / Wo;
        const int yo = (int)(r % Ho);
        const int64_t img = r / Ho;
        const int H = Ho >> 1, W = Wo >> 1;
        const int ph = (yo & 1) * 2 + (xo & 1);
        dst = ((((int64_t)ph * n_img + img) * H + (yo >> 1)) * W + (xo >> 1)) * C + c;
    } else {
        const int row = Ho * Wo * C;
        const int64_t img = (gid * 4) / row;
        const int k = (int)(gid * 4 - img * row);
        dst = ((int64_t)(k / kc) * n_img + img) * kc + k % kc;
    }
    *reinterpret_cast<float4 *>(out + dst) = o;
}

// One launch of every kernel above, with its grid and its template instance: backward_pass and the tuning build's single-launch hook
// (gl_tune_dcgan_grad_op, at the end of this file) both go through these.
void launch_tanh_grad(hipStream_t st, const float *y, const float *cot, const uint8_t *target, int64_t m, float *g4, float *loss)
{
    if (target)
        hipLaunchKernelGGL(tanh_grad_kernel<true>, dim3((unsigned)m), dim3(kThreads), 0, st, y, (const float *)nullptr, target, g4, loss);
    else
        hipLaunchKernelGGL(tanh_grad_kernel<false>, dim3((unsigned)m), dim3(kThreads), 0, st, y, cot, (const uint8_t *)nullptr, g4, (float *)nullptr);
}

void launch_patch_rgb(hipStream_t st, const float *g4, int64_t m, float *patch)
{
    hipLaunchKernelGGL(patch_rgb_kernel, dim3((unsigned)gl_ceil_div(m * 1024 * 16, kThreads)), dim3(kThreads), 0, st, g4, m, patch);
}

// planar: the phase-planar form of layers 3, 2, 1 (kc unused); otherwise layer 0's rows in K chunks of kc floats
void launch_relu_bn_grad(hipStream_t st, bool planar, const float *dA, const float *a, const float *scale, int64_t m, int Ho, int Wo, int C, int kc, float *out)
{
    const int64_t elems4 = m * Ho * Wo * (C / 4);
    const dim3 grid((unsigned)gl_ceil_div(elems4, kThreads)), block(kThreads);
    if (planar)
        hipLaunchKernelGGL(relu_bn_grad_kernel<true>, grid, block, 0, st, dA, a, scale, m, Ho, Wo, C, 0, out);
    else
        hipLaunchKernelGGL(relu_bn_grad_kernel<false>, grid, block, 0, st, dA, a, scale, m, Ho, Wo, C, kc, out);
}

int upload_pack(gl_ctx *ctx, float **dev, const std::vector<float> &host)
{
    (void)hipFree(*dev);
    *dev = nullptr;
    GL_HIP(gl_device_alloc(ctx, (void **)dev, host.size() * sizeof(float)));
    GL_HIP(hipMemcpyAsync(*dev, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    GL_HIP(hipStreamSynchronize(ctx->stream));
    return GL_OK;
}

// the transposed packs, from the raw weights gl_dcgan_set_conv_weight kept on the host
int pack_grad_weights(gl_dcgan *g)
{
    if (!g->grad_dirty) return GL_OK;
    GL_HIP(hipStreamSynchronize(g->ctx->stream));          // an earlier gradient call may still read the packs this replaces
    for (int l = 0; l < 5; ++l) {
        const int ci_n = g->cin[l], co_n = g->cout[l];
        const std::vector<float> &w = g->h_w[l];
        auto W = [&](int ci, int co, int ky, int kx) { return w[(((size_t)ci * co_n + co) * 4 + ky) * 4 + kx]; };
        std::vector<float> pk;
        if (l == 0) {
            // [K chunk][z_dim -> cols_pad][kGradK0], k = (ky*4+kx) * C1 + co: the NHWC order of gpre_0's rows
            const size_t K = (size_t)16 * co_n, cols_pad = (size_t)gl_ceil_div(ci_n, 128) * 128;
            pk.assign(cols_pad * K, 0.0f);
            for (int ci = 0; ci < ci_n; ++ci)
                for (int ky = 0; ky < 4; ++ky)
                    for (int kx = 0; kx < 4; ++kx)
                        for (int co = 0; co < co_n; ++co) {
                            const size_t k = (size_t)(ky * 4 + kx) * co_n + co;
                            pk[((k / kGradK0) * cols_pad + ci) * kGradK0 + k % kGradK0] = W(ci, co, ky, kx);
                        }
        } else if (l < 4) {
            // [input phase][C_in -> cols_pad][K = 4 taps x C_out]
            const size_t K = (size_t)4 * co_n, cols_pad = (size_t)gl_ceil_div(ci_n, 128) * 128;
            pk.assign(4 * cols_pad * K, 0.0f);
            for (int py = 0; py < 2; ++py)
                for (int px = 0; px < 2; ++px)
                    for (int ty = 0; ty < 2; ++ty)
                        for (int tx = 0; tx < 2; ++tx) {
                            const int ky = kBwdKy[py][ty], kx = kBwdKy[px][tx], tap = ty * 2 + tx, phase = py * 2 + px;
                            for (int ci = 0; ci < ci_n; ++ci) {
                                float *dst = &pk[((size_t)phase * cols_pad + ci) * K];
                                for (int co = 0; co < co_n; ++co) dst[gl_conv_k_index(tap, co, 4)] = W(ci, co, ky, kx);
                            }
                        }
        } else {
            // [C_in -> cols_pad][K = 64], k = (ky*4+kx) * 3 + co, columns 48..63 zero
            const size_t K = 64, cols_pad = (size_t)gl_ceil_div(ci_n, 64) * 64;
            pk.assign(cols_pad * K, 0.0f);
            for (int ci = 0; ci < ci_n; ++ci)
                for (int ky = 0; ky < 4; ++ky)
                    for (int kx = 0; kx < 4; ++kx)
                        for (int co = 0; co < co_n; ++co) pk[(size_t)ci * K + (size_t)(ky * 4 + kx) * co_n + co] = W(ci, co, ky, kx);
        }
        const int rc = upload_pack(g->ctx, &g->gw[l], pk);
        if (rc != GL_OK) return rc;
    }
    if (g->have_att) {
        // [C -> cols_pad][K = 2 C/8 + C -> a multiple of 32], k the column of the rows [dq | dk | dv | 0]: one tap, so the K order is the identity
        const int C = g->cout[2], rows = g->att_cols;
        const size_t K = (size_t)gl_attention_grad_cols(C), cols_pad = (size_t)gl_ceil_div(C, 128) * 128;
        std::vector<float> pk(cols_pad * K, 0.0f);
        for (int c = 0; c < C; ++c)
            for (int k = 0; k < rows; ++k) pk[(size_t)c * K + k] = g->h_att_w[(size_t)k * C + c];
        const int rc = upload_pack(g->ctx, &g->gw_att, pk);
        if (rc != GL_OK) return rc;
    }
    g->grad_dirty = false;
    return GL_OK;
}

// images per pass: gl_dcgan_set_chunk's value (default 4096) under the 3 GiB a buffer descriptor may span -- the largest tensors here are a_3
// (32 x 32 x C3) and the patch rows (32 x 32 x 64)
int64_t grad_pass_images(const gl_dcgan *g)
{
    int64_t want = g->chunk > 0 ? g->chunk : 4096;
    const int widest = g->cout[3] > 64 ? g->cout[3] : 64;
    const int64_t cap = (int64_t)(0xB0000000ull / ((uint64_t)1024 * widest * 4));
    return want < cap ? want : cap;
}

int ensure_grad_workspace(gl_dcgan *g, int64_t n)
{
    int64_t want = grad_pass_images(g);
    if (n < want) want = n;
    if (want <= g->gws_chunk && (!g->have_att || g->gws_dqkv)) return GL_OK;
    if (want < g->gws_chunk) want = g->gws_chunk;
    GL_HIP(hipStreamSynchronize(g->ctx->stream));
    float **all[] = {&g->gws_y, &g->gws_g4, &g->gws_patch, &g->gws_da[0], &g->gws_da[1], &g->gws_da[2], &g->gws_da[3],
                     &g->gws_gp[0], &g->gws_gp[1], &g->gws_gp[2], &g->gws_gp[3], &g->gws_dqkv, &g->gws_att_stats};
    for (float **p : all) { (void)hipFree(*p); *p = nullptr; }
    g->gws_chunk = 0;
    GL_HIP(gl_device_alloc(g->ctx, (void **)&g->gws_y, (size_t)want * IMG * 4));
    GL_HIP(gl_device_alloc(g->ctx, (void **)&g->gws_g4, (size_t)want * IMG * 4));
    GL_HIP(gl_device_alloc(g->ctx, (void **)&g->gws_patch, (size_t)want * 1024 * 64 * 4));
    int hw = 16;
    for (int l = 0; l < 4; ++l) {
        GL_HIP(gl_device_alloc(g->ctx, (void **)&g->gws_da[l], (size_t)want * hw * g->cout[l] * 4));
        GL_HIP(gl_device_alloc(g->ctx, (void **)&g->gws_gp[l], (size_t)want * hw * g->cout[l] * 4));
        hw *= 4;
    }
    if (g->have_att) {
        GL_HIP(gl_device_alloc(g->ctx, (void **)&g->gws_dqkv, (size_t)want * 256 * gl_attention_grad_cols(g->cout[2]) * 4));
        GL_HIP(gl_device_alloc(g->ctx, (void **)&g->gws_att_stats, (size_t)want * 3 * 256 * 4));
    }
    g->gws_chunk = want;
    return GL_OK;
}

// the backward of one pass: g->ws_a holds the activations of these m images, y their output
int backward_pass(gl_dcgan *g, int64_t m, const float *y, const float *cot, const uint8_t *target, float *grad_z, float *loss)
{
    gl_ctx *ctx = g->ctx;
    launch_tanh_grad(ctx->stream, y, cot, target, m, g->gws_g4, loss);
    GL_LAUNCH_CHECK();
    launch_patch_rgb(ctx->stream, g->gws_g4, m, g->gws_patch);
    GL_LAUNCH_CHECK();
    // layer 4: dA_3 [m * 32 * 32][C3] = patch [.][64] x gw[4]^T
    {
        GlGatherConv p = {};
        p.in = g->gws_patch; p.positions = m * 1024; p.H = 32; p.W = 32; p.Cin = 64;
        p.wpack = g->gw[4]; p.cols = g->cin[4]; p.cols_pad = (int)gl_ceil_div(p.cols, 64) * 64; p.ntaps = 1;
        p.tap_dy[0] = 1; p.tap_dx[0] = 1;
        p.out = g->gws_da[3]; p.Ho = 32; p.Wo = 32; p.omul = 1;
        p.scale = g->ident_scale; p.shift = g->ident_shift; p.cmod = 1; p.act = 0; p.zero = ctx->zero_page;
        const int rc = gl_launch_gather_conv(ctx, p, 1);
        if (rc != GL_OK) return rc;
    }
    // layers 3, 2, 1: mask + BatchNorm scale into the phase-planar form, then four accumulated stride-1 gathers
    int hw = 16;                                             // grid of a_{l-1}
    for (int l = 3; l >= 1; --l) {
        const int Cl = g->cout[l];
        launch_relu_bn_grad(ctx->stream, true, g->gws_da[l], g->ws_a[l], g->scale[l], m, 2 * hw, 2 * hw, Cl, 0, g->gws_gp[l]);
        GL_LAUNCH_CHECK();
        const int K = 4 * Cl, cols_pad = (int)gl_ceil_div(g->cin[l], 128) * 128;
        for (int py = 0; py < 2; ++py)
            for (int px = 0; px < 2; ++px) {
                const int ph = py * 2 + px;
                GlGatherConv p = {};
                p.in = g->gws_gp[l] + (int64_t)ph * m * hw * hw * Cl;
                p.positions = m * hw * hw; p.H = hw; p.W = hw; p.Cin = Cl;
                p.wpack = g->gw[l] + (int64_t)ph * cols_pad * K; p.cols = g->cin[l]; p.cols_pad = cols_pad; p.ntaps = 4;
                uint32_t dy = 0, dx = 0;
                for (int ty = 0; ty < 2; ++ty)
                    for (int tx = 0; tx < 2; ++tx) {
                        const int tap = ty * 2 + tx;
                        dy |= (uint32_t)(kBwdDy[py][ty] + 1) << (2 * tap);
                        dx |= (uint32_t)(kBwdDy[px][tx] + 1) << (2 * tap);
                    }
                p.tap_dy[0] = dy; p.tap_dx[0] = dx;
                p.out = g->gws_da[l - 1]; p.Ho = hw; p.Wo = hw; p.omul = 1;
                p.scale = g->ident_scale; p.shift = g->ident_shift; p.cmod = 1; p.act = 0; p.zero = ctx->zero_page;
                p.residual = ph ? g->gws_da[l - 1] : nullptr;
                const int rc = gl_launch_gather_conv(ctx, p, 1);
                if (rc != GL_OK) return rc;
            }
        if (l == 3 && g->have_att) {
            // layer 3 read the attention block's output: gws_da[2] is dY.  dX = dY + [dq | dk | dv | 0] x [Wq; Wk; Wv], in place
            const int C = g->cout[2], K = gl_attention_grad_cols(C);
            int rc = gl_launch_attention_grad(ctx, C, g->ws_qkv, g->gws_da[2], g->att_gamma, m, g->gws_dqkv, g->gws_att_stats);
            if (rc != GL_OK) return rc;
            GlGatherConv p = {};
            p.in = g->gws_dqkv; p.positions = m * 256; p.H = 16; p.W = 16; p.Cin = K;
            p.wpack = g->gw_att; p.cols = C; p.cols_pad = (int)gl_ceil_div(C, 128) * 128; p.ntaps = 1;
            p.tap_dy[0] = 1; p.tap_dx[0] = 1;
            p.out = g->gws_da[2]; p.Ho = 16; p.Wo = 16; p.omul = 1;
            p.scale = g->ident_scale; p.shift = g->ident_shift; p.cmod = 1; p.act = 0; p.zero = ctx->zero_page;
            p.residual = g->gws_da[2];
            rc = gl_launch_gather_conv(ctx, p, 1);
            if (rc != GL_OK) return rc;
        }
        hw /= 2;
    }
    // layer 0: gpre_0 rows [m][16 C1] x gw[0]^T -> grad_z [m][z_dim].  K = 16 C1 is by far the longest sum of the path (16 384 terms at
    // features_g = 64) and the matrix cores add it term after term in fp32, so it is cut into chunks of kGradK0 terms that are added through
    // the residual, in ascending order: the rounding error of a row stays that of a kGradK0-term sum whatever the width.
    {
        const int C1 = g->cout[0], chunks = 16 * C1 / kGradK0;
        launch_relu_bn_grad(ctx->stream, false, g->gws_da[0], g->ws_a[0], g->scale[0], m, 4, 4, C1, kGradK0, g->gws_gp[0]);
        GL_LAUNCH_CHECK();
        const int cols_pad = (int)gl_ceil_div(g->z_dim, 128) * 128;
        for (int ch = 0; ch < chunks; ++ch) {
            GlGatherConv p = {};
            p.in = g->gws_gp[0] + (int64_t)ch * m * kGradK0; p.positions = m; p.H = 1; p.W = 1; p.Cin = kGradK0;
            p.wpack = g->gw[0] + (int64_t)ch * cols_pad * kGradK0; p.cols = g->z_dim; p.cols_pad = cols_pad; p.ntaps = 1;
            p.tap_dy[0] = 1; p.tap_dx[0] = 1;
            p.out = grad_z; p.Ho = 1; p.Wo = 1; p.omul = 1;
            p.scale = g->ident_scale; p.shift = g->ident_shift; p.cmod = 1; p.act = 0; p.zero = ctx->zero_page;
            p.residual = ch ? grad_z : nullptr;
            const int rc = gl_launch_gather_conv(ctx, p, 1);
            if (rc != GL_OK) return rc;
        }
    }
    return GL_OK;
}

int grad_passes(gl_dcgan *g, const float *z, int64_t n, const float *cot, const uint8_t *target, float *grad_z, float *out_f32, float *loss)
{
    int rc = pack_grad_weights(g);
    if (rc == GL_OK) rc = ensure_grad_workspace(g, n);
    if (rc != GL_OK) return rc;
    const int64_t per_pass = grad_pass_images(g);
    for (int64_t i0 = 0; i0 < n;) {
        // the forward cuts a call into passes of a multiple of 512 images once its workspace holds that many: ask for sizes it runs as ONE pass
        int64_t m = n - i0 < per_pass ? n - i0 : per_pass;
        if (m > 512) m -= m % 512;
        float *y = out_f32 ? out_f32 + i0 * IMG : g->gws_y;
        rc = gl_dcgan_forward(g, z + i0 * g->z_dim, m, y, nullptr);
        if (rc != GL_OK) return rc;
        if (g->fwd_last_m != m) {
            gl_set_error("gl_dcgan gradient: the forward ran %lld images as more than one pass", (long long)m);
            return GL_ERR_STATE;
        }
        rc = backward_pass(g, m, y, cot ? cot + i0 * IMG : nullptr, target ? target + i0 * IMG : nullptr, grad_z + i0 * g->z_dim, loss ? loss + i0 : nullptr);
        if (rc != GL_OK) return rc;
        i0 += m;
    }
    return GL_OK;
}

// checks shared by the two entry points; *run says whether there is anything to do
int grad_enter(gl_dcgan *g, int64_t n, const char *who, bool *run)
{
    *run = false;
    GL_REQUIRE(g && n >= 0, "%s: bad argument", who);
    for (int l = 0; l < 5; ++l)
        if (!g->have_w[l] || (l < 4 && !g->have_bn[l])) {
            gl_set_error("%s: weights of layer %d not loaded", who, l);
            return GL_ERR_STATE;
        }
    if (!g->have_bias) { gl_set_error("%s: gen.4.bias not loaded", who); return GL_ERR_STATE; }
    bool sn = false;
    for (int l = 0; l < 4; ++l) sn |= g->have_sn[l];
    // with the spectral-norm state held (gl_dcgan_set_spectral_hold) g->scale[l] carries bn_scale / sigma and G is a fixed function of z; a state that
    // every forward advances is not, and that includes the plain VAEGAN stack (attention comes with spectral normalisation there)
    if ((g->have_att || sn) && !g->sn_hold) {
        gl_set_error("%s: generators with self-attention or spectral normalisation (VAEGAN) have no backward pass", who);
        return GL_ERR_STATE;
    }
    *run = n > 0;
    return GL_OK;
}

}  // namespace

extern "C" {

int gl_dcgan_vjp_z(gl_dcgan *g, const float *z_dev, int64_t n, const float *cot_dev, float *grad_z_dev, float *out_f32_dev)
{
    gl_make_current(g ? g->ctx : nullptr);
    bool run;
    int rc = grad_enter(g, n, "gl_dcgan_vjp_z", &run);
    if (rc != GL_OK || !run) return rc;
    GL_REQUIRE(z_dev && cot_dev && grad_z_dev, "gl_dcgan_vjp_z: NULL device pointer");
    GL_REQUIRE(((reinterpret_cast<uintptr_t>(cot_dev) | reinterpret_cast<uintptr_t>(out_f32_dev)) & 15) == 0,
               "gl_dcgan_vjp_z: cot_dev and out_f32_dev must be 16-byte aligned");
    const int precision = g->precision;
    g->precision = 0;                                       // the kept activations are the fp32-product forward's
    rc = grad_passes(g, z_dev, n, cot_dev, nullptr, grad_z_dev, out_f32_dev, nullptr);
    g->precision = precision;
    return rc;
}

int gl_dcgan_l2_grad_z(gl_dcgan *g, const float *z_dev, const uint8_t *target_u8_dev, int64_t n, float *grad_z_dev, float *loss_dev)
{
    gl_make_current(g ? g->ctx : nullptr);
    bool run;
    int rc = grad_enter(g, n, "gl_dcgan_l2_grad_z", &run);
    if (rc != GL_OK || !run) return rc;
    GL_REQUIRE(z_dev && target_u8_dev && grad_z_dev && loss_dev, "gl_dcgan_l2_grad_z: NULL device pointer");
    GL_REQUIRE((reinterpret_cast<uintptr_t>(target_u8_dev) & 3) == 0, "gl_dcgan_l2_grad_z: target_u8_dev must be 4-byte aligned");
    const int precision = g->precision;
    g->precision = 0;
    rc = grad_passes(g, z_dev, n, nullptr, target_u8_dev, grad_z_dev, nullptr, loss_dev);
    g->precision = precision;
    return rc;
}

}  // extern "C"

#ifdef GL_TUNING
// One launch of one kernel of this file on device buffers that gl_tune_grad_op (gl_tune.hip) has put between guards: through the launchers
// backward_pass uses.  ip[0] = images.  nb: the bytes of in[0 .. 3] and out[0 .. 1] (0 for a NULL slot); every buffer a kernel touches must have
// exactly the size its shape gives.
#define GL_TUNE_NEED(slot, bytes)                                                                                                              \
    GL_REQUIRE(nb[slot] == (int64_t)(bytes), "%s: buffer %d (inputs 0 - 3, outputs 4 - 5) has %lld bytes, the shape needs %lld", __func__, slot, \
               (long long)nb[slot], (long long)(bytes))
int gl_tune_dcgan_grad_op(gl_ctx *ctx, int op, const int64_t *ip, const int64_t *nb, void *const *in, void *const *out)
{
    hipStream_t st = ctx->stream;
    const int64_t m = ip[0];
    GL_REQUIRE(m > 0 && m <= 4096, "gl_tune_dcgan_grad_op: images in 1..4096");
    switch (op) {
    case 0:   // tanh_grad_kernel<false>: in = y, cot [m][3][64][64]; out = g4
        GL_TUNE_NEED(0, m * IMG * 4);
        GL_TUNE_NEED(1, m * IMG * 4);
        GL_TUNE_NEED(4, m * IMG * 4);
        launch_tanh_grad(st, (const float *)in[0], (const float *)in[1], nullptr, m, (float *)out[0], nullptr);
        break;
    case 1:   // tanh_grad_kernel<true>: in = y, target codes; out = g4, loss [m]
        GL_TUNE_NEED(0, m * IMG * 4);
        GL_TUNE_NEED(1, m * IMG);
        GL_TUNE_NEED(4, m * IMG * 4);
        GL_TUNE_NEED(5, m * 4);
        launch_tanh_grad(st, (const float *)in[0], nullptr, (const uint8_t *)in[1], m, (float *)out[0], (float *)out[1]);
        break;
    case 2:   // patch_rgb_kernel: in = g4 [m][3][64][64]; out = patch [m][1024][64]
        GL_TUNE_NEED(0, m * IMG * 4);
        GL_TUNE_NEED(4, m * 1024 * 64 * 4);
        launch_patch_rgb(st, (const float *)in[0], m, (float *)out[0]);
        break;
    case 3: { // relu_bn_grad_kernel<ip[4] != 0>: ip[1..3] = Ho, Wo, C, ip[5] = kc; in = dA, a [m][Ho][Wo][C], scale [C]; out = gpre
        GL_REQUIRE(ip[1] > 0 && ip[1] <= 1024 && ip[2] > 0 && ip[2] <= 1024 && ip[3] > 0 && ip[3] <= 4096 && ip[3] % 4 == 0, "gl_tune_dcgan_grad_op: bad shape");
        GL_REQUIRE(ip[4] ? (ip[1] % 2 == 0 && ip[2] % 2 == 0) : (ip[5] > 0 && ip[5] % 4 == 0 && (ip[1] * ip[2] * ip[3]) % ip[5] == 0),
                   "gl_tune_dcgan_grad_op: odd grid, or kc does not divide the row");
        const int64_t bytes = m * ip[1] * ip[2] * ip[3] * 4;
        GL_TUNE_NEED(0, bytes);
        GL_TUNE_NEED(1, bytes);
        GL_TUNE_NEED(2, ip[3] * 4);
        GL_TUNE_NEED(4, bytes);
        launch_relu_bn_grad(st, ip[4] != 0, (const float *)in[0], (const float *)in[1], (const float *)in[2], m, (int)ip[1], (int)ip[2], (int)ip[3], (int)ip[5],
                            (float *)out[0]);
        break;
    }
    default:
        gl_set_error("gl_tune_dcgan_grad_op: unknown op %d", op);
        return GL_ERR_INVALID;
    }
    GL_LAUNCH_CHECK();
    return GL_OK;
}
#undef GL_TUNE_NEED
#endif
