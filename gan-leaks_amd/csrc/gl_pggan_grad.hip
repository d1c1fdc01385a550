// Gradient of the progressive-GAN generator with respect to its latent input: grad_z = (dG/dz)^T cot, the white-box attack's hot path on PGGAN.
//
// A pass of m images first runs the forward with fp32 products in keep mode (gl_pggan_forward, precision 0): every layer's output stays in a
// buffer of its own -- layer 0 (ConvTranspose2d) after its LeakyReLU, every 3 x 3 layer after LeakyReLU and PixelNorm -- together with the
// PixelNorm factor `inv` of every position.  Backwards, with layers numbered as in gl_pggan.h:
//   g            = cot * (1 - y^2)                      (steps == 0: g = cot, the output has no tanh)
//   dA_top       = alpha g x W_rgb[steps];  the second toRGB branch gives (1 - alpha) * (2 x 2 cell sums of g) x W_rgb[steps-1] at half resolution,
//                  added to the gradient that reaches the block's input through the block (block first, then rgb); skipped at alpha == 1
//   gpre_l       = slope(a_l) inv_l (dA_l - a_l mean_c(dA_l a_l)),  slope = 1 where a > 0, else 0.2       (PixelNorm and LeakyReLU, one wave per position)
//   dIn_l        = conv3x3(gpre_l) with the taps mirrored, the weight matrix transposed and sqrt(2 / (9 C_in)) folded into the pack: the forward's
//                  fp32 tap-gather GEMM (gl_launch_gather_conv) with C_in(l) columns, one launch per 128 channels of gpre_l (kConvChunk below)
//   upsampling   : the first convolution of a block reads through nearest x2, so its dIn lives on the full-resolution grid; the next PixelNorm
//                  gradient kernel loads (00 + 01) + (10 + 11) of every 2 x 2 cell
//   d zn         = gpre_0 [m][16 C] x W_init in K chunks of 1024 terms added through the GEMM's residual in ascending order
//   dz           = inv_z (d zn - zn mean(d zn zn)), zn and inv_z recomputed from z                           (PixelNorm of the latent)
// No atomics and no split whose order depends on the launch: every output is one fixed-order fp32 sum, and a row depends on its image alone.
// The backward adds no matrix-core kernel of its own.  Transposed packs and workspaces are built on the first gradient call only.
#include "gl_pggan.h"
#include <cmath>

namespace {

constexpr int kThreads = 256;
// The matrix cores add a GEMM row term after term in fp32, so the rounding error of a K-term sum grows like sqrt(K).  At 512 channels the 3 x 3
// data gradient has K = 4608 and the last GEMM K = 8192, and with each as one sum a gradient row measured 4.0x the error of float32 autograd on
// the host (which blocks its sums).  Both are therefore cut into fixed chunks that are added through the GEMM's residual in ascending order:
constexpr int kGradK0 = 1024;                      // K chunk of the last GEMM
constexpr int kConvChunk = 128;                    // channels of gpre per launch of a 3 x 3 data gradient (K = 1152); up to 128 channels: one launch
constexpr uint64_t kKeepBytes = 1536ull << 20;     // default pass: kept activations of at most this many bytes

struct Layer { int hw, C, cin; };
Layer layer_of(const gl_pggan *g, int l)
{
    if (l < 2) return Layer{4, g->C, l == 0 ? g->z_pad : g->C};
    const int s = (l - 2) / 2;
    return Layer{4 << (s + 1), g->cout[s], (l & 1) ? g->cout[s] : g->cin[s]};
}
int cols_pad_of(int cols) { return cols % 128 == 0 ? cols : (int)gl_ceil_div(cols, 64) * 64; }

// one workgroup per image of `img` values (NCHW).  L2: cot = 2 (y - x), x = 2 u / 255 - 1 the target's value, and loss = sum (y - x)^2 -- the
// squares are added in double, per thread over its strided share and then down a fixed tree.  g = cot * (1 - y^2), or cot without tanh.
template <bool L2>
__global__ void __launch_bounds__(kThreads) pg_out_grad_kernel(const float *__restrict__ y, const float *__restrict__ cot, const uint8_t *__restrict__ target,
                                                               int img, int use_tanh, float *__restrict__ gout, float *__restrict__ loss)
{
    __shared__ double red[kThreads];
    const int64_t base = (int64_t)blockIdx.x * img;
    double acc = 0.0;
    for (int i = threadIdx.x; i < img; i += kThreads) {
        const float yy = y[base + i];
        float c;
        if constexpr (L2) {
            const float diff = yy - (2.0f * ((float)target[base + i] / 255.0f) - 1.0f);
            acc += (double)diff * (double)diff;
            c = 2.0f * diff;
        } else {
            c = cot[base + i];
        }
        gout[base + i] = use_tanh ? c * (1.0f - yy * yy) : c;
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

// toRGB backwards (K = nc <= 4: element-wise).  dA[pos][c] = sum_o d[o] w[o * C + c] over the H x H grid of dA, one thread per element, o ascending;
// d[o] = factor * gout[n][o][y][x], or with `pool` factor * ((g00 + g01) + (g10 + g11)) of the 2 x 2 cell of the 2H x 2H image.
// w: the forward's toRGB pack (gl_pggan_set_rgb), the input scale folded in.
__global__ void __launch_bounds__(kThreads) pg_rgb_grad_kernel(const float *__restrict__ gout, const float *__restrict__ w, int64_t total, int H, int C, int nc,
                                                               int pool, float factor, float *__restrict__ dA)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    int64_t r = i / C;
    const int x = (int)(r % H);
    r /= H;
    const int y = (int)(r % H);
    const int64_t n = r / H;
    const int R = pool ? 2 * H : H;
    float acc = 0.0f;
    for (int o = 0; o < nc; ++o) {
        const float *p = gout + ((n * nc + o) * R + (pool ? 2 * y : y)) * (int64_t)R + (pool ? 2 * x : x);
        const float d = pool ? __fmul_rn(factor, __fadd_rn(__fadd_rn(p[0], p[1]), __fadd_rn(p[R], p[R + 1]))) : __fmul_rn(factor, p[0]);
        acc = fmaf(d, w[(int64_t)o * C + c], acc);
    }
    dA[i] = acc;
}

// PixelNorm + LeakyReLU backwards, one wave per position of the H x H grid: with a = leaky * inv the kept activation,
//   gpre = slope(a) inv (d - a mean_c(d a)),  d = dA[pos][c], or with `pool` (dA on the 2H x 2H grid) (00 + 01) + (10 + 11) of the position's cell,
// plus extra[pos][c] when given.  The channel sum is one fmaf chain per lane over c = lane, lane + 64, ..., then the xor butterfly 32 .. 1.
// out is cut into chunks of kConvChunk channels, [chunk][pos][<= kConvChunk]: the inputs of the data gradient's launches.
__global__ void __launch_bounds__(kThreads) pg_pn_grad_kernel(const float *__restrict__ dA, const float *__restrict__ a, const float *__restrict__ inv,
                                                              const float *__restrict__ extra, int64_t positions, int H, int C, int pool,
                                                              float *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t pos = wave; pos < positions; pos += nwaves) {
        const float *src = dA + pos * C;
        const int64_t row = (int64_t)2 * H * C;          // one row of the 2H x 2H grid
        if (pool) {
            const int x = (int)(pos % H);
            const int64_t r = pos / H;
            const int y = (int)(r % H);
            const int64_t n = r / H;
            src = dA + ((n * 2 * H + 2 * y) * 2 * H + 2 * x) * (int64_t)C;
        }
        const float *ap = a + pos * C, *ep = extra ? extra + pos * C : nullptr;
        auto load = [&](int c) {
            float d = pool ? __fadd_rn(__fadd_rn(src[c], src[C + c]), __fadd_rn(src[row + c], src[row + C + c])) : src[c];
            if (ep) d = __fadd_rn(d, ep[c]);
            return d;
        };
        float s = 0.0f;
        for (int c = lane; c < C; c += 64) s = fmaf(load(c), ap[c], s);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        const float mean = s / (float)C, iv = inv[pos];
        for (int c = lane; c < C; c += 64) {
            const float av = ap[c];
            const float t = __fmul_rn(iv, __fsub_rn(load(c), __fmul_rn(av, mean)));
            const int c0 = c & ~(kConvChunk - 1);
            const int cc = C - c0 < kConvChunk ? C - c0 : kConvChunk;
            out[(int64_t)c0 * positions + pos * cc + (c - c0)] = av > 0.0f ? t : __fmul_rn(0.2f, t);
        }
    }
}

// layer 0 (LeakyReLU only): gpre = slope(h) dA over the rows [n][K] (K = 16 C), cut into K chunks of kGradK0 floats: [chunk][n][<= kGradK0]
__global__ void __launch_bounds__(kThreads) pg_leaky_grad_kernel(const float *__restrict__ dA, const float *__restrict__ h, int64_t n_img, int K,
                                                                 float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_img * K) return;
    const int64_t img = i / K;
    const int k = (int)(i - img * K);
    const int ch = k / kGradK0, k0 = ch * kGradK0;
    const int kc = K - k0 < kGradK0 ? K - k0 : kGradK0;
    const float d = dA[i];
    out[(int64_t)ch * n_img * kGradK0 + img * kc + (k - k0)] = h[i] > 0.0f ? d : __fmul_rn(0.2f, d);
}

// PixelNorm of the latent backwards, in place on grad [n][d] (holding d zn): dz = inv (d zn - zn mean(d zn zn)), zn = z inv as the forward forms
// them (pixelnorm_rows_kernel).  One wave per row.
__global__ void __launch_bounds__(kThreads) pg_rowpn_grad_kernel(const float *__restrict__ z, int64_t n, int d, float *__restrict__ grad)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (row >= n) return;
    const float *src = z + row * d;
    float *gp = grad + row * d;
    float ss = 0.0f;
    for (int c = lane; c < d; c += 64) { const float t = src[c]; ss = fmaf(t, t, ss); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const float inv = 1.0f / sqrtf(ss / (float)d + 1e-8f);
    float s = 0.0f;
    for (int c = lane; c < d; c += 64) s = fmaf(gp[c], __fmul_rn(src[c], inv), s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mean = s / (float)d;
    for (int c = lane; c < d; c += 64) gp[c] = __fmul_rn(inv, __fsub_rn(gp[c], __fmul_rn(__fmul_rn(src[c], inv), mean)));
}

// One launch of every kernel above, with its grid and its template instance: backward_pass and the tuning build's single-launch hook
// (gl_tune_pggan_grad_op, at the end of this file) both go through these.
void launch_out_grad(hipStream_t st, const float *y, const float *cot, const uint8_t *target, int64_t m, int img, int use_tanh, float *gout, float *loss)
{
    if (target)
        hipLaunchKernelGGL(pg_out_grad_kernel<true>, dim3((unsigned)m), dim3(kThreads), 0, st, y, (const float *)nullptr, target, img, use_tanh, gout, loss);
    else
        hipLaunchKernelGGL(pg_out_grad_kernel<false>, dim3((unsigned)m), dim3(kThreads), 0, st, y, cot, (const uint8_t *)nullptr, img, use_tanh, gout,
                           (float *)nullptr);
}

// H: the grid of dA (half the image's with `pool`)
void launch_rgb_grad(hipStream_t st, const float *gout, const float *w, int64_t m, int H, int C, int nc, int pool, float factor, float *dA)
{
    const int64_t total = m * H * H * C;
    hipLaunchKernelGGL(pg_rgb_grad_kernel, dim3((unsigned)gl_ceil_div(total, kThreads)), dim3(kThreads), 0, st, gout, w, total, H, C, nc, pool, factor, dA);
}

void launch_pn_grad(hipStream_t st, const float *dA, const float *a, const float *inv, const float *extra, int64_t m, int H, int C, int pool, float *out)
{
    const int64_t positions = m * H * H;
    int64_t blocks = gl_ceil_div(positions, 4);
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(pg_pn_grad_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, dA, a, inv, extra, positions, H, C, pool, out);
}

void launch_leaky_grad(hipStream_t st, const float *dA, const float *h, int64_t m, int K, float *out)
{
    hipLaunchKernelGGL(pg_leaky_grad_kernel, dim3((unsigned)gl_ceil_div(m * K, kThreads)), dim3(kThreads), 0, st, dA, h, m, K, out);
}

void launch_rowpn_grad(hipStream_t st, const float *z, int64_t m, int d, float *grad)
{
    hipLaunchKernelGGL(pg_rowpn_grad_kernel, dim3((unsigned)gl_ceil_div(m, 4)), dim3(kThreads), 0, st, z, m, d, grad);
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

// the transposed packs of every loaded layer, from the raw weights gl_pggan_set_initial / gl_pggan_set_block kept on the host
int pack_grad_weights(gl_pggan *g)
{
    if (!g->grad_dirty) return GL_OK;
    GL_HIP(hipStreamSynchronize(g->ctx->stream));          // an earlier gradient call may still read the packs this replaces
    {
        // [K chunk][z_dim -> cols_pad][<= kGradK0], k = (ky*4+kx) * C + co: the NHWC order of gpre_0's rows
        const int C = g->C, K = 16 * C;
        const size_t cols_pad = (size_t)gl_ceil_div(g->z_dim, 128) * 128;
        std::vector<float> pk(cols_pad * K, 0.0f);
        for (int ci = 0; ci < g->z_dim; ++ci)
            for (int co = 0; co < C; ++co)
                for (int t = 0; t < 16; ++t) {
                    const int k = t * C + co, ch = k / kGradK0, k0 = ch * kGradK0;
                    const int kc = K - k0 < kGradK0 ? K - k0 : kGradK0;
                    pk[(size_t)ch * cols_pad * kGradK0 + (size_t)ci * kc + (k - k0)] = g->h_init_w[((size_t)ci * C + co) * 16 + t];
                }
        const int rc = upload_pack(g->ctx, &g->gw[0], pk);
        if (rc != GL_OK) return rc;
    }
    for (int l = 1; l < kPgLayers; ++l) {
        if (l >= 2 && !g->have_blk[(l - 2) / 2]) continue;
        const Layer L = layer_of(g, l);
        const int K = 9 * L.C;
        const double scale = std::sqrt(2.0 / (9.0 * (double)L.cin));
        const std::vector<float> &w = g->h_conv_w[l];       // [C_out][C_in][3][3]
        // [channel chunk of gpre][C_in -> cols_pad][9 taps x <= kConvChunk channels]
        const size_t cols_pad = (size_t)cols_pad_of(L.cin);
        std::vector<float> pk(cols_pad * K, 0.0f);
        for (int co = 0; co < L.C; ++co) {
            const int c0 = co & ~(kConvChunk - 1);
            const int cc = L.C - c0 < kConvChunk ? L.C - c0 : kConvChunk;
            for (int ci = 0; ci < L.cin; ++ci)
                for (int t = 0; t < 9; ++t)
                    pk[(size_t)c0 * 9 * cols_pad + (size_t)ci * 9 * cc + gl_conv_k_index(t, co - c0, 9)] =
                        (float)((double)w[((size_t)co * L.cin + ci) * 9 + (8 - t)] * scale);
        }
        const int rc = upload_pack(g->ctx, &g->gw[l], pk);
        if (rc != GL_OK) return rc;
    }
    g->grad_dirty = false;
    return GL_OK;
}

// floats per image: the kept activations with their PixelNorm factors, and the widest tensor a rolling gradient buffer has to hold (the data
// gradient of a block's first convolution lives on the full-resolution grid with the block's INPUT channels)
void grad_sizes(const gl_pggan *g, int steps, size_t *kept, size_t *widest)
{
    *kept = 0;
    *widest = 0;
    for (int l = 0; l < 2 + 2 * steps; ++l) {
        const Layer L = layer_of(g, l);
        const size_t hw2 = (size_t)L.hw * L.hw;
        *kept += hw2 * L.C + hw2;
        const size_t w = hw2 * (l >= 1 && L.cin > L.C ? L.cin : L.C);
        if (w > *widest) *widest = w;
    }
}

// images per pass: gl_pggan_set_chunk's value, else what keeps the kept activations under kKeepBytes; under the 3 GiB a buffer descriptor may span
int64_t grad_pass_images(const gl_pggan *g, int steps)
{
    size_t kept, widest;
    grad_sizes(g, steps, &kept, &widest);
    int64_t want = g->chunk > 0 ? g->chunk : (int64_t)(kKeepBytes / (kept * 4));
    const int64_t cap = (int64_t)(0xB0000000ull / (widest * 4));
    if (want > cap) want = cap;
    return want < 1 ? 1 : want;
}

void free_grad_workspace(gl_pggan *g)
{
    for (int l = 0; l < kPgLayers; ++l) {
        (void)hipFree(g->keep_act[l]); (void)hipFree(g->keep_inv[l]);
        g->keep_act[l] = g->keep_inv[l] = nullptr;
    }
    float **all[] = {&g->gws_y, &g->gws_g, &g->gws_roll[0], &g->gws_roll[1], &g->gws_roll[2]};
    for (float **p : all) { (void)hipFree(*p); *p = nullptr; }
    g->gws_imgs = 0;
    g->gws_steps = -1;
}

int ensure_grad_workspace(gl_pggan *g, int steps, int64_t n)
{
    int64_t want = grad_pass_images(g, steps);
    if (n < want) want = n;
    if (steps == g->gws_steps && want <= g->gws_imgs) return GL_OK;
    GL_HIP(hipStreamSynchronize(g->ctx->stream));
    free_grad_workspace(g);
    size_t kept, widest;
    grad_sizes(g, steps, &kept, &widest);
    const size_t img = (size_t)g->nc * (4 << steps) * (4 << steps);
    for (int l = 0; l < 2 + 2 * steps; ++l) {
        const Layer L = layer_of(g, l);
        const size_t hw2 = (size_t)L.hw * L.hw;
        GL_HIP(gl_device_alloc(g->ctx, (void **)&g->keep_act[l], (size_t)want * hw2 * L.C * 4));
        if (l >= 1) GL_HIP(gl_device_alloc(g->ctx, (void **)&g->keep_inv[l], (size_t)want * hw2 * 4));
    }
    GL_HIP(gl_device_alloc(g->ctx, (void **)&g->gws_y, (size_t)want * img * 4));
    GL_HIP(gl_device_alloc(g->ctx, (void **)&g->gws_g, (size_t)want * img * 4));
    for (int k = 0; k < 3; ++k) GL_HIP(gl_device_alloc(g->ctx, (void **)&g->gws_roll[k], (size_t)want * widest * 4));
    g->gws_imgs = want;
    g->gws_steps = steps;
    return GL_OK;
}

int conv_bwd(gl_pggan *g, int l, int64_t m, const float *gpre, float *out)
{
    const Layer L = layer_of(g, l);
    const int64_t positions = m * L.hw * L.hw;
    const int cols_pad = cols_pad_of(L.cin);
    uint32_t dy = 0, dx = 0;
    for (int t = 0; t < 9; ++t) { dy |= (uint32_t)(t / 3) << (2 * t); dx |= (uint32_t)(t % 3) << (2 * t); }
    for (int c0 = 0; c0 < L.C; c0 += kConvChunk) {
        GlGatherConv p = {};
        p.in = gpre + (int64_t)c0 * positions; p.positions = positions; p.H = L.hw; p.W = L.hw; p.up = 0;
        p.Cin = L.C - c0 < kConvChunk ? L.C - c0 : kConvChunk;
        p.wpack = g->gw[l] + (int64_t)c0 * 9 * cols_pad; p.cols = L.cin; p.cols_pad = cols_pad; p.ntaps = 9;
        p.tap_dy[0] = dy; p.tap_dx[0] = dx;
        p.out = out; p.Ho = L.hw; p.Wo = L.hw; p.omul = 1;
        p.scale = g->ones; p.shift = g->ctx->zero_page; p.cmod = 1; p.act = 0; p.zero = g->ctx->zero_page;
        p.residual = c0 ? out : nullptr;
        const int rc = gl_launch_gather_conv(g->ctx, p, 1);
        if (rc != GL_OK) return rc;
    }
    return GL_OK;
}

// the backward of one pass: keep_act / keep_inv hold the activations of these m images, y their output
int backward_pass(gl_pggan *g, int64_t m, int steps, float alpha, const float *z, const float *y, const float *cot, const uint8_t *target, float *grad_z,
                  float *loss)
{
    gl_ctx *ctx = g->ctx;
    const int R = 4 << steps, nc = g->nc, top = 1 + 2 * steps, img = nc * R * R;
    launch_out_grad(ctx->stream, y, cot, target, m, img, steps > 0 ? 1 : 0, g->gws_g, loss);
    GL_LAUNCH_CHECK();
    float *A = g->gws_roll[0], *B = g->gws_roll[1], *E = nullptr;
    {
        const Layer L = layer_of(g, top);
        launch_rgb_grad(ctx->stream, g->gws_g, g->w_rgb[steps], m, R, L.C, nc, 0, steps > 0 ? alpha : 1.0f, A);
        GL_LAUNCH_CHECK();
    }
    if (steps > 0 && alpha != 1.0f) {
        const Layer L = layer_of(g, top - 2);
        E = g->gws_roll[2];
        launch_rgb_grad(ctx->stream, g->gws_g, g->w_rgb[steps - 1], m, R / 2, L.C, nc, 1, 1.0f - alpha, E);
        GL_LAUNCH_CHECK();
    }
    bool pooled = false;      // A holds the gradient on the 2x grid of the layer that takes it next
    for (int l = top; l >= 1; --l) {
        const Layer L = layer_of(g, l);
        launch_pn_grad(ctx->stream, A, g->keep_act[l], g->keep_inv[l], l == top - 2 ? E : (const float *)nullptr, m, L.hw, L.C, pooled ? 1 : 0, B);
        GL_LAUNCH_CHECK();
        const int rc = conv_bwd(g, l, m, B, A);
        if (rc != GL_OK) return rc;
        pooled = l >= 2 && (l & 1) == 0;      // conv1 of a block read its input through the upsampling
    }
    // layer 0: gpre_0 rows [m][16 C] x gw[0]^T -> grad_z [m][z_dim].  K = 16 C is the longest sum of the path (8192 terms at 512 channels): chunks of
    // kGradK0 terms added through the residual, in ascending order
    {
        const int K = 16 * g->C, chunks = (int)gl_ceil_div(K, kGradK0);
        launch_leaky_grad(ctx->stream, A, g->keep_act[0], m, K, B);
        GL_LAUNCH_CHECK();
        const int cols_pad = (int)gl_ceil_div(g->z_dim, 128) * 128;
        for (int ch = 0; ch < chunks; ++ch) {
            const int k0 = ch * kGradK0, kc = K - k0 < kGradK0 ? K - k0 : kGradK0;
            GlGatherConv p = {};
            p.in = B + (int64_t)ch * m * kGradK0; p.positions = m; p.H = 1; p.W = 1; p.Cin = kc;
            p.wpack = g->gw[0] + (int64_t)ch * cols_pad * kGradK0; p.cols = g->z_dim; p.cols_pad = cols_pad; p.ntaps = 1;
            p.tap_dy[0] = 1; p.tap_dx[0] = 1;
            p.out = grad_z; p.Ho = 1; p.Wo = 1; p.omul = 1;
            p.scale = g->ones; p.shift = ctx->zero_page; p.cmod = 1; p.act = 0; p.zero = ctx->zero_page;
            p.residual = ch ? grad_z : nullptr;
            const int rc = gl_launch_gather_conv(ctx, p, 1);
            if (rc != GL_OK) return rc;
        }
        launch_rowpn_grad(ctx->stream, z, m, g->z_dim, grad_z);
        GL_LAUNCH_CHECK();
    }
    return GL_OK;
}

int grad_passes(gl_pggan *g, const float *z, int64_t n, int steps, float alpha, const float *cot, const uint8_t *target, float *grad_z, float *out_f32,
                float *loss)
{
    int rc = pack_grad_weights(g);
    if (rc == GL_OK) rc = ensure_grad_workspace(g, steps, n);
    if (rc != GL_OK) return rc;
    const int64_t per_pass = grad_pass_images(g, steps) < g->gws_imgs ? grad_pass_images(g, steps) : g->gws_imgs;
    const int64_t img = (int64_t)g->nc * (4 << steps) * (4 << steps);
    // the forward of a pass: fp32 products, keep mode, and a chunk that makes it run these m images as one pass; all three restored
    const int precision = g->precision;
    const int64_t chunk = g->chunk;
    for (int64_t i0 = 0; i0 < n && rc == GL_OK; i0 += per_pass) {
        const int64_t m = n - i0 < per_pass ? n - i0 : per_pass;
        float *y = out_f32 ? out_f32 + i0 * img : g->gws_y;
        g->precision = 0; g->keep = true; g->chunk = m;
        rc = gl_pggan_forward(g, z + i0 * g->z_dim, m, steps, alpha, y, nullptr);
        g->precision = precision; g->keep = false; g->chunk = chunk;
        if (rc == GL_OK)
            rc = backward_pass(g, m, steps, alpha, z + i0 * g->z_dim, y, cot ? cot + i0 * img : nullptr, target ? target + i0 * img : nullptr,
                               grad_z + i0 * g->z_dim, loss ? loss + i0 : nullptr);
    }
    return rc;
}

// checks shared by the two entry points (those of gl_pggan_forward); *run says whether there is anything to do
int grad_enter(gl_pggan *g, int64_t n, int steps, const char *who, bool *run)
{
    *run = false;
    GL_REQUIRE(g && n >= 0 && steps >= 0 && steps <= kPgBlocks, "%s: bad argument (steps in [0,8])", who);
    if (!g->have_init) { gl_set_error("%s: initial block not loaded", who); return GL_ERR_STATE; }
    for (int s = 0; s < steps; ++s) {
        GL_REQUIRE(g->cin[s] % 32 == 0 && g->cout[s] % 32 == 0, "%s: block %d has %d -> %d channels; the K slices need multiples of 32", who, s, g->cin[s],
                   g->cout[s]);
        if (!g->have_blk[s]) { gl_set_error("%s: prog_blocks.%d not loaded", who, s); return GL_ERR_STATE; }
    }
    if (!g->have_rgb[steps] || (steps > 0 && !g->have_rgb[steps - 1])) {
        gl_set_error("%s: rgb_layers.%d/%d not loaded", who, steps, steps - 1);
        return GL_ERR_STATE;
    }
    *run = n > 0;
    return GL_OK;
}

}  // namespace

void gl_pggan_grad_free(gl_pggan *g)
{
    free_grad_workspace(g);
    for (int l = 0; l < kPgLayers; ++l) { (void)hipFree(g->gw[l]); g->gw[l] = nullptr; }
}

extern "C" {

int gl_pggan_vjp_z(gl_pggan *g, const float *z_dev, int64_t n, int steps, float alpha, const float *cot_dev, float *grad_z_dev, float *out_f32_dev)
{
    gl_make_current(g ? g->ctx : nullptr);
    bool run;
    const int rc = grad_enter(g, n, steps, "gl_pggan_vjp_z", &run);
    if (rc != GL_OK || !run) return rc;
    GL_REQUIRE(z_dev && cot_dev && grad_z_dev, "gl_pggan_vjp_z: NULL device pointer");
    return grad_passes(g, z_dev, n, steps, alpha, cot_dev, nullptr, grad_z_dev, out_f32_dev, nullptr);
}

int gl_pggan_l2_grad_z(gl_pggan *g, const float *z_dev, const uint8_t *target_u8_dev, int64_t n, int steps, float alpha, float *grad_z_dev, float *loss_dev)
{
    gl_make_current(g ? g->ctx : nullptr);
    bool run;
    const int rc = grad_enter(g, n, steps, "gl_pggan_l2_grad_z", &run);
    if (rc != GL_OK || !run) return rc;
    GL_REQUIRE(z_dev && target_u8_dev && grad_z_dev && loss_dev, "gl_pggan_l2_grad_z: NULL device pointer");
    return grad_passes(g, z_dev, n, steps, alpha, nullptr, target_u8_dev, grad_z_dev, nullptr, loss_dev);
}

}  // extern "C"

#ifdef GL_TUNING
// One launch of one kernel of this file on device buffers that gl_tune_grad_op (gl_tune.hip) has put between guards: through the launchers
// backward_pass uses.  ip[0] = images; fp[0]: the toRGB factor.  nb: the bytes of in[0 .. 3] and out[0 .. 1] (0 for a NULL slot); every buffer a
// kernel touches must have exactly the size its shape gives.
#define GL_TUNE_NEED(slot, bytes)                                                                                                              \
    GL_REQUIRE(nb[slot] == (int64_t)(bytes), "%s: buffer %d (inputs 0 - 3, outputs 4 - 5) has %lld bytes, the shape needs %lld", __func__, slot, \
               (long long)nb[slot], (long long)(bytes))
int gl_tune_pggan_grad_op(gl_ctx *ctx, int op, const int64_t *ip, const int64_t *nb, const float *fp, void *const *in, void *const *out)
{
    hipStream_t st = ctx->stream;
    const int64_t m = ip[0];
    GL_REQUIRE(m > 0 && m <= 4096, "gl_tune_pggan_grad_op: images in 1..4096");
    for (int k = 1; k <= 4; ++k) GL_REQUIRE(ip[k] >= 0 && ip[k] <= (1 << 20), "gl_tune_pggan_grad_op: argument %d out of range", k);
    switch (op) {
    case 0:   // pg_out_grad_kernel<false>: ip[1] = values per image, ip[2] = use_tanh; in = y, cot; out = g
        GL_REQUIRE(ip[1] > 0, "gl_tune_pggan_grad_op: bad shape");
        GL_TUNE_NEED(0, m * ip[1] * 4);
        GL_TUNE_NEED(1, m * ip[1] * 4);
        GL_TUNE_NEED(4, m * ip[1] * 4);
        launch_out_grad(st, (const float *)in[0], (const float *)in[1], nullptr, m, (int)ip[1], (int)ip[2], (float *)out[0], nullptr);
        break;
    case 1:   // pg_out_grad_kernel<true>: in = y, target codes; out = g, loss [m]
        GL_REQUIRE(ip[1] > 0, "gl_tune_pggan_grad_op: bad shape");
        GL_TUNE_NEED(0, m * ip[1] * 4);
        GL_TUNE_NEED(1, m * ip[1]);
        GL_TUNE_NEED(4, m * ip[1] * 4);
        GL_TUNE_NEED(5, m * 4);
        launch_out_grad(st, (const float *)in[0], nullptr, (const uint8_t *)in[1], m, (int)ip[1], (int)ip[2], (float *)out[0], (float *)out[1]);
        break;
    case 2: { // pg_rgb_grad_kernel: ip[1..4] = H (grid of dA), C, nc, pool; in = g [m][nc][R][R] (R = H, or 2 H with pool), w [nc][C]; out = dA [m][H][H][C]
        GL_REQUIRE(ip[1] > 0 && ip[2] > 0 && ip[3] > 0 && ip[3] <= 4, "gl_tune_pggan_grad_op: bad shape");
        const int64_t R = ip[4] ? 2 * ip[1] : ip[1];
        GL_TUNE_NEED(0, m * ip[3] * R * R * 4);
        GL_TUNE_NEED(1, ip[3] * ip[2] * 4);
        GL_TUNE_NEED(4, m * ip[1] * ip[1] * ip[2] * 4);
        launch_rgb_grad(st, (const float *)in[0], (const float *)in[1], m, (int)ip[1], (int)ip[2], (int)ip[3], (int)ip[4], fp[0], (float *)out[0]);
        break;
    }
    case 3: { // pg_pn_grad_kernel: ip[1..3] = H, C, pool; in = dA ([m][H][H][C], or on the 2H grid with pool), a, inv [m][H][H], extra or NULL; out = gpre chunks
        GL_REQUIRE(ip[1] > 0 && ip[2] > 0 && ip[2] % 32 == 0, "gl_tune_pggan_grad_op: bad shape");
        const int64_t bytes = m * ip[1] * ip[1] * ip[2] * 4;
        GL_TUNE_NEED(0, ip[3] ? 4 * bytes : bytes);
        GL_TUNE_NEED(1, bytes);
        GL_TUNE_NEED(2, m * ip[1] * ip[1] * 4);
        if (in[3]) GL_TUNE_NEED(3, bytes);
        GL_TUNE_NEED(4, bytes);
        launch_pn_grad(st, (const float *)in[0], (const float *)in[1], (const float *)in[2], (const float *)in[3], m, (int)ip[1], (int)ip[2], (int)ip[3],
                       (float *)out[0]);
        break;
    }
    case 4:   // pg_leaky_grad_kernel: ip[1] = K; in = dA, h [m][K]; out = [chunk][m][<= kGradK0]
        GL_REQUIRE(ip[1] > 0, "gl_tune_pggan_grad_op: bad shape");
        GL_TUNE_NEED(0, m * ip[1] * 4);
        GL_TUNE_NEED(1, m * ip[1] * 4);
        GL_TUNE_NEED(4, m * ip[1] * 4);
        launch_leaky_grad(st, (const float *)in[0], (const float *)in[1], m, (int)ip[1], (float *)out[0]);
        break;
    case 5:   // pg_rowpn_grad_kernel, in place on out (which the caller has filled with d zn): ip[1] = d; in = z [m][d]
        GL_REQUIRE(ip[1] > 0, "gl_tune_pggan_grad_op: bad shape");
        GL_TUNE_NEED(0, m * ip[1] * 4);
        GL_TUNE_NEED(4, m * ip[1] * 4);
        launch_rowpn_grad(st, (const float *)in[0], m, (int)ip[1], (float *)out[0]);
        break;
    default:
        gl_set_error("gl_tune_pggan_grad_op: unknown op %d", op);
        return GL_ERR_INVALID;
    }
    GL_LAUNCH_CHECK();
    return GL_OK;
}
#undef GL_TUNE_NEED
#endif
