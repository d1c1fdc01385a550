// Image gradient of the distance the l2-lpips attacks use:  loss(y, x) = 0.2 * LPIPS(y, x) + mean_k (y - x)^2  and  cot = d loss / d y,
// the white-box attack's loss under that distance (GAN-Leaks section 5.4; Loss('l2-lpips'), attack_models/utils.py:166-176, PNetLin.forward,
// attack_models/lpips_pytorch/models/networks_basic.py:134-181).  x = 2 u / 255 - 1 are the targets' 8-bit codes.
//
// A pass of m images first runs VGG16 with fp32 products in keep mode: the output of every convolution after its ReLU stays in a buffer of its
// own, NHWC, with the four 2 x 2 max-pools.  conv1_1 (K = 27) is a plain fp32 kernel here, the other twelve are the forward's fp32 tap-gather
// GEMM (gl_launch_gather_conv).  The targets' side enters only through their normalised tap values n^x ("reference rows",
// gl_lpips_ref_rows_u8): the targets do not move between the steps of a descent, so their forward runs once.  Backwards, from relu5_3 down:
//   tap gradient   r = sqrt(sum_c f^2), n = f / (r + 1e-10), dn_c = 0.4 w_c (n_c - n^x_c) / (H_l W_l),
//                  df = (dn - n (n . dn) r / (r + 1e-10)) / (r + 1e-10); where r == 0 the projection term is taken as 0 (torch gives NaN there)
//   pool           a position takes the pooled gradient if it is the first maximum of its 2 x 2 cell in row-major order (torch's rule)
//   ReLU           ... and passes what it has on where its kept activation is > 0
//                  -- the three are one kernel, one wave per full-resolution position: a gather, no atomics and no scatter --
//   dIn            = conv3x3(gpre) with the taps mirrored and the weight matrix transposed: gl_launch_gather_conv with C_in columns, one launch
//                  per 128 channels of gpre, added through the GEMM's residual in ascending order (kConvChunk: gl_pggan_grad.hip has the reason)
//   conv1_1        one wave per pixel: 9 taps x 64 channels down to the 3 image channels, divided by the input scale, NHWC -> NCHW, plus
//                  2 (y - x) / (3 H W)
// Every output element is one fixed-order fp32 sum (the loss: a double sum over fixed strides and a fixed tree), so a row of cot depends on
// its image alone -- not on n, the pass size or whether the caller handed the reference rows over.  The backward adds no matrix-core kernel.
#include "gl_lpips.h"
#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kConvChunk = 128;                    // channels of gpre per launch of a 3 x 3 data gradient (K = 1152)
constexpr uint64_t kKeepBytes = 4096ull << 20;     // default pass: kept activations of at most this many bytes (4.9 MB per 64 x 64 image)
constexpr float kEps = 1e-10f;                     // normalize_tensor's eps, added after the square root (util/util.py:72)

const int kCout[kLpNumConv] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
const int kCin[kLpNumConv] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
const int kAfter[kLpNumConv] = {0, 2, 0, 2, 0, 0, 2, 0, 0, 2, 0, 0, 1};      // 1 = LPIPS tap, 2 = tap then 2 x 2 max-pool
const int kTapC[kLpTaps] = {64, 128, 256, 512, 512};

__constant__ float g_shift[3] = {-.030f, -.088f, -.188f};   // networks_basic.py:115
__constant__ float g_scale[3] = {.458f, .448f, .450f};      // networks_basic.py:116

struct TapGeom { int64_t off[kLpTaps]; int hw[kLpTaps]; };  // position offset of every tap inside an image's per-position row, and its H_l W_l

__device__ __forceinline__ float pixel_of(float v) { return v; }
__device__ __forceinline__ float pixel_of(uint8_t c) { return (float)(2.0 * ((double)c / 255.0) - 1.0); }      // attack_models/utils.py:82

__device__ __forceinline__ float wave_sum(float s)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

// conv1_1 + ReLU straight from the image (NCHW, float or 8-bit codes): thread = (position, output channel), an fmaf chain from the bias over
// k = (ky * 3 + kx) * 3 + c.  w: the raw weights [64][3][3][3].  out: NHWC [positions][64].
template <typename T>
__global__ void __launch_bounds__(kThreads) lg_conv1_kernel(const T *__restrict__ img, int64_t positions, int H, int W, const float *__restrict__ w,
                                                            const float *__restrict__ bias, float *__restrict__ out)
{
    __shared__ float ws[27][64];
    for (int i = threadIdx.x; i < 27 * 64; i += kThreads) {
        const int co = i & 63, k = i >> 6, c = k % 3, t = k / 3;
        ws[k][co] = w[(co * 3 + c) * 9 + t];
    }
    __syncthreads();
    const int co = threadIdx.x & 63;
    const float b = bias[co];
    const int64_t HW = (int64_t)H * W;
    for (int64_t pos = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); pos < positions; pos += (int64_t)gridDim.x * 4) {
        const int64_t im = pos / HW;
        const int pin = (int)(pos - im * HW);
        const int y = pin / W, x = pin - y * W;
        float acc = b;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = __fdiv_rn(__fsub_rn(pixel_of(img[(im * 3 + c) * HW + (int64_t)yy * W + xx]), g_shift[c]), g_scale[c]);
                acc = fmaf(v, ws[t * 3 + c][co], acc);
            }
        }
        out[pos * 64 + co] = fmaxf(acc, 0.0f);
    }
}

// 2 x 2 / stride 2 max-pool, NHWC, C % 4 == 0
__global__ void __launch_bounds__(kThreads) lg_maxpool_kernel(const float *__restrict__ in, int64_t n, int H, int W, int C, float *__restrict__ out)
{
    const int Ho = H / 2, Wo = W / 2, C4 = C / 4;
    const int64_t total = n * Ho * Wo * C4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        int64_t r = i / C4;
        const int xo = (int)(r % Wo);
        r /= Wo;
        const int yo = (int)(r % Ho);
        const int64_t im = r / Ho;
        const float4 *p = reinterpret_cast<const float4 *>(in + (((im * H + 2 * yo) * W + 2 * xo) * (int64_t)C)) + c4;
        const float4 a = p[0], b = p[C4], c = p[(int64_t)W * C4], d = p[(int64_t)W * C4 + C4];
        float4 m;
        m.x = fmaxf(fmaxf(a.x, b.x), fmaxf(c.x, d.x));
        m.y = fmaxf(fmaxf(a.y, b.y), fmaxf(c.y, d.y));
        m.z = fmaxf(fmaxf(a.z, b.z), fmaxf(c.z, d.z));
        m.w = fmaxf(fmaxf(a.w, b.w), fmaxf(c.w, d.w));
        reinterpret_cast<float4 *>(out)[i] = m;
    }
}

// r + eps of a position whose lane holds channels lane, lane + 64, ...: one fmaf chain per lane, the xor butterfly 32 .. 1, a rounded root
template <int J>
__device__ __forceinline__ float tap_norm(const float (&f)[J], float *r_out)
{
    float ss = 0.0f;
#pragma unroll
    for (int j = 0; j < J; ++j) ss = fmaf(f[j], f[j], ss);
    const float r = gl_sqrt_rn(wave_sum(ss));
    *r_out = r;
    return __fadd_rn(r, kEps);
}

// reference rows: ref[img][off + pin * C + c] = f / (|f|_c + 1e-10), one wave per position (C = 64 J)
template <int J>
__global__ void __launch_bounds__(kThreads) lg_ref_kernel(const float *__restrict__ f, int64_t positions, int HW, float *__restrict__ ref, int64_t ref_ld,
                                                          int64_t off)
{
    constexpr int C = 64 * J;
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t pos = wave; pos < positions; pos += nwaves) {
        float v[J], r;
#pragma unroll
        for (int j = 0; j < J; ++j) v[j] = f[pos * C + lane + 64 * j];
        const float den = tap_norm<J>(v, &r);
        const int64_t im = pos / HW;
        float *dst = ref + im * ref_ld + off + (pos - im * HW) * C;
#pragma unroll
        for (int j = 0; j < J; ++j) dst[lane + 64 * j] = __fdiv_rn(v[j], den);
    }
}

// Gradient with respect to the input of one convolution's ReLU, one wave per position of its h x w grid (C = 64 J channels, a lane holds
// channels lane + 64 j).  a: the kept activation.  What arrives from above (mode): 0 nothing (relu5_3), 1 D[pos][c] on the same grid, 2 D on
// the pooled (h/2) x (w/2) grid -- taken by the first maximum of the 2 x 2 cell in row-major order.  With ref != NULL the layer is an LPIPS
// tap: its gradient (header) is added to what arrived, and part[img][part_off + pin] = sum_c w_c (n_c - n^x_c)^2 is the position's term of the
// loss.  out = (a > 0 ? g : 0), cut into chunks of kConvChunk channels: [chunk][pos][<= kConvChunk], the inputs of the data gradient's launches.
template <int J>
__global__ void __launch_bounds__(kThreads) lg_act_grad_kernel(const float *__restrict__ a, const float *__restrict__ D, int mode, int64_t positions, int h, int w,
                                                               const float *__restrict__ ref, int64_t ref_ld, int64_t ref_off, const float *__restrict__ lin,
                                                               float coef, float *__restrict__ part, int64_t part_ld, int64_t part_off,
                                                               float *__restrict__ out)
{
    constexpr int C = 64 * J;
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int hw = h * w;
    for (int64_t pos = wave; pos < positions; pos += nwaves) {
        const int64_t im = pos / hw;
        const int pin = (int)(pos - im * hw);
        float av[J], g[J];
#pragma unroll
        for (int j = 0; j < J; ++j) av[j] = a[pos * C + lane + 64 * j];
        if (mode == 1) {
#pragma unroll
            for (int j = 0; j < J; ++j) g[j] = D[pos * C + lane + 64 * j];
        } else if (mode == 2) {
            const int y = pin / w, x = pin - y * w;
            const int q = (y & 1) * 2 + (x & 1);
            const int64_t base = (im * h + (y & ~1)) * (int64_t)w + (x & ~1);
            const int64_t cell = (im * (h / 2) + (y >> 1)) * (int64_t)(w / 2) + (x >> 1);
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int c = lane + 64 * j;
                bool first = true;
#pragma unroll
                for (int qq = 0; qq < 4; ++qq) {
                    if (qq == q) continue;
                    const float o = a[(base + (qq >> 1) * w + (qq & 1)) * C + c];
                    first = first && (qq < q ? av[j] > o : av[j] >= o);
                }
                g[j] = first ? D[cell * C + c] : 0.0f;
            }
        } else {
#pragma unroll
            for (int j = 0; j < J; ++j) g[j] = 0.0f;
        }
        if (ref) {
            float r;
            const float den = tap_norm<J>(av, &r);
            const float *rp = ref + im * ref_ld + ref_off + (int64_t)pin * C;
            float nv[J], dn[J], sq = 0.0f, dot = 0.0f;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int c = lane + 64 * j;
                nv[j] = __fdiv_rn(av[j], den);
                const float diff = __fsub_rn(nv[j], rp[c]);
                const float wd = __fmul_rn(lin[c], diff);
                sq = fmaf(wd, diff, sq);
                dn[j] = __fmul_rn(coef, wd);
                dot = fmaf(nv[j], dn[j], dot);
            }
            sq = wave_sum(sq);
            dot = wave_sum(dot);
            const float proj = r > 0.0f ? __fmul_rn(dot, __fdiv_rn(r, den)) : 0.0f;
#pragma unroll
            for (int j = 0; j < J; ++j) g[j] = __fadd_rn(g[j], __fdiv_rn(__fsub_rn(dn[j], __fmul_rn(nv[j], proj)), den));
            if (lane == 0) part[im * part_ld + part_off + pin] = sq;
        }
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int c = lane + 64 * j;
            const int c0 = c & ~(kConvChunk - 1);
            const int cc = C - c0 < kConvChunk ? C - c0 : kConvChunk;
            out[(int64_t)c0 * positions + pos * cc + (c - c0)] = av[j] > 0.0f ? g[j] : 0.0f;
        }
    }
}

// conv1_1 backwards and the L2 term, one wave per pixel, lane = conv1_1's output channel:
//   s_c = sum over the 9 taps (ascending) and the 64 channels (butterfly) of gpre[pixel - tap offset][co] w[co][c][tap]
//   cot[img][c][pixel] = s_c / scale_c + 2 (y - x) / (3 H W)
template <typename T>
__global__ void __launch_bounds__(kThreads) lg_conv1_grad_kernel(const float *__restrict__ gpre, const float *__restrict__ w, const float *__restrict__ yimg,
                                                                 const T *__restrict__ target, int64_t positions, int H, int W, float two_over_d,
                                                                 float *__restrict__ cot)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t HW = (int64_t)H * W;
    float wr[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) wr[k] = w[lane * 27 + k];          // [co][c][ky][kx]
    for (int64_t pos = wave; pos < positions; pos += nwaves) {
        const int64_t im = pos / HW;
        const int pin = (int)(pos - im * HW);
        const int y = pin / W, x = pin - y * W;
        float s[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = y - (t / 3 - 1), xx = x - (t % 3 - 1);   // the output position that read this pixel through tap t
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
            const float gv = gpre[((im * H + yy) * (int64_t)W + xx) * 64 + lane];
#pragma unroll
            for (int c = 0; c < 3; ++c) s[c] = fmaf(gv, wr[c * 9 + t], s[c]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] = wave_sum(s[c]);
        if (lane < 3) {
            const float sc = lane == 0 ? s[0] : (lane == 1 ? s[1] : s[2]);
            const int64_t o = (im * 3 + lane) * HW + pin;
            const float diff = __fsub_rn(yimg[o], pixel_of(target[o]));
            cot[o] = __fadd_rn(__fdiv_rn(sc, g_scale[lane]), __fmul_rn(two_over_d, diff));
        }
    }
}

// loss[img] = sum_l 0.2 / (H_l W_l) sum_pos part_l[pos] + sum_k (y - x)^2 / D: one workgroup per image, doubles, per thread over its strided
// share and then down a fixed tree
template <typename T>
__global__ void __launch_bounds__(kThreads) lg_loss_kernel(const float *__restrict__ part, int64_t part_ld, TapGeom geom, const float *__restrict__ yimg,
                                                           const T *__restrict__ target, int64_t Dimg, float *__restrict__ loss)
{
    __shared__ double red[kThreads];
    const int64_t im = blockIdx.x;
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t < kLpTaps; ++t) {
        const float *p = part + im * part_ld + geom.off[t];
        double s = 0.0;
        for (int i = threadIdx.x; i < geom.hw[t]; i += kThreads) s += (double)p[i];
        acc += s * (0.2 / (double)geom.hw[t]);
    }
    double l2 = 0.0;
    for (int64_t i = threadIdx.x; i < Dimg; i += kThreads) {
        const float diff = __fsub_rn(yimg[im * Dimg + i], pixel_of(target[im * Dimg + i]));
        l2 += (double)diff * (double)diff;
    }
    red[threadIdx.x] = acc + l2 / (double)Dimg;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[im] = (float)red[0];
}

int cols_pad_of(int cols) { return cols % 128 == 0 ? cols : (int)gl_ceil_div(cols, 64) * 64; }

int upload(gl_ctx *ctx, float **dev, const std::vector<float> &host)
{
    (void)hipFree(*dev);
    *dev = nullptr;
    GL_HIP(gl_device_alloc(ctx, (void **)dev, host.size() * sizeof(float)));
    GL_HIP(hipMemcpyAsync(*dev, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    GL_HIP(hipStreamSynchronize(ctx->stream));
    return GL_OK;
}

// the transposed packs of every convolution, from the raw weights gl_lpips_set_conv kept on the host, and the lin weights
int pack_grad_weights(gl_lpips *l)
{
    if (!l->grad_dirty) return GL_OK;
    GL_HIP(hipStreamSynchronize(l->ctx->stream));          // an earlier gradient call may still read the packs this replaces
    int rc = upload(l->ctx, &l->gw[0], l->w_host[0]);
    for (int ci = 1; ci < kLpNumConv && rc == GL_OK; ++ci) {
        const int C = kCout[ci], cin = kCin[ci], K = 9 * C;
        const std::vector<float> &w = l->w_host[ci];       // [C_out][C_in][3][3]
        // [channel chunk of gpre][C_in -> cols_pad][9 taps x <= kConvChunk channels]
        const size_t cols_pad = (size_t)cols_pad_of(cin);
        std::vector<float> pk(cols_pad * K, 0.0f);
        for (int co = 0; co < C; ++co) {
            const int c0 = co & ~(kConvChunk - 1);
            const int cc = C - c0 < kConvChunk ? C - c0 : kConvChunk;
            for (int i = 0; i < cin; ++i)
                for (int t = 0; t < 9; ++t)
                    pk[(size_t)c0 * 9 * cols_pad + (size_t)i * 9 * cc + gl_conv_k_index(t, co - c0, 9)] = w[((size_t)co * cin + i) * 9 + (8 - t)];
        }
        rc = upload(l->ctx, &l->gw[ci], pk);
    }
    if (rc != GL_OK) return rc;
    l->grad_dirty = false;
    return GL_OK;
}

// the lin weights may change without the convolutions doing so (gl_lpips_set_lin): 1472 floats, compared on every call, uploaded when they differ
int upload_lin(gl_lpips *l)
{
    std::vector<float> lin;
    for (int t = 0; t < kLpTaps; ++t) lin.insert(lin.end(), l->lin_host[t].begin(), l->lin_host[t].end());
    if (l->g_lin && lin == l->g_lin_host) return GL_OK;
    GL_HIP(hipStreamSynchronize(l->ctx->stream));          // an earlier gradient call may still read the old values
    if (!l->g_lin) GL_HIP(gl_device_alloc(l->ctx, (void **)&l->g_lin, lin.size() * sizeof(float)));
    l->g_lin_host = lin;
    GL_HIP(hipMemcpyAsync(l->g_lin, l->g_lin_host.data(), lin.size() * sizeof(float), hipMemcpyHostToDevice, l->ctx->stream));
    GL_HIP(hipStreamSynchronize(l->ctx->stream));
    return GL_OK;
}

struct Geom {
    int h[kLpNumConv], w[kLpNumConv];      // the grid of every convolution
    TapGeom tap;                           // positions
    int64_t ref_off[kLpTaps], ref_dim;     // floats
    int64_t part_dim, kept;                // positions per image over the five taps; kept floats per image (activations and pools)
};

Geom geom_of(int H, int W)
{
    Geom g = {};
    int h = H, w = W, t = 0;
    for (int ci = 0; ci < kLpNumConv; ++ci) {
        g.h[ci] = h; g.w[ci] = w;
        g.kept += (int64_t)h * w * kCout[ci];
        if (kAfter[ci]) {
            g.tap.off[t] = g.part_dim; g.tap.hw[t] = h * w;
            g.ref_off[t] = g.ref_dim;
            g.part_dim += (int64_t)h * w;
            g.ref_dim += (int64_t)h * w * kTapC[t];
            ++t;
        }
        if (kAfter[ci] == 2) { h /= 2; w /= 2; g.kept += (int64_t)h * w * kCout[ci]; }
    }
    return g;
}

// images per pass: gl_lpips_set_chunk's value, else what keeps the kept activations under kKeepBytes; under the 3 GiB a buffer descriptor may span
int64_t pass_images(const gl_lpips *l, int H, int W)
{
    const Geom g = geom_of(H, W);
    int64_t want = l->chunk > 0 ? l->chunk : (int64_t)(kKeepBytes / ((uint64_t)g.kept * 4));
    const int64_t cap = (int64_t)(0xB0000000ull / ((uint64_t)H * W * 64 * 4));
    if (want > cap) want = cap;
    return want < 1 ? 1 : want;
}

void free_workspace(gl_lpips *l)
{
    for (int ci = 0; ci < kLpNumConv; ++ci) { (void)hipFree(l->keep[ci]); l->keep[ci] = nullptr; }
    float **all[] = {&l->keep_pool[0], &l->keep_pool[1], &l->keep_pool[2], &l->keep_pool[3], &l->g_roll[0], &l->g_roll[1], &l->g_part, &l->g_ref};
    for (float **p : all) { (void)hipFree(*p); *p = nullptr; }
    l->g_imgs = 0;
    l->g_H = l->g_W = 0;
}

int ensure_workspace(gl_lpips *l, int64_t n, int H, int W)
{
    int64_t want = pass_images(l, H, W);
    if (n < want) want = n;
    if (H == l->g_H && W == l->g_W && want <= l->g_imgs) return GL_OK;
    GL_HIP(hipStreamSynchronize(l->ctx->stream));
    free_workspace(l);
    const Geom g = geom_of(H, W);
    int pool = 0;
    for (int ci = 0; ci < kLpNumConv; ++ci) {
        GL_HIP(gl_device_alloc(l->ctx, (void **)&l->keep[ci], (size_t)want * g.h[ci] * g.w[ci] * kCout[ci] * 4));
        if (kAfter[ci] == 2) GL_HIP(gl_device_alloc(l->ctx, (void **)&l->keep_pool[pool++], (size_t)want * (g.h[ci] / 2) * (g.w[ci] / 2) * kCout[ci] * 4));
    }
    for (int k = 0; k < 2; ++k) GL_HIP(gl_device_alloc(l->ctx, (void **)&l->g_roll[k], (size_t)want * H * W * 64 * 4));      // the widest tensor: H x W x 64
    GL_HIP(gl_device_alloc(l->ctx, (void **)&l->g_part, (size_t)want * g.part_dim * 4));
    GL_HIP(gl_device_alloc(l->ctx, (void **)&l->g_ref, (size_t)want * g.ref_dim * 4));
    l->g_imgs = want; l->g_H = H; l->g_W = W;
    return GL_OK;
}

unsigned wave_blocks(int64_t positions)
{
    int64_t b = gl_ceil_div(positions, 4);
    return (unsigned)(b < 1 ? 1 : (b > 16384 ? 16384 : b));
}

// One launch of every kernel above, with its grid and its template instance: the passes below and the tuning build's single-launch hook
// (gl_tune_lpips_grad_op, at the end of this file) both go through these.
template <typename T>
void launch_conv1(hipStream_t st, const T *img, int64_t m, int H, int W, const float *w, const float *bias, float *out)
{
    hipLaunchKernelGGL(lg_conv1_kernel<T>, dim3(wave_blocks(m * H * W)), dim3(kThreads), 0, st, img, m * H * W, H, W, w, bias, out);
}

void launch_maxpool(hipStream_t st, const float *in, int64_t m, int h, int w, int C, float *out)
{
    const int64_t items = m * (h / 2) * (w / 2) * (C / 4);
    int64_t blocks = gl_ceil_div(items, kThreads);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(lg_maxpool_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, in, m, h, w, C, out);
}

void launch_ref(hipStream_t st, int C, const float *f, int64_t positions, int hw, float *ref, int64_t ref_ld, int64_t off)
{
    const dim3 grid(wave_blocks(positions)), block(kThreads);
    switch (C) {
    case 64: hipLaunchKernelGGL(lg_ref_kernel<1>, grid, block, 0, st, f, positions, hw, ref, ref_ld, off); break;
    case 128: hipLaunchKernelGGL(lg_ref_kernel<2>, grid, block, 0, st, f, positions, hw, ref, ref_ld, off); break;
    case 256: hipLaunchKernelGGL(lg_ref_kernel<4>, grid, block, 0, st, f, positions, hw, ref, ref_ld, off); break;
    default: hipLaunchKernelGGL(lg_ref_kernel<8>, grid, block, 0, st, f, positions, hw, ref, ref_ld, off); break;
    }
}

void launch_act_grad(hipStream_t st, int C, const float *a, const float *D, int mode, int64_t m, int h, int w, const float *ref, int64_t ref_ld, int64_t ref_off,
                     const float *lin, float *part, int64_t part_ld, int64_t part_off, float *out)
{
    const int64_t positions = m * h * w;
    const float coef = (float)(0.4 / ((double)h * w));
    const dim3 grid(wave_blocks(positions)), block(kThreads);
#define GL_ACT_GRAD(J) hipLaunchKernelGGL(lg_act_grad_kernel<J>, grid, block, 0, st, a, D, mode, positions, h, w, ref, ref_ld, ref_off, lin, coef, part, part_ld, \
                                          part_off, out)
    switch (C) {
    case 64: GL_ACT_GRAD(1); break;
    case 128: GL_ACT_GRAD(2); break;
    case 256: GL_ACT_GRAD(4); break;
    default: GL_ACT_GRAD(8); break;
    }
#undef GL_ACT_GRAD
}

void launch_conv1_grad(hipStream_t st, const float *gpre, const float *w, const float *y, const uint8_t *target, int64_t m, int H, int W, float *cot)
{
    const int64_t D = 3ll * H * W;
    hipLaunchKernelGGL(lg_conv1_grad_kernel<uint8_t>, dim3(wave_blocks(m * H * W)), dim3(kThreads), 0, st, gpre, w, y, target, m * H * W, H, W,
                       (float)(2.0 / (double)D), cot);
}

void launch_loss(hipStream_t st, const float *part, int64_t part_ld, const TapGeom &tap, const float *y, const uint8_t *target, int64_t m, int64_t D, float *loss)
{
    hipLaunchKernelGGL(lg_loss_kernel<uint8_t>, dim3((unsigned)m), dim3(kThreads), 0, st, part, part_ld, tap, y, target, D, loss);
}

// the keep-mode forward of m images: keep[ci] = relu(conv_ci), keep_pool[k] = the max-pool after taps 0 .. 3
template <typename T>
int forward_keep(gl_lpips *l, const T *img, int64_t m, int H, int W, const Geom &g)
{
    gl_ctx *ctx = l->ctx;
    launch_conv1<T>(ctx->stream, img, m, H, W, l->gw[0], l->bias[0], l->keep[0]);
    GL_LAUNCH_CHECK();
    const float *cur = l->keep[0];
    int pool = 0;
    uint32_t dy = 0, dx = 0;
    for (int t = 0; t < 9; ++t) { dy |= (uint32_t)(t / 3) << (2 * t); dx |= (uint32_t)(t % 3) << (2 * t); }
    for (int ci = 1; ci < kLpNumConv; ++ci) {
        const int h = g.h[ci], w = g.w[ci];
        GlGatherConv p = {};
        p.in = cur; p.positions = m * h * w; p.H = h; p.W = w; p.Cin = kCin[ci]; p.ntaps = 9;
        p.wpack = l->w[ci]; p.cols = kCout[ci]; p.cols_pad = kCout[ci];
        p.tap_dy[0] = dy; p.tap_dx[0] = dx;
        p.out = l->keep[ci]; p.Ho = h; p.Wo = w; p.omul = 1;
        p.scale = l->ones; p.shift = l->bias[ci]; p.cmod = kCout[ci]; p.act = 1; p.zero = ctx->zero_page;
        const int rc = gl_launch_gather_conv(ctx, p, 1);
        if (rc != GL_OK) return rc;
        cur = l->keep[ci];
        if (kAfter[ci] == 2) {
            launch_maxpool(ctx->stream, cur, m, h, w, kCout[ci], l->keep_pool[pool]);
            GL_LAUNCH_CHECK();
            cur = l->keep_pool[pool++];
        }
    }
    return GL_OK;
}

// reference rows of the m images whose activations the keep buffers hold
int ref_rows(gl_lpips *l, int64_t m, const Geom &g, float *ref)
{
    hipStream_t st = l->ctx->stream;
    int t = 0;
    for (int ci = 0; ci < kLpNumConv; ++ci) {
        if (!kAfter[ci]) continue;
        const int hw = g.h[ci] * g.w[ci];
        launch_ref(st, kCout[ci], l->keep[ci], m * hw, hw, ref, g.ref_dim, g.ref_off[t]);
        GL_LAUNCH_CHECK();
        ++t;
    }
    return GL_OK;
}

int conv_bwd(gl_lpips *l, int ci, int64_t m, const Geom &g, const float *gpre, float *out)
{
    const int C = kCout[ci], cin = kCin[ci], h = g.h[ci], w = g.w[ci];
    const int64_t positions = m * h * w;
    const int cols_pad = cols_pad_of(cin);
    uint32_t dy = 0, dx = 0;
    for (int t = 0; t < 9; ++t) { dy |= (uint32_t)(t / 3) << (2 * t); dx |= (uint32_t)(t % 3) << (2 * t); }
    for (int c0 = 0; c0 < C; c0 += kConvChunk) {
        GlGatherConv p = {};
        p.in = gpre + (int64_t)c0 * positions; p.positions = positions; p.H = h; p.W = w; p.up = 0;
        p.Cin = C - c0 < kConvChunk ? C - c0 : kConvChunk;
        p.wpack = l->gw[ci] + (int64_t)c0 * 9 * cols_pad; p.cols = cin; p.cols_pad = cols_pad; p.ntaps = 9;
        p.tap_dy[0] = dy; p.tap_dx[0] = dx;
        p.out = out; p.Ho = h; p.Wo = w; p.omul = 1;
        p.scale = l->ones; p.shift = l->ctx->zero_page; p.cmod = 1; p.act = 0; p.zero = l->ctx->zero_page;
        p.residual = c0 ? out : nullptr;
        const int rc = gl_launch_gather_conv(l->ctx, p, 1);
        if (rc != GL_OK) return rc;
    }
    return GL_OK;
}

// the backward of one pass: the keep buffers hold the activations of y's m images, ref their targets' reference rows
int backward_pass(gl_lpips *l, int64_t m, int H, int W, const Geom &g, const float *y, const uint8_t *target, const float *ref, float *cot, float *loss)
{
    hipStream_t st = l->ctx->stream;
    float *A = l->g_roll[0], *B = l->g_roll[1];      // A: the gradient arriving at a layer's output, B: gpre, the data gradient's input
    int t = kLpTaps - 1, lin_off = 64 + 128 + 256 + 512;
    for (int ci = kLpNumConv - 1; ci >= 0; --ci) {
        const int h = g.h[ci], w = g.w[ci], C = kCout[ci];
        const int mode = ci == kLpNumConv - 1 ? 0 : (kAfter[ci] == 2 ? 2 : 1);
        const bool tap = kAfter[ci] != 0;
        const float *rp = tap ? ref : nullptr;
        const int64_t ro = tap ? g.ref_off[t] : 0, po = tap ? g.tap.off[t] : 0;
        const float *lin = l->g_lin + (tap ? lin_off : 0);
        launch_act_grad(st, C, l->keep[ci], A, mode, m, h, w, rp, g.ref_dim, ro, lin, l->g_part, g.part_dim, po, B);
        GL_LAUNCH_CHECK();
        if (tap) { --t; if (t >= 0) lin_off -= kTapC[t]; }
        if (ci == 0) break;
        const int rc = conv_bwd(l, ci, m, g, B, A);
        if (rc != GL_OK) return rc;
    }
    const int64_t D = 3ll * H * W;
    launch_conv1_grad(st, B, l->gw[0], y, target, m, H, W, cot);
    GL_LAUNCH_CHECK();
    launch_loss(st, l->g_part, g.part_dim, g.tap, y, target, m, D, loss);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

// checks shared by the two entry points (those of the forward); *run says whether there is anything to do
int grad_enter(gl_lpips *l, int64_t n, int H, int W, const char *who, bool *run)
{
    *run = false;
    GL_REQUIRE(l && n >= 0, "%s: bad argument", who);
    GL_REQUIRE(H >= 16 && W >= 16 && H % 16 == 0 && W % 16 == 0, "%s: H, W must be multiples of 16 (four 2x2 pools), got %dx%d", who, H, W);
    for (int i = 0; i < kLpNumConv; ++i)
        if (!l->have_w[i]) { gl_set_error("%s: VGG16 conv %d not loaded", who, i); return GL_ERR_STATE; }
    for (int i = 0; i < kLpTaps; ++i)
        if (!l->have_lin[i]) { gl_set_error("%s: lin%d not loaded", who, i); return GL_ERR_STATE; }
    *run = n > 0;
    return GL_OK;
}

}  // namespace

void gl_lpips_grad_free(gl_lpips *l)
{
    free_workspace(l);
    for (int ci = 0; ci < kLpNumConv; ++ci) { (void)hipFree(l->gw[ci]); l->gw[ci] = nullptr; }
    (void)hipFree(l->g_lin);
    l->g_lin = nullptr;
    l->g_lin_host.clear();
    l->grad_dirty = true;
}

extern "C" {

int64_t gl_lpips_ref_dim(int H, int W)
{
    if (H < 16 || W < 16 || H % 16 || W % 16) return -1;
    return geom_of(H, W).ref_dim;
}

int gl_lpips_ref_rows_u8(gl_lpips *l, const uint8_t *target_u8_dev, int64_t n, int H, int W, float *ref_dev)
{
    gl_make_current(l ? l->ctx : nullptr);
    bool run;
    int rc = grad_enter(l, n, H, W, "gl_lpips_ref_rows_u8", &run);
    if (rc != GL_OK || !run) return rc;
    GL_REQUIRE(target_u8_dev && ref_dev, "gl_lpips_ref_rows_u8: NULL device pointer");
    rc = pack_grad_weights(l);
    if (rc == GL_OK) rc = ensure_workspace(l, n, H, W);
    if (rc != GL_OK) return rc;
    const Geom g = geom_of(H, W);
    const int64_t per = pass_images(l, H, W) < l->g_imgs ? pass_images(l, H, W) : l->g_imgs, D = 3ll * H * W;
    for (int64_t i0 = 0; i0 < n && rc == GL_OK; i0 += per) {
        const int64_t m = n - i0 < per ? n - i0 : per;
        rc = forward_keep<uint8_t>(l, target_u8_dev + i0 * D, m, H, W, g);
        if (rc == GL_OK) rc = ref_rows(l, m, g, ref_dev + i0 * g.ref_dim);
    }
    return rc;
}

int gl_lpips_grad_image(gl_lpips *l, const float *y_f32_dev, const uint8_t *target_u8_dev, const float *ref_dev, int64_t n, int H, int W, float *cot_dev,
                        float *loss_dev)
{
    gl_make_current(l ? l->ctx : nullptr);
    bool run;
    int rc = grad_enter(l, n, H, W, "gl_lpips_grad_image", &run);
    if (rc != GL_OK || !run) return rc;
    GL_REQUIRE(y_f32_dev && target_u8_dev && cot_dev && loss_dev, "gl_lpips_grad_image: NULL device pointer");
    rc = pack_grad_weights(l);
    if (rc == GL_OK) rc = upload_lin(l);
    if (rc == GL_OK) rc = ensure_workspace(l, n, H, W);
    if (rc != GL_OK) return rc;
    const Geom g = geom_of(H, W);
    const int64_t per = pass_images(l, H, W) < l->g_imgs ? pass_images(l, H, W) : l->g_imgs, D = 3ll * H * W;
    for (int64_t i0 = 0; i0 < n && rc == GL_OK; i0 += per) {
        const int64_t m = n - i0 < per ? n - i0 : per;
        const float *ref = ref_dev ? ref_dev + i0 * g.ref_dim : l->g_ref;
        if (!ref_dev) {
            rc = forward_keep<uint8_t>(l, target_u8_dev + i0 * D, m, H, W, g);
            if (rc == GL_OK) rc = ref_rows(l, m, g, l->g_ref);
        }
        if (rc == GL_OK) rc = forward_keep<float>(l, y_f32_dev + i0 * D, m, H, W, g);
        if (rc == GL_OK) rc = backward_pass(l, m, H, W, g, y_f32_dev + i0 * D, target_u8_dev + i0 * D, ref, cot_dev + i0 * D, loss_dev + i0);
    }
    return rc;
}

}  // extern "C"

#ifdef GL_TUNING
// One launch of one kernel of this file on device buffers that gl_tune_grad_op (gl_tune.hip) has put between guards: through the launchers the
// passes use.  ip: the integer arguments in the order given per op; a NULL in[] slot reaches the kernel as NULL (D without mode, ref without a tap).
// nb: the bytes of in[0 .. 3] and out[0 .. 1] (0 for a NULL slot); every buffer a kernel touches must have exactly the size its shape gives.
#define GL_TUNE_NEED(slot, bytes)                                                                                                              \
    GL_REQUIRE(nb[slot] == (int64_t)(bytes), "%s: buffer %d (inputs 0 - 3, outputs 4 - 5) has %lld bytes, the shape needs %lld", __func__, slot, \
               (long long)nb[slot], (long long)(bytes))
int gl_tune_lpips_grad_op(gl_ctx *ctx, int op, const int64_t *ip, const int64_t *nb, void *const *in, void *const *out)
{
    hipStream_t st = ctx->stream;
    const int64_t m = ip[0];
    const int H = (int)ip[1], W = (int)ip[2], C = (int)ip[3];
    GL_REQUIRE(m > 0 && m <= 4096 && ip[1] > 0 && ip[1] <= (1 << 20) && ip[2] > 0 && ip[2] <= (1 << 20) && ip[3] >= 0 && ip[3] <= 512,
               "gl_tune_lpips_grad_op: bad shape");
    const int64_t hw = (int64_t)H * W;
    const bool jwidth = C == 64 || C == 128 || C == 256 || C == 512;
    switch (op) {
    case 0:   // lg_conv1_kernel<float>: in = img [m][3][H][W], w [64][3][3][3], bias [64]; out = [m H W][64]
    case 1:   // lg_conv1_kernel<uint8_t>
        GL_TUNE_NEED(0, m * 3 * hw * (op == 0 ? 4 : 1));
        GL_TUNE_NEED(1, 64 * 27 * 4);
        GL_TUNE_NEED(2, 64 * 4);
        GL_TUNE_NEED(4, m * hw * 64 * 4);
        if (op == 0) launch_conv1<float>(st, (const float *)in[0], m, H, W, (const float *)in[1], (const float *)in[2], (float *)out[0]);
        else launch_conv1<uint8_t>(st, (const uint8_t *)in[0], m, H, W, (const float *)in[1], (const float *)in[2], (float *)out[0]);
        break;
    case 2:   // lg_maxpool_kernel: in = [m][H][W][C]; out = [m][H/2][W/2][C]
        GL_REQUIRE(H % 2 == 0 && W % 2 == 0 && C > 0 && C % 4 == 0, "gl_tune_lpips_grad_op: max-pool needs even H, W and C %% 4 == 0");
        GL_TUNE_NEED(0, m * hw * C * 4);
        GL_TUNE_NEED(4, m * (hw / 4) * C * 4);
        launch_maxpool(st, (const float *)in[0], m, H, W, C, (float *)out[0]);
        break;
    case 3:   // lg_ref_kernel<C / 64>: in = f [m H W][C]; out = ref [m][ip[4]] written from ip[5] on
        GL_REQUIRE(jwidth, "gl_tune_lpips_grad_op: C must be 64, 128, 256 or 512");
        GL_REQUIRE(ip[5] >= 0 && ip[5] + hw * C <= ip[4], "gl_tune_lpips_grad_op: reference rows too short");
        GL_TUNE_NEED(0, m * hw * C * 4);
        GL_TUNE_NEED(4, m * ip[4] * 4);
        launch_ref(st, C, (const float *)in[0], m * hw, (int)hw, (float *)out[0], ip[4], ip[5]);
        break;
    case 4: { // lg_act_grad_kernel<C / 64>: in = a, D, ref [m][ip[5]] (tap values from ip[6] on), lin [C]; out = gpre chunks, part [m][ip[7]] (from ip[8] on)
        const int mode = (int)ip[4];
        GL_REQUIRE(jwidth, "gl_tune_lpips_grad_op: C must be 64, 128, 256 or 512");
        GL_REQUIRE(mode >= 0 && mode <= 2 && (mode != 2 || (H % 2 == 0 && W % 2 == 0)), "gl_tune_lpips_grad_op: bad mode");
        GL_TUNE_NEED(0, m * hw * C * 4);
        GL_TUNE_NEED(1, mode == 0 ? 0 : (mode == 1 ? m * hw * C * 4 : m * (hw / 4) * C * 4));
        GL_TUNE_NEED(4, m * hw * C * 4);
        if (in[2]) {
            GL_REQUIRE(ip[6] >= 0 && ip[6] + hw * C <= ip[5] && ip[8] >= 0 && ip[8] + hw <= ip[7], "gl_tune_lpips_grad_op: tap rows too short");
            GL_TUNE_NEED(2, m * ip[5] * 4);
            GL_TUNE_NEED(3, C * 4);
            GL_TUNE_NEED(5, m * ip[7] * 4);
        }
        launch_act_grad(st, C, (const float *)in[0], (const float *)in[1], mode, m, H, W, (const float *)in[2], ip[5], ip[6], (const float *)in[3],
                        (float *)out[1], ip[7], ip[8], (float *)out[0]);
        break;
    }
    case 5:   // lg_conv1_grad_kernel<uint8_t>: in = gpre [m H W][64], w [64][3][3][3], y [m][3][H][W], target codes; out = cot [m][3][H][W]
        GL_TUNE_NEED(0, m * hw * 64 * 4);
        GL_TUNE_NEED(1, 64 * 27 * 4);
        GL_TUNE_NEED(2, m * 3 * hw * 4);
        GL_TUNE_NEED(3, m * 3 * hw);
        GL_TUNE_NEED(4, m * 3 * hw * 4);
        launch_conv1_grad(st, (const float *)in[0], (const float *)in[1], (const float *)in[2], (const uint8_t *)in[3], m, H, W, (float *)out[0]);
        break;
    case 6: { // lg_loss_kernel<uint8_t>: ip[1] = values per image, ip[2] = part_ld, ip[4 + t] = hw of tap t (offsets: their running sum);
              // in = part [m][part_ld], y [m][ip[1]], target codes; out = loss [m]
        TapGeom tg = {};
        int64_t off = 0;
        for (int t = 0; t < kLpTaps; ++t) {
            GL_REQUIRE(ip[4 + t] > 0 && ip[4 + t] <= (1 << 24), "gl_tune_lpips_grad_op: bad tap size");
            tg.off[t] = off; tg.hw[t] = (int)ip[4 + t];
            off += ip[4 + t];
        }
        GL_REQUIRE(off <= ip[2], "gl_tune_lpips_grad_op: part rows too short");
        GL_TUNE_NEED(0, m * ip[2] * 4);
        GL_TUNE_NEED(1, m * ip[1] * 4);
        GL_TUNE_NEED(2, m * ip[1]);
        GL_TUNE_NEED(4, m * 4);
        launch_loss(st, (const float *)in[0], ip[2], tg, (const float *)in[1], (const uint8_t *)in[2], m, ip[1], (float *)out[0]);
        break;
    }
    default:
        gl_set_error("gl_tune_lpips_grad_op: unknown op %d", op);
        return GL_ERR_INVALID;
    }
    GL_LAUNCH_CHECK();
    return GL_OK;
}
#undef GL_TUNE_NEED
#endif
