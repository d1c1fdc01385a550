// The VAEGAN encoder behind the C ABI (reference: gan_models/vaegan/train.py:61-96, `Encoder.encode`), for inference:
//   h1..h4 = ReLU(BatchNorm2d(Conv2d(k4, s2, p1)))      3 -> 64 -> 128 -> 256 -> 512 channels, 64 x 64 -> 4 x 4
//   z_mu   = fc1_1(ReLU(BatchNorm1d(fc1(flatten h4))))  8192 -> 4 z -> z        (head 0)
//   z_var  = fc2_1(ReLU(BatchNorm1d(fc2(flatten h4))))                          (head 1)
// Every layer is ONE launch of one kernel, enc_gemm_kernel: C[M][N] = act(scale[n] * sum_k A(m, k) B[k][n] + shift[n]) with the operand
// A gathered on the fly.  Activations are NHWC, so the output [images * Ho * Wo][Co] of a layer IS the row-major C and the input of the
// next gather; a convolution row m = (image, oy, ox) reads k = (ky * 4 + kx) * Ci + ci at pixel (2 oy - 1 + ky, 2 ox - 1 + kx), zero outside
// the image (padding = 1 pads the layer's INPUT with zeros: post-ReLU activations, or image values in [-1, 1]).  The first layer gathers
// straight from the NCHW image, bytes or floats (K = 48); a byte u is read as fl32(2 * (u / 255.) - 1) with the expression in float64, the
// codec's lattice.  BatchNorm (eval, eps 1e-5) and the bias fold into scale / shift on the host in double.  ChannelsToLinear flattens NCHW (c * 16 + y * 4 + x);
// h4 here is (y * 4 + x) * 512 + c, so the rows of fc1 / fc2 are permuted on the host when they are packed.
// Arithmetic: fp32 products and sums on the vector unit.  An output is one sum over k in ascending chunks of 16, ascending inside a chunk,
// by one thread: it depends on its own row of A alone, not on the images that share the launch or the pass.  No atomics, no split K.
#include "gl_common.h"
#include <cmath>
#include <vector>

struct gl_vaegan_enc {
    gl_ctx *ctx;
    int z_dim;
    float *w[4], *scale[4], *shift[4];                           // convolutions: packed [16 Ci][Co], folded BatchNorm
    float *fc_w[2], *fc_scale[2], *fc_shift[2];                  // heads: fc [8192][4 z] (rows permuted to NHWC), folded BatchNorm1d
    float *out_w[2], *out_b[2];                                  //        fc*_1 [4 z][z], bias
    bool have_conv[4], have_head[2];
    int64_t chunk;                                               // images per pass
    int64_t ws_images;
    float *ws_a, *ws_b, *ws_h;                                   // h1 / h3, h2 / h4, the hidden rows of one head
};

namespace {

constexpr int kThreads = 256;
constexpr int TM = 64, TN = 64, TK = 16;                         // a workgroup's tile of C, and the chunk of k
constexpr int A_LD = TM + 4;                                     // 16-byte aligned rows, off the power of two
constexpr int ENC_CHANS[5] = {3, 64, 128, 256, 512};
constexpr int ENC_FLAT = 512 * 4 * 4;
constexpr int64_t ENC_DEFAULT_CHUNK = 512;                       // 384 KiB of activations per image

enum { A_NHWC = 0, A_IMAGE_F32 = 1, A_IMAGE_U8 = 2, A_DENSE = 3 };

// the value of an image element as the codec reads bytes (gl_codec.hip's table): the float64 expression 2 * (u / 255.) - 1 the reference
// evaluates (attack_models/utils.py:82), rounded to float32 -- the lattice prepare_images accepts floats on
__device__ __forceinline__ float enc_decode(uint8_t u) { return (float)(2.0 * ((double)u / 255.0) - 1.0); }

// C[m][n] = act(scale[n] * sum_k A(m, k) B[k][n] + shift[n]); scale == nullptr: 1.  B [K][N] row-major.
//   A_DENSE: A [M][K] row-major, K % 4 == 0.            A_NHWC: activations [images][H][H][Ci], Ci % 4 == 0, K = 16 Ci.
//   A_IMAGE_*: images [images][3][H][H], K = 48.
// 256 threads, thread (ty, tx) = (tid / 16, tid % 16) owns rows ty * 4 .. + 3 and columns tx * 4 .. + 3 of the 64 x 64 tile.
template <int KIND>
__global__ void __launch_bounds__(kThreads) enc_gemm_kernel(const void *__restrict__ A, const float *__restrict__ B, const float *__restrict__ scale,
                                                            const float *__restrict__ shift, float *__restrict__ C, int64_t M, int N, int K, int Ci,
                                                            int H, int relu)
{
    __shared__ __attribute__((aligned(16))) float As[TK][A_LD];
    __shared__ __attribute__((aligned(16))) float Bs[TK][TN];
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    const int64_t m0 = (int64_t)blockIdx.x * TM;
    const int n0 = blockIdx.y * TN;

    // the row of A this thread stages: fixed for the whole loop
    const int ar = (KIND == A_NHWC || KIND == A_DENSE) ? tid >> 2 : tid & 63;
    const int ak = (KIND == A_NHWC || KIND == A_DENSE) ? (tid & 3) * 4 : tid >> 6;
    const int64_t am = m0 + ar;
    const bool a_row = am < M;
    const int Ho = H >> 1;
    int64_t img = 0;
    int iy0 = 0, ix0 = 0;
    if (KIND != A_DENSE && a_row) {
        img = am / (Ho * Ho);
        const int rem = (int)(am - img * (Ho * Ho));
        iy0 = 2 * (rem / Ho) - 1;
        ix0 = 2 * (rem % Ho) - 1;
    }
    const int bc = tid & 63, bk = tid >> 6;                      // the column and first row of B this thread stages
    const bool b_col = n0 + bc < N;

    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;

    for (int k0 = 0; k0 < K; k0 += TK) {
        if (KIND == A_NHWC || KIND == A_DENSE) {
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            const int k = k0 + ak;
            if (a_row && k < K) {
                if (KIND == A_DENSE) {
                    v = *reinterpret_cast<const float4 *>(static_cast<const float *>(A) + am * K + k);
                } else {
                    const int tap = k / Ci, ci = k - tap * Ci;   // Ci % 4 == 0: the four values share the tap
                    const int iy = iy0 + (tap >> 2), ix = ix0 + (tap & 3);
                    if (iy >= 0 && iy < H && ix >= 0 && ix < H)
                        v = *reinterpret_cast<const float4 *>(static_cast<const float *>(A) + ((img * H + iy) * H + ix) * Ci + ci);
                }
            }
            As[ak + 0][ar] = v.x; As[ak + 1][ar] = v.y; As[ak + 2][ar] = v.z; As[ak + 3][ar] = v.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int kk = ak + 4 * i, k = k0 + kk;
                float v = 0.0f;
                if (a_row && k < K) {
                    const int tap = k / 3, ci = k - tap * 3;
                    const int iy = iy0 + (tap >> 2), ix = ix0 + (tap & 3);
                    if (iy >= 0 && iy < H && ix >= 0 && ix < H) {
                        const int64_t at = ((img * 3 + ci) * H + iy) * H + ix;
                        v = KIND == A_IMAGE_U8 ? enc_decode(static_cast<const uint8_t *>(A)[at]) : static_cast<const float *>(A)[at];
                    }
                }
                As[kk][ar] = v;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int kk = bk + 4 * i, k = k0 + kk;
            Bs[kk][bc] = (b_col && k < K) ? B[(int64_t)k * N + n0 + bc] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < TK; ++kk) {
            const float4 a = *reinterpret_cast<const float4 *>(&As[kk][ty * 4]);
            const float4 b = *reinterpret_cast<const float4 *>(&Bs[kk][tx * 4]);
            const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
        }
        __syncthreads();                                         // the chunk has been read by every wave before it is overwritten
    }

#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t m = m0 + ty * 4 + i;
        if (m >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + tx * 4 + j;
            if (n >= N) continue;
            float v = acc[i][j];
            if (scale) v *= scale[n];
            v += shift[n];
            if (relu) v = fmaxf(v, 0.0f);
            C[m * N + n] = v;
        }
    }
}

int enc_launch(gl_ctx *ctx, int kind, const void *A, const float *B, const float *scale, const float *shift, float *C, int64_t M, int N, int K, int Ci,
               int H, int relu)
{
    const dim3 grid((unsigned)gl_ceil_div(M, TM), (unsigned)gl_ceil_div(N, TN));
    switch (kind) {
    case A_NHWC: hipLaunchKernelGGL(enc_gemm_kernel<A_NHWC>, grid, dim3(kThreads), 0, ctx->stream, A, B, scale, shift, C, M, N, K, Ci, H, relu); break;
    case A_IMAGE_F32: hipLaunchKernelGGL(enc_gemm_kernel<A_IMAGE_F32>, grid, dim3(kThreads), 0, ctx->stream, A, B, scale, shift, C, M, N, K, Ci, H, relu); break;
    case A_IMAGE_U8: hipLaunchKernelGGL(enc_gemm_kernel<A_IMAGE_U8>, grid, dim3(kThreads), 0, ctx->stream, A, B, scale, shift, C, M, N, K, Ci, H, relu); break;
    default: hipLaunchKernelGGL(enc_gemm_kernel<A_DENSE>, grid, dim3(kThreads), 0, ctx->stream, A, B, scale, shift, C, M, N, K, Ci, H, relu); break;
    }
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int enc_upload(gl_ctx *ctx, float **dev, const std::vector<float> &host)
{
    if (*dev) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(*dev); *dev = nullptr; }
    GL_HIP(hipMalloc((void **)dev, host.size() * sizeof(float)));
    GL_HIP(hipMemcpyAsync(*dev, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    GL_HIP(hipStreamSynchronize(ctx->stream));
    return GL_OK;
}

// BatchNorm(eval, eps 1e-5) after a layer with bias b: y = s (x + b - mean) + beta, s = gamma / sqrt(var + eps), in double
void enc_fold(const float *b, const float *gamma, const float *beta, const float *mean, const float *var, int n, std::vector<float> &sc,
              std::vector<float> &sh)
{
    sc.resize(n); sh.resize(n);
    for (int i = 0; i < n; ++i) {
        const double s = (double)gamma[i] / std::sqrt((double)var[i] + 1e-5);
        sc[i] = (float)s;
        sh[i] = (float)(((double)b[i] - (double)mean[i]) * s + (double)beta[i]);
    }
}

const char *enc_missing(const gl_vaegan_enc *e)
{
    static const char *conv[4] = {"cv1 / bn1 (gl_vaegan_enc_set_conv layer 0)", "cv2 / bn2 (gl_vaegan_enc_set_conv layer 1)",
                                  "cv3 / bn3 (gl_vaegan_enc_set_conv layer 2)", "cv4 / bn4 (gl_vaegan_enc_set_conv layer 3)"};
    static const char *head[2] = {"fc1 / bn6 / fc1_1 (gl_vaegan_enc_set_head head 0)", "fc2 / bn7 / fc2_1 (gl_vaegan_enc_set_head head 1)"};
    for (int l = 0; l < 4; ++l)
        if (!e->have_conv[l]) return conv[l];
    for (int h = 0; h < 2; ++h)
        if (!e->have_head[h]) return head[h];
    return nullptr;
}

}  // namespace

extern "C" {

int gl_vaegan_enc_create(gl_ctx *ctx, int z_dim, int d, gl_vaegan_enc **out)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx && out, "gl_vaegan_enc_create: NULL argument");
    GL_REQUIRE(d == 64, "gl_vaegan_enc_create: d must be 64, got %d: the reference hard-wires 512 * 4 * 4 inputs to the encoder's heads "
               "(gan_models/vaegan/train.py:79,83), so no other width loads", d);
    GL_REQUIRE(z_dim >= 1 && z_dim <= 4096, "gl_vaegan_enc_create: z_dim must be in 1..4096, got %d", z_dim);
    gl_vaegan_enc *e = new gl_vaegan_enc();
    e->ctx = ctx; e->z_dim = z_dim;
    for (int l = 0; l < 4; ++l) { e->w[l] = e->scale[l] = e->shift[l] = nullptr; e->have_conv[l] = false; }
    for (int h = 0; h < 2; ++h) { e->fc_w[h] = e->fc_scale[h] = e->fc_shift[h] = e->out_w[h] = e->out_b[h] = nullptr; e->have_head[h] = false; }
    e->chunk = ENC_DEFAULT_CHUNK; e->ws_images = 0; e->ws_a = e->ws_b = e->ws_h = nullptr;
    *out = e;
    return GL_OK;
}

int gl_vaegan_enc_destroy(gl_vaegan_enc *e)
{
    gl_make_current(e ? e->ctx : nullptr);
    if (!e) return GL_OK;
    (void)hipStreamSynchronize(e->ctx->stream);
    for (int l = 0; l < 4; ++l) { (void)hipFree(e->w[l]); (void)hipFree(e->scale[l]); (void)hipFree(e->shift[l]); }
    for (int h = 0; h < 2; ++h) {
        (void)hipFree(e->fc_w[h]); (void)hipFree(e->fc_scale[h]); (void)hipFree(e->fc_shift[h]); (void)hipFree(e->out_w[h]); (void)hipFree(e->out_b[h]);
    }
    (void)hipFree(e->ws_a); (void)hipFree(e->ws_b); (void)hipFree(e->ws_h);
    delete e;
    return GL_OK;
}

int gl_vaegan_enc_set_chunk(gl_vaegan_enc *e, int64_t images_per_pass)
{
    GL_REQUIRE(e, "gl_vaegan_enc_set_chunk: NULL handle");
    GL_REQUIRE(images_per_pass >= 0 && images_per_pass <= (1 << 20), "gl_vaegan_enc_set_chunk: images_per_pass must be in 0..2^20 (0 = the default)");
    e->chunk = images_per_pass ? images_per_pass : ENC_DEFAULT_CHUNK;
    return GL_OK;
}

int gl_vaegan_enc_set_conv(gl_vaegan_enc *e, int layer, const float *w, const float *bias, const float *bn_weight, const float *bn_bias,
                           const float *bn_running_mean, const float *bn_running_var)
{
    gl_make_current(e ? e->ctx : nullptr);
    GL_REQUIRE(e && layer >= 0 && layer < 4 && w && bias && bn_weight && bn_bias && bn_running_mean && bn_running_var,
               "gl_vaegan_enc_set_conv: bad argument (layer 0..3, no NULL pointer)");
    const int Ci = ENC_CHANS[layer], Co = ENC_CHANS[layer + 1];
    // [Co][Ci][ky][kx] -> [(ky * 4 + kx) * Ci + ci][Co]
    std::vector<float> pk((size_t)16 * Ci * Co);
    for (int co = 0; co < Co; ++co)
        for (int ci = 0; ci < Ci; ++ci)
            for (int t = 0; t < 16; ++t) pk[((size_t)t * Ci + ci) * Co + co] = w[((size_t)co * Ci + ci) * 16 + t];
    std::vector<float> sc, sh;
    enc_fold(bias, bn_weight, bn_bias, bn_running_mean, bn_running_var, Co, sc, sh);
    e->have_conv[layer] = false;
    int rc = enc_upload(e->ctx, &e->w[layer], pk);
    if (rc == GL_OK) rc = enc_upload(e->ctx, &e->scale[layer], sc);
    if (rc == GL_OK) rc = enc_upload(e->ctx, &e->shift[layer], sh);
    if (rc != GL_OK) return rc;
    e->have_conv[layer] = true;
    return GL_OK;
}

int gl_vaegan_enc_set_head(gl_vaegan_enc *e, int head, const float *fc_w, const float *fc_b, const float *bn_weight, const float *bn_bias,
                           const float *bn_running_mean, const float *bn_running_var, const float *out_w, const float *out_b)
{
    gl_make_current(e ? e->ctx : nullptr);
    GL_REQUIRE(e && (head == 0 || head == 1) && fc_w && fc_b && bn_weight && bn_bias && bn_running_mean && bn_running_var && out_w && out_b,
               "gl_vaegan_enc_set_head: bad argument (head 0 or 1, no NULL pointer)");
    const int z = e->z_dim, hid = 4 * z;
    // fc [4 z][c * 16 + p] -> [p * 512 + c][4 z]: ChannelsToLinear flattens NCHW, h4 is NHWC
    std::vector<float> pk((size_t)ENC_FLAT * hid);
    for (int o = 0; o < hid; ++o)
        for (int c = 0; c < 512; ++c)
            for (int p = 0; p < 16; ++p) pk[((size_t)p * 512 + c) * hid + o] = fc_w[(size_t)o * ENC_FLAT + c * 16 + p];
    std::vector<float> sc, sh;
    enc_fold(fc_b, bn_weight, bn_bias, bn_running_mean, bn_running_var, hid, sc, sh);
    std::vector<float> po((size_t)hid * z);
    for (int o = 0; o < z; ++o)
        for (int k = 0; k < hid; ++k) po[(size_t)k * z + o] = out_w[(size_t)o * hid + k];
    e->have_head[head] = false;
    int rc = enc_upload(e->ctx, &e->fc_w[head], pk);
    if (rc == GL_OK) rc = enc_upload(e->ctx, &e->fc_scale[head], sc);
    if (rc == GL_OK) rc = enc_upload(e->ctx, &e->fc_shift[head], sh);
    if (rc == GL_OK) rc = enc_upload(e->ctx, &e->out_w[head], po);
    if (rc == GL_OK) rc = enc_upload(e->ctx, &e->out_b[head], std::vector<float>(out_b, out_b + z));
    if (rc != GL_OK) return rc;
    e->have_head[head] = true;
    return GL_OK;
}

int gl_vaegan_enc_encode(gl_vaegan_enc *e, const uint8_t *images_u8_dev, const float *images_f32_dev, int64_t n, float *mu_dev, float *logvar_dev)
{
    gl_make_current(e ? e->ctx : nullptr);
    GL_REQUIRE(e && n >= 0 && n < (1ll << 31), "gl_vaegan_enc_encode: bad argument");
    if (const char *missing = enc_missing(e)) {
        gl_set_error("gl_vaegan_enc_encode: weights not loaded: %s", missing);
        return GL_ERR_STATE;
    }
    if (n == 0) return GL_OK;
    GL_REQUIRE((images_u8_dev != nullptr) != (images_f32_dev != nullptr), "gl_vaegan_enc_encode: exactly one of images_u8_dev, images_f32_dev must be given");
    GL_REQUIRE(mu_dev && logvar_dev, "gl_vaegan_enc_encode: NULL output pointer");
    GL_REQUIRE((reinterpret_cast<uintptr_t>(images_f32_dev) & 3) == 0 && ((reinterpret_cast<uintptr_t>(mu_dev) | reinterpret_cast<uintptr_t>(logvar_dev)) & 3) == 0,
               "gl_vaegan_enc_encode: float arrays must be 4-byte aligned");
    gl_ctx *ctx = e->ctx;
    const int z = e->z_dim, hid = 4 * z;
    const int64_t pass = n < e->chunk ? n : e->chunk;
    if (pass > e->ws_images) {
        GL_HIP(hipStreamSynchronize(ctx->stream));
        (void)hipFree(e->ws_a); (void)hipFree(e->ws_b); (void)hipFree(e->ws_h);
        e->ws_a = e->ws_b = e->ws_h = nullptr;
        e->ws_images = 0;
        GL_HIP(gl_device_alloc(ctx, (void **)&e->ws_a, (size_t)pass * 32 * 32 * 64 * 4));
        GL_HIP(gl_device_alloc(ctx, (void **)&e->ws_b, (size_t)pass * 16 * 16 * 128 * 4));
        GL_HIP(gl_device_alloc(ctx, (void **)&e->ws_h, (size_t)pass * hid * 4));
        e->ws_images = pass;
    }
    for (int64_t lo = 0; lo < n; lo += pass) {
        const int64_t m = n - lo < pass ? n - lo : pass;
        const void *img = images_u8_dev ? static_cast<const void *>(images_u8_dev + lo * 3 * 64 * 64) : static_cast<const void *>(images_f32_dev + lo * 3 * 64 * 64);
        int rc = enc_launch(ctx, images_u8_dev ? A_IMAGE_U8 : A_IMAGE_F32, img, e->w[0], e->scale[0], e->shift[0], e->ws_a, m * 32 * 32, 64, 48, 3, 64, 1);
        if (rc == GL_OK) rc = enc_launch(ctx, A_NHWC, e->ws_a, e->w[1], e->scale[1], e->shift[1], e->ws_b, m * 16 * 16, 128, 16 * 64, 64, 32, 1);
        if (rc == GL_OK) rc = enc_launch(ctx, A_NHWC, e->ws_b, e->w[2], e->scale[2], e->shift[2], e->ws_a, m * 8 * 8, 256, 16 * 128, 128, 16, 1);
        if (rc == GL_OK) rc = enc_launch(ctx, A_NHWC, e->ws_a, e->w[3], e->scale[3], e->shift[3], e->ws_b, m * 4 * 4, 512, 16 * 256, 256, 8, 1);
        for (int h = 0; h < 2 && rc == GL_OK; ++h) {
            float *out = (h == 0 ? mu_dev : logvar_dev) + lo * z;
            rc = enc_launch(ctx, A_DENSE, e->ws_b, e->fc_w[h], e->fc_scale[h], e->fc_shift[h], e->ws_h, m, hid, ENC_FLAT, 0, 0, 1);
            if (rc == GL_OK) rc = enc_launch(ctx, A_DENSE, e->ws_h, e->out_w[h], nullptr, e->out_b[h], out, m, z, hid, 0, 0, 0);
        }
        if (rc != GL_OK) return rc;
    }
    return GL_OK;
}

}  // extern "C"
