// TUNING BUILD ONLY (linked into libganleaks_hip_tuning.so, never into libganleaks_hip.so; not part of include/ganleaks.h).
// Four entries: gl_tune_winograd_bound (a timing experiment, below), gl_tune_conv_layer (one convolution launch on host arrays, for the
// per-layer tests), gl_tune_split_post (one launch of a stand-alone PixelNorm / LPIPS tap kernel on a split activation) and gl_tune_attention
// (one launch of the self-attention kernel of gl_dcgan.hip; at the end of the file).
//
// gl_tune_winograd_bound: the measured UPPER bound of what Winograd F(2x2,3x3) could buy on the split-fp16 convolution path (VERDICT r2
// "Next 1").  F(2x2,3x3) replaces a 3x3 convolution over P positions by 16 independent GEMMs  M_j = U_j (C_out x C_in) . V_j (C_in x P/4)
// plus an input transform (4 C bytes / position read, 16 C written) and an output transform (16 C_out read, 4 C_out written).  The GEMM stage
// is exactly what the existing tap-gather kernel runs for a ONE-tap convolution, so it can be timed today with the tuned kernel:
//     ms[0] = the direct 3x3 split-fp16 convolution (gl_launch_gather_conv_h3, 9 taps) on n images of H x W, C_in -> C_out, split output
//     ms[1] = the 16 Winograd GEMMs: 16 launches of the same kernel with 1 tap, P/4 rows each, own weights, fp32 output (the accumulators M_j)
// on random operands (the clock the chip holds depends on the data).  Everything a real Winograd kernel adds -- the two transforms, and for a
// fused kernel the small per-component tile (the 16 accumulator sets of a tile share one register file: 64 x 64 per component and CU instead
// of 256 x 256, i.e. 4 x the staging bytes per MFMA) -- comes on top of ms[1].
#include "gl_conv.h"
#include <cmath>
#include <cstring>
#include <vector>

namespace {

__global__ void __launch_bounds__(256) tune_fill_split_kernel(char *__restrict__ out, int64_t chunks, unsigned seed)
{
    // one thread = one 128-byte chunk: 32 hi halves + 32 lo halves of ReLU-like values (half of them zero), |lo| <= 2^-11 |hi|
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < chunks; i += (int64_t)gridDim.x * blockDim.x) {
        unsigned s = seed ^ (unsigned)(i * 2654435761u);
        _Float16 *hi = reinterpret_cast<_Float16 *>(out + i * 128), *lo = hi + 32;
        for (int k = 0; k < 32; ++k) {
            s = s * 1664525u + 1013904223u;
            const float u = (float)((s >> 9) & 0x7FFF) / 32768.0f;          // [0, 1)
            const float v = (s & 0x100u) ? 0.0f : u * 8.0f;
            s = s * 1664525u + 1013904223u;
            const float l = v * ((float)((s >> 9) & 0x7FFF) / 32768.0f - 0.5f) * (1.0f / 2048.0f);
            hi[k] = (_Float16)v;
            lo[k] = (_Float16)l;
        }
    }
}

}  // namespace

extern "C" int gl_tune_winograd_bound(gl_ctx *ctx, int Cin, int Cout, int H, int W, int64_t n_img, int reps, float *ms_out)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx && ms_out && Cin % 32 == 0 && Cout % 32 == 0 && H % 2 == 0 && W % 2 == 0 && n_img > 0 && reps > 0, "gl_tune_winograd_bound: bad argument");
    const int64_t P = n_img * H * W, T = P / 4;
    const int cols_pad = (int)gl_ceil_div(Cout, 128) * 128;
    char *in = nullptr, *V = nullptr;
    float *out = nullptr, *M = nullptr, *w9 = nullptr, *w1 = nullptr, *ones = nullptr, *zeros = nullptr;
    int rc = GL_OK;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto cleanup = [&]() {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(in); (void)hipFree(V); (void)hipFree(out); (void)hipFree(M); (void)hipFree(w9); (void)hipFree(w1); (void)hipFree(ones); (void)hipFree(zeros);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    };
#define TUNE_HIP(e) do { if ((e) != hipSuccess) { gl_set_error("gl_tune_winograd_bound: %s failed", #e); cleanup(); return GL_ERR_HIP; } } while (0)
    TUNE_HIP(hipMalloc((void **)&in, (size_t)P * Cin * 4));
    TUNE_HIP(hipMalloc((void **)&V, (size_t)16 * T * Cin * 4));
    TUNE_HIP(hipMalloc((void **)&out, (size_t)P * Cout * 4));
    TUNE_HIP(hipMalloc((void **)&M, (size_t)16 * T * Cout * 4));
    TUNE_HIP(hipMalloc((void **)&w9, (size_t)cols_pad * 9 * Cin * 4));
    TUNE_HIP(hipMalloc((void **)&w1, (size_t)16 * cols_pad * Cin * 4));
    TUNE_HIP(hipMalloc((void **)&ones, (size_t)Cout * 4));
    TUNE_HIP(hipMalloc((void **)&zeros, (size_t)Cout * 4));
    TUNE_HIP(hipEventCreate(&e0));
    TUNE_HIP(hipEventCreate(&e1));
    {
        std::vector<float> w((size_t)cols_pad * 9 * Cin), sp(w.size()), one(Cout, 1.0f), zero(Cout, 0.0f);
        unsigned s = 12345u;
        auto gauss = [&]() { float a = 0; for (int k = 0; k < 4; ++k) { s = s * 1664525u + 1013904223u; a += (float)(s >> 8) / 16777216.0f; } return (a - 2.0f) * 1.7f; };
        for (float &v : w) v = gauss() * 4096.0f;                       // already at the packed scale (max ~ 2^13)
        for (size_t r = (size_t)Cout * 9 * Cin; r < w.size(); ++r) w[r] = 0.0f;
        gl_split_weights_host(w.data(), cols_pad, (size_t)9 * Cin, 1.0f, sp.data());
        TUNE_HIP(hipMemcpy(w9, sp.data(), sp.size() * 4, hipMemcpyHostToDevice));
        for (int j = 0; j < 16; ++j) {
            std::vector<float> u((size_t)cols_pad * Cin, 0.0f), us(u.size());
            for (size_t r = 0; r < (size_t)Cout * Cin; ++r) u[r] = gauss() * 4096.0f;
            gl_split_weights_host(u.data(), cols_pad, (size_t)Cin, 1.0f, us.data());
            TUNE_HIP(hipMemcpy(w1 + (size_t)j * cols_pad * Cin, us.data(), us.size() * 4, hipMemcpyHostToDevice));
        }
        TUNE_HIP(hipMemcpy(ones, one.data(), Cout * 4, hipMemcpyHostToDevice));
        TUNE_HIP(hipMemcpy(zeros, zero.data(), Cout * 4, hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(tune_fill_split_kernel, dim3(4096), dim3(256), 0, ctx->stream, in, P * Cin / 32, 1u);
    hipLaunchKernelGGL(tune_fill_split_kernel, dim3(4096), dim3(256), 0, ctx->stream, V, 16 * T * Cin / 32, 2u);
    TUNE_HIP(hipGetLastError());

    GlGatherConv d = {};
    d.in = reinterpret_cast<const float *>(in); d.positions = P; d.H = H; d.W = W; d.Cin = Cin; d.ntaps = 9;
    {
        uint32_t dy = 0, dx = 0;
        for (int t = 0; t < 9; ++t) { dy |= (uint32_t)(t / 3) << (2 * t); dx |= (uint32_t)(t % 3) << (2 * t); }
        d.tap_dy[0] = dy; d.tap_dx[0] = dx;
    }
    d.wpack = w9; d.cols = Cout; d.cols_pad = cols_pad;
    d.out = out; d.Ho = H; d.Wo = W; d.omul = 1; d.out_mode = 2;
    d.scale = ones; d.shift = zeros; d.cmod = Cout; d.act = 1; d.zero = ctx->zero_page;
    GlGatherConv g = d;
    g.positions = T; g.H = 1; g.W = 1; g.Ho = 1; g.Wo = 1; g.ntaps = 1; g.tap_dy[0] = 1; g.tap_dx[0] = 1;       // one tap at (0, 0)
    g.out_mode = 0; g.act = 0;

    auto run_direct = [&]() { return gl_launch_gather_conv_h3(ctx, d, 1); };
    auto run_gemms = [&]() {
        for (int j = 0; j < 16; ++j) {
            GlGatherConv q = g;
            q.in = reinterpret_cast<const float *>(V + (size_t)j * T * Cin * 4);
            q.wpack = w1 + (size_t)j * cols_pad * Cin;
            q.out = M + (size_t)j * T * Cout;
            const int r = gl_launch_gather_conv_h3(ctx, q, 1);
            if (r != GL_OK) return r;
        }
        return (int)GL_OK;
    };
    for (int which = 0; which < 2 && rc == GL_OK; ++which) {
        rc = which ? run_gemms() : run_direct();                     // warm-up
        if (rc != GL_OK) break;
        TUNE_HIP(hipEventRecord(e0, ctx->stream));
        for (int r = 0; r < reps && rc == GL_OK; ++r) rc = which ? run_gemms() : run_direct();
        TUNE_HIP(hipEventRecord(e1, ctx->stream));
        TUNE_HIP(hipEventSynchronize(e1));
        float ms = 0.0f;
        TUNE_HIP(hipEventElapsedTime(&ms, e0, e1));
        ms_out[which] = ms / reps;
    }
#undef TUNE_HIP
    cleanup();
    return rc;
}

// gl_tune_conv_layer: ONE launch of gl_launch_gather_conv (kernel 0) or gl_launch_gather_conv_h3 (kernel 1) on a problem given as plain host
// arrays, for tests/test_gpu_conv_layers.py, which compares the whole output tensor with a float64 convolution.  The entry packs the operands the
// way production code does (fp32: gl_conv_k_index order padded to cols_pad; split: gl_split_weights_host / gl_launch_split_rows /
// gl_pack_tail_weights_host with the scale conventions of dcgan_prepare_h3 -- stored activations carry kTuneActScale, weights 2^wexp,
// scale' = s / 2^wexp, shift' = t * kTuneActScale; fp32 output of the split kernel holds true values: scale' = s / (2^wexp * kTuneActScale)),
// and returns the RAW output bytes: decoding the split and planar layouts is the test's job, so the layouts are under test as well.
// Input and output each sit inside a larger allocation: in_guard bytes of `poison` (fp32 values, split like the input on the split path) on
// both sides of the input -- a read that should have been a zero fill returns poison, not something arbitrary -- and 4 KiB of `sentinel` bytes on
// both sides of the output, which is itself pre-filled with `sentinel`; the guards come back so that the caller can see they are untouched.
struct GlTuneConvLayer {                 // mirrored field by field in tests/conv_layer_common.py
    int32_t kernel, phases, ntaps, up;
    int64_t n_img;
    int32_t H, W, Cin, cols, cols_pad;
    int32_t Ho, Wo, omul;
    uint32_t tap_dy[4], tap_dx[4];
    int32_t oy[4], ox[4];
    int32_t planar, out_mode, cmod, act;
    int64_t ld_planar;
    int32_t wexp, tail_wexp;
    const float *in;                     // [n_img][H >> up][W >> up][Cin]
    const float *w;                      // natural order [phases][cols][ntaps][Cin]
    const float *scale, *shift;          // [cmod], true values
    const float *residual;               // nullptr or [n_img][Ho][Wo][cols]
    const float *tail_w;                 // nullptr or [48][cols]: the fused tail; the output is then tail_out [48][n_img * Ho * Wo]
    float poison;
    int32_t sentinel;                    // byte value
    int64_t in_guard;                    // bytes of each input guard: >= 2 (W + 1) Cin 4 rounded up to 4 KiB, a multiple of Cin * 4
    int64_t out_bytes;                   // must be what the problem writes (checked)
    void *out;                           // <- out_bytes
    void *in_guards;                     // <- 2 * in_guard bytes: below | above the input, read back after the launch
    void *out_guards;                    // <- 2 * 4096 bytes: below | above the output
    int64_t sat_delta;                   // <- change of the context's split-store saturation counter
    int32_t form;                        // <- gl_tune_conv_form of the launch
    // fused epilogues (split kernel, out_mode 2).  fuse: 0 none, 1 PixelNorm (pixnorm_act = kTuneActScale), 2 PixelNorm + toRGB (rgb_inv_act =
    // 1 / kTuneActScale), 3 LPIPS tap (tap_scale 16384, tap_eps 1e-10 * kTuneActScale; + the 2 x 2 max-pool when tap_pool != 0), 4 tap AND
    // PixelNorm (which the launcher must refuse).  rgb_out, the V rows and the pooled tensor each get an allocation of their own, pre-filled
    // with `sentinel` between 4 KiB sentinel guards; for fuse 2 and 3 `out` must come back all sentinel.
    int32_t fuse, rgb_n, tap_fmt, tap_pool;
    int32_t reserved_i[3];
    const float *rgb_w, *rgb_b;          // [rgb_n][cols], [rgb_n], true values
    const float *tap_coef;               // [cols]
    void *rgb_out;                       // <- n_img * Ho * Wo * 16 bytes ([pos][4] fp32)
    void *tap_V;                         // <- v_bytes: the whole row buffer
    void *pool_out;                      // <- n_img * (Ho / 2) * (Wo / 2) * cols * 4 bytes (split layout)
    void *aux_guards;                    // <- 3 * 2 * 4096 bytes: below | above of rgb_out, V, pool (sentinel where the buffer was not used)
    void *reserved_p[1];
    int64_t tap_ldv, tap_off, tap_row0;  // as in GlGatherConv; tap_ldv < 0: K-blocked rows of -tap_ldv cells (tap_fmt 1 only)
    int64_t v_bytes;                     // size of the V buffer; every row the launch may touch must lie inside (checked)
};

// the stand-alone kernels sit in anonymous namespaces: tuning-build wrappers at the end of gl_pggan.hip / gl_lpips.hip
int gl_tune_pixelnorm_split(gl_ctx *ctx, char *x, int64_t positions, int C);
int gl_tune_tap_split(gl_ctx *ctx, const char *f, int64_t n, int H, int W, int C, const float *coef, char *V, int64_t ldv, int64_t off, char *pooled, int fmt,
                      float eps, int64_t row0);

// bytes a V buffer needs for rows [0, rows) of k_end halves each in this layout, or -1 when layout and format do not go together
static int64_t tune_v_need(int fmt, int64_t ldv, int64_t rows, int64_t k_end)
{
    if (fmt == 0) return (ldv > 0 && ldv % 128 == 0 && ldv >= k_end * 4) ? rows * ldv : -1;
    if (ldv >= 0) return (ldv % 8 == 0 && ldv >= k_end * 2) ? rows * ldv : -1;
    return (-ldv) * 64 >= k_end ? (rows + 255) / 256 * (-ldv) * 32768 : -1;
}

static const float kTuneActScale = 16.0f;        // gl_dcgan.hip kActScale

extern "C" int gl_tune_conv_layer(gl_ctx *ctx, GlTuneConvLayer *q)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx && q && q->in && q->w && q->scale && q->shift && q->out && q->in_guards && q->out_guards, "gl_tune_conv_layer: NULL argument");
    GL_REQUIRE((q->kernel == 0 || q->kernel == 1) && q->phases >= 1 && q->phases <= 4 && q->ntaps >= 1 && q->ntaps <= 16 && q->n_img > 0 && q->H > 0 &&
                   q->W > 0 && q->Cin > 0 && q->Cin % 32 == 0 && q->cols > 0 && q->cols <= q->cols_pad && q->cmod > 0 && (q->up == 0 || q->up == 1) &&
                   q->Ho > 0 && q->Wo > 0 && q->omul >= 1,
               "gl_tune_conv_layer: bad problem");
    GL_REQUIRE(q->kernel == 1 || (!q->tail_w && q->out_mode == 0), "gl_tune_conv_layer: split output and the fused tail are the split kernel's");
    GL_REQUIRE(!q->tail_w || q->cols == 64 || q->cols == 128, "gl_tune_conv_layer: the fused tail takes 64 or 128 channels");
    for (int ph = 0; ph < q->phases; ++ph)
        GL_REQUIRE(q->oy[ph] >= 0 && q->ox[ph] >= 0 && (q->H - 1) * q->omul + q->oy[ph] < q->Ho && (q->W - 1) * q->omul + q->ox[ph] < q->Wo,
                   "gl_tune_conv_layer: the output map of phase %d leaves the %d x %d output", ph, q->Ho, q->Wo);
    const bool h3 = q->kernel == 1;
    const int Hs = q->H >> q->up, Ws = q->W >> q->up, K = q->ntaps * q->Cin;
    const int64_t positions = q->n_img * q->H * q->W, opos = q->n_img * q->Ho * q->Wo;
    const int64_t in_bytes = q->n_img * Hs * Ws * q->Cin * 4;
    const int64_t lead = ((2ll * (q->W + 1) * q->Cin * 4) + 4095) / 4096 * 4096;
    GL_REQUIRE(q->in_guard >= lead && q->in_guard % (q->Cin * 4) == 0, "gl_tune_conv_layer: in_guard=%lld must be >= %lld and a multiple of Cin * 4",
               (long long)q->in_guard, (long long)lead);
    if (q->planar) GL_REQUIRE(q->ld_planar >= opos && opos == positions, "gl_tune_conv_layer: planar output needs ld_planar >= positions and an identity map");
    const int64_t out_bytes = q->tail_w ? 48 * opos * 4 : q->planar ? (int64_t)q->cols * q->ld_planar * 4 : opos * q->cols * 4;
    GL_REQUIRE(q->out_bytes == out_bytes, "gl_tune_conv_layer: out_bytes=%lld, the problem writes %lld", (long long)q->out_bytes, (long long)out_bytes);
    constexpr int64_t OG = 4096;
    const int64_t in_total = in_bytes + 2 * q->in_guard;
    const size_t w_elems = (size_t)q->phases * q->cols_pad * K;
    const int fuse = q->fuse;
    const bool f_rgb = fuse == 2, f_tap = fuse == 3 || fuse == 4, f_pool = f_tap && q->tap_pool != 0;
    GL_REQUIRE(fuse >= 0 && fuse <= 4, "gl_tune_conv_layer: fuse=%d", fuse);
    GL_REQUIRE(fuse == 0 || (h3 && q->out_mode == 2 && !q->tail_w && !q->planar && q->cols % 32 == 0), "gl_tune_conv_layer: the fused epilogues need the split kernel and split output");
    GL_REQUIRE(fuse == 0 || q->aux_guards, "gl_tune_conv_layer: NULL aux_guards");
    GL_REQUIRE(!f_rgb || (q->rgb_w && q->rgb_b && q->rgb_out && q->rgb_n >= 1 && q->rgb_n <= 4), "gl_tune_conv_layer: toRGB needs rgb_w, rgb_b, rgb_out and rgb_n in 1..4");
    const int64_t rgb_bytes = f_rgb ? opos * 16 : 0;
    const int64_t pool_bytes = f_pool ? q->n_img * (q->Ho / 2) * (q->Wo / 2) * q->cols * 4 : 0;
    const int64_t v_bytes = f_tap ? q->v_bytes : 0;
    if (f_tap) {
        GL_REQUIRE(q->tap_coef && q->tap_V && (q->tap_fmt == 0 || q->tap_fmt == 1) && q->tap_row0 >= 0 && q->tap_off >= 0 && q->tap_off % 64 == 0 &&
                       (!f_pool || q->pool_out),
                   "gl_tune_conv_layer: bad tap arguments");
        // the kernel takes the row from the output position: every row [tap_row0, tap_row0 + n_img) up to half tap_off + Ho * Wo * cols must lie
        // inside the buffer the caller sized
        const int64_t need = tune_v_need(q->tap_fmt, q->tap_ldv, q->tap_row0 + q->n_img, q->tap_off + (int64_t)q->Ho * q->Wo * q->cols);
        GL_REQUIRE(need > 0 && need <= v_bytes, "gl_tune_conv_layer: the V rows need %lld bytes, v_bytes=%lld (tap_ldv=%lld)", (long long)need,
                   (long long)v_bytes, (long long)q->tap_ldv);
    }

    char *d_in = nullptr, *d_split = nullptr, *d_out = nullptr, *d_tail = nullptr, *d_rgb = nullptr, *d_V = nullptr, *d_pool = nullptr;
    float *d_w = nullptr, *d_scale = nullptr, *d_shift = nullptr, *d_res = nullptr, *d_rgbw = nullptr, *d_rgbb = nullptr, *d_coef = nullptr;
    auto cleanup = [&]() {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(d_in); (void)hipFree(d_split); (void)hipFree(d_out); (void)hipFree(d_tail); (void)hipFree(d_rgb); (void)hipFree(d_V); (void)hipFree(d_pool);
        (void)hipFree(d_w); (void)hipFree(d_scale); (void)hipFree(d_shift); (void)hipFree(d_res); (void)hipFree(d_rgbw); (void)hipFree(d_rgbb); (void)hipFree(d_coef);
    };
#define TUNE_HIP(e) do { if ((e) != hipSuccess) { gl_set_error("gl_tune_conv_layer: %s failed", #e); cleanup(); return GL_ERR_HIP; } } while (0)
#define TUNE_RC(e) do { const int rc_ = (e); if (rc_ != GL_OK) { cleanup(); return rc_; } } while (0)
    TUNE_HIP(hipMalloc((void **)&d_in, (size_t)in_total));
    if (h3) TUNE_HIP(hipMalloc((void **)&d_split, (size_t)in_total));
    TUNE_HIP(hipMalloc((void **)&d_out, (size_t)(out_bytes + 2 * OG)));
    TUNE_HIP(hipMalloc((void **)&d_w, w_elems * 4));
    TUNE_HIP(hipMalloc((void **)&d_scale, (size_t)q->cmod * 4));
    TUNE_HIP(hipMalloc((void **)&d_shift, (size_t)q->cmod * 4));
    if (q->residual) TUNE_HIP(hipMalloc((void **)&d_res, (size_t)(opos * q->cols * 4)));
    if (q->tail_w) TUNE_HIP(hipMalloc((void **)&d_tail, 24 * 1024));
    if (f_rgb) {
        TUNE_HIP(hipMalloc((void **)&d_rgb, (size_t)(rgb_bytes + 2 * OG)));
        TUNE_HIP(hipMalloc((void **)&d_rgbw, (size_t)q->rgb_n * q->cols * 4));
        TUNE_HIP(hipMalloc((void **)&d_rgbb, 16));
        TUNE_HIP(hipMemcpy(d_rgbw, q->rgb_w, (size_t)q->rgb_n * q->cols * 4, hipMemcpyHostToDevice));
        TUNE_HIP(hipMemset(d_rgbb, 0, 16));
        TUNE_HIP(hipMemcpy(d_rgbb, q->rgb_b, (size_t)q->rgb_n * 4, hipMemcpyHostToDevice));
        TUNE_HIP(hipMemsetAsync(d_rgb, q->sentinel & 0xFF, (size_t)(rgb_bytes + 2 * OG), ctx->stream));
    }
    if (f_tap) {
        TUNE_HIP(hipMalloc((void **)&d_V, (size_t)(v_bytes + 2 * OG)));
        TUNE_HIP(hipMalloc((void **)&d_coef, (size_t)q->cols * 4));
        TUNE_HIP(hipMemcpy(d_coef, q->tap_coef, (size_t)q->cols * 4, hipMemcpyHostToDevice));
        TUNE_HIP(hipMemsetAsync(d_V, q->sentinel & 0xFF, (size_t)(v_bytes + 2 * OG), ctx->stream));
    }
    if (f_pool) {
        TUNE_HIP(hipMalloc((void **)&d_pool, (size_t)(pool_bytes + 2 * OG)));
        TUNE_HIP(hipMemsetAsync(d_pool, q->sentinel & 0xFF, (size_t)(pool_bytes + 2 * OG), ctx->stream));
    }
    {
        // input: [guard | tensor | guard] as fp32 rows of Cin values; the split path converts all of it, guards included
        std::vector<float> guard((size_t)(q->in_guard / 4), q->poison);
        TUNE_HIP(hipMemcpyAsync(d_in, guard.data(), (size_t)q->in_guard, hipMemcpyHostToDevice, ctx->stream));
        TUNE_HIP(hipMemcpyAsync(d_in + q->in_guard, q->in, (size_t)in_bytes, hipMemcpyHostToDevice, ctx->stream));
        TUNE_HIP(hipMemcpyAsync(d_in + q->in_guard + in_bytes, guard.data(), (size_t)q->in_guard, hipMemcpyHostToDevice, ctx->stream));
        TUNE_HIP(hipStreamSynchronize(ctx->stream));
        if (h3) TUNE_RC(gl_launch_split_rows(ctx, reinterpret_cast<const float *>(d_in), in_total / (q->Cin * 4), q->Cin, q->Cin, kTuneActScale, d_split));
        // weights: natural [phase][col][tap][ci] -> [phase][cols_pad][gl_conv_k_index(tap, ci)], rows beyond cols zero
        std::vector<float> pk(w_elems, 0.0f);
        for (int ph = 0; ph < q->phases; ++ph)
            for (int c = 0; c < q->cols; ++c)
                for (int t = 0; t < q->ntaps; ++t)
                    for (int ci = 0; ci < q->Cin; ++ci)
                        pk[((size_t)ph * q->cols_pad + c) * K + gl_conv_k_index(t, ci, q->ntaps)] = q->w[(((size_t)ph * q->cols + c) * q->ntaps + t) * q->Cin + ci];
        if (h3) {
            std::vector<float> sp(w_elems);
            gl_split_weights_host(pk.data(), (size_t)q->phases * q->cols_pad, (size_t)K, std::ldexp(1.0f, q->wexp), sp.data());
            pk.swap(sp);
        }
        TUNE_HIP(hipMemcpy(d_w, pk.data(), w_elems * 4, hipMemcpyHostToDevice));
        std::vector<float> sc(q->scale, q->scale + q->cmod), sh(q->shift, q->shift + q->cmod);
        if (h3) {
            const bool stored = q->out_mode == 2 || q->tail_w;      // the output (or the tail's operand) carries kTuneActScale
            for (int i = 0; i < q->cmod; ++i) {
                sc[i] = std::ldexp(sc[i], -q->wexp) / (stored ? 1.0f : kTuneActScale);
                sh[i] = stored ? sh[i] * kTuneActScale : sh[i];
            }
        }
        TUNE_HIP(hipMemcpy(d_scale, sc.data(), (size_t)q->cmod * 4, hipMemcpyHostToDevice));
        TUNE_HIP(hipMemcpy(d_shift, sh.data(), (size_t)q->cmod * 4, hipMemcpyHostToDevice));
        if (q->residual) TUNE_HIP(hipMemcpy(d_res, q->residual, (size_t)(opos * q->cols * 4), hipMemcpyHostToDevice));
        if (q->tail_w) {
            std::vector<float> img(24 * 1024 / 4, 0.0f);
            gl_pack_tail_weights_host(q->tail_w, q->cols, std::ldexp(1.0f, q->tail_wexp), img.data());
            TUNE_HIP(hipMemcpy(d_tail, img.data(), 24 * 1024, hipMemcpyHostToDevice));
        }
    }
    TUNE_HIP(hipMemsetAsync(d_out, q->sentinel & 0xFF, (size_t)(out_bytes + 2 * OG), ctx->stream));
    int sat0 = 0, sat1 = 0;
    TUNE_HIP(hipStreamSynchronize(ctx->stream));
    TUNE_HIP(hipMemcpy(&sat0, ctx->h3_sat, 4, hipMemcpyDeviceToHost));

    GlGatherConv p = {};
    p.in = reinterpret_cast<const float *>((h3 ? d_split : d_in) + q->in_guard);
    p.positions = positions; p.H = q->H; p.W = q->W; p.Cin = q->Cin; p.up = q->up;
    p.wpack = d_w; p.cols = q->cols; p.cols_pad = q->cols_pad; p.ntaps = q->ntaps;
    for (int i = 0; i < 4; ++i) { p.tap_dy[i] = q->tap_dy[i]; p.tap_dx[i] = q->tap_dx[i]; p.oy[i] = q->oy[i]; p.ox[i] = q->ox[i]; }
    p.out = reinterpret_cast<float *>(d_out + OG); p.Ho = q->Ho; p.Wo = q->Wo; p.omul = q->omul;
    p.planar = q->planar; p.ld_planar = q->ld_planar; p.out_mode = q->out_mode;
    p.scale = d_scale; p.shift = d_shift; p.cmod = q->cmod; p.act = q->act; p.residual = d_res; p.zero = ctx->zero_page;
    if (q->tail_w) {
        p.tail_w = d_tail; p.tail_out = reinterpret_cast<float *>(d_out + OG); p.tail_ld = opos;
        p.tail_scale = std::ldexp(1.0f / kTuneActScale, -q->tail_wexp);       // `out` is ignored by the fused-tail forms; it stays inside the guarded block
    }
    if (fuse == 1 || fuse == 2 || fuse == 4) p.pixnorm_act = kTuneActScale;
    if (f_rgb) { p.rgb_w = d_rgbw; p.rgb_b = d_rgbb; p.rgb_out = reinterpret_cast<float *>(d_rgb + OG); p.rgb_n = q->rgb_n; p.rgb_inv_act = 1.0f / kTuneActScale; }
    if (f_tap) {
        p.tap_V = d_V + OG; p.tap_coef = d_coef; p.tap_ldv = q->tap_ldv; p.tap_off = q->tap_off; p.tap_row0 = q->tap_row0; p.tap_fmt = q->tap_fmt;
        p.tap_pool = f_pool ? d_pool + OG : nullptr; p.tap_scale = 16384.0f; p.tap_eps = 1e-10f * kTuneActScale;
    }
    gl_tune_conv_form = 0;
    TUNE_RC(h3 ? gl_launch_gather_conv_h3(ctx, p, q->phases) : gl_tune_gather_conv(ctx, p, q->phases));
    TUNE_HIP(hipStreamSynchronize(ctx->stream));
    q->form = gl_tune_conv_form;
    TUNE_HIP(hipMemcpy(&sat1, ctx->h3_sat, 4, hipMemcpyDeviceToHost));
    q->sat_delta = (int64_t)sat1 - sat0;
    char *d_src = h3 ? d_split : d_in;
    TUNE_HIP(hipMemcpy(q->in_guards, d_src, (size_t)q->in_guard, hipMemcpyDeviceToHost));
    TUNE_HIP(hipMemcpy(reinterpret_cast<char *>(q->in_guards) + q->in_guard, d_src + q->in_guard + in_bytes, (size_t)q->in_guard, hipMemcpyDeviceToHost));
    TUNE_HIP(hipMemcpy(q->out_guards, d_out, (size_t)OG, hipMemcpyDeviceToHost));
    TUNE_HIP(hipMemcpy(reinterpret_cast<char *>(q->out_guards) + OG, d_out + OG + out_bytes, (size_t)OG, hipMemcpyDeviceToHost));
    TUNE_HIP(hipMemcpy(q->out, d_out + OG, (size_t)out_bytes, hipMemcpyDeviceToHost));
    if (fuse) {
        char *ag = reinterpret_cast<char *>(q->aux_guards);
        std::memset(ag, q->sentinel & 0xFF, (size_t)(6 * OG));
        char *bufs[3] = {d_rgb, d_V, d_pool};
        void *host[3] = {q->rgb_out, q->tap_V, q->pool_out};
        const int64_t bytes[3] = {rgb_bytes, v_bytes, pool_bytes};
        for (int b = 0; b < 3; ++b) {
            if (!bufs[b]) continue;
            TUNE_HIP(hipMemcpy(ag + (2 * b) * OG, bufs[b], (size_t)OG, hipMemcpyDeviceToHost));
            TUNE_HIP(hipMemcpy(ag + (2 * b + 1) * OG, bufs[b] + OG + bytes[b], (size_t)OG, hipMemcpyDeviceToHost));
            TUNE_HIP(hipMemcpy(host[b], bufs[b] + OG, (size_t)bytes[b], hipMemcpyDeviceToHost));
        }
    }
#undef TUNE_HIP
#undef TUNE_RC
    cleanup();
    return GL_OK;
}

// gl_tune_split_post: ONE launch of a stand-alone kernel that follows a convolution on the split layout -- pixelnorm_split_kernel (op 0, in place),
// lpips_tap_split_kernel (op 1) or lpips_tap_pool_split_kernel (op 2) -- on host bytes of a split activation [n_img * H * W][C], for
// tests/test_gpu_conv_epilogues.py.  Same treatment as above: every buffer between 4 KiB sentinel guards, V and pool pre-filled with the sentinel,
// raw bytes back.  The tap parameters mean what they mean in GlGatherConv; the scale is the kernels' own (16384).
struct GlTuneSplitPost {                 // mirrored field by field in tests/conv_layer_common.py
    int32_t op, C, H, W;
    int64_t n_img;
    int32_t tap_fmt, sentinel;
    int64_t tap_ldv, tap_off, tap_row0, v_bytes;
    float tap_eps;
    int32_t reserved_i;
    const void *act;                     // n_img * H * W * C * 4 bytes
    const float *tap_coef;               // [C] (ops 1, 2)
    void *act_out;                       // <- the activation buffer after the launch (op 0: normalised; ops 1, 2: must be unchanged)
    void *tap_V;                         // <- v_bytes
    void *pool_out;                      // <- n_img * (H / 2) * (W / 2) * C * 4 bytes (op 2)
    void *guards;                        // <- 3 * 2 * 4096 bytes: below | above of the activation, V, pool
};

extern "C" int gl_tune_split_post(gl_ctx *ctx, GlTuneSplitPost *q)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx && q && q->act && q->act_out && q->guards, "gl_tune_split_post: NULL argument");
    GL_REQUIRE(q->op >= 0 && q->op <= 2 && q->n_img > 0 && q->H > 0 && q->W > 0 && q->C > 0 && q->C % 32 == 0, "gl_tune_split_post: bad problem");
    const bool tap = q->op != 0, pool = q->op == 2;
    constexpr int64_t OG = 4096;
    const int64_t positions = q->n_img * q->H * q->W, act_bytes = positions * q->C * 4;
    const int64_t v_bytes = tap ? q->v_bytes : 0, pool_bytes = pool ? q->n_img * (q->H / 2) * (q->W / 2) * q->C * 4 : 0;
    if (tap) {
        GL_REQUIRE((q->C == 64 || q->C == 128 || q->C == 256 || q->C == 512) && q->tap_coef && q->tap_V && (q->tap_fmt == 0 || q->tap_fmt == 1) &&
                       q->tap_row0 >= 0 && q->tap_off >= 0 && q->tap_off % 64 == 0,
                   "gl_tune_split_post: bad tap arguments");
        GL_REQUIRE(!pool || (q->pool_out && q->H % 2 == 0 && q->W % 2 == 0), "gl_tune_split_post: the pool needs even H and W");
        const int64_t need = tune_v_need(q->tap_fmt, q->tap_ldv, q->tap_row0 + q->n_img, q->tap_off + (int64_t)q->H * q->W * q->C);
        GL_REQUIRE(need > 0 && need <= v_bytes, "gl_tune_split_post: the V rows need %lld bytes, v_bytes=%lld (tap_ldv=%lld)", (long long)need,
                   (long long)v_bytes, (long long)q->tap_ldv);
    }
    char *d_act = nullptr, *d_V = nullptr, *d_pool = nullptr;
    float *d_coef = nullptr;
    auto cleanup = [&]() {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(d_act); (void)hipFree(d_V); (void)hipFree(d_pool); (void)hipFree(d_coef);
    };
#define TUNE_HIP(e) do { if ((e) != hipSuccess) { gl_set_error("gl_tune_split_post: %s failed", #e); cleanup(); return GL_ERR_HIP; } } while (0)
#define TUNE_RC(e) do { const int rc_ = (e); if (rc_ != GL_OK) { cleanup(); return rc_; } } while (0)
    TUNE_HIP(hipMalloc((void **)&d_act, (size_t)(act_bytes + 2 * OG)));
    TUNE_HIP(hipMemset(d_act, q->sentinel & 0xFF, (size_t)(act_bytes + 2 * OG)));
    TUNE_HIP(hipMemcpy(d_act + OG, q->act, (size_t)act_bytes, hipMemcpyHostToDevice));
    if (tap) {
        TUNE_HIP(hipMalloc((void **)&d_V, (size_t)(v_bytes + 2 * OG)));
        TUNE_HIP(hipMemset(d_V, q->sentinel & 0xFF, (size_t)(v_bytes + 2 * OG)));
        TUNE_HIP(hipMalloc((void **)&d_coef, (size_t)q->C * 4));
        TUNE_HIP(hipMemcpy(d_coef, q->tap_coef, (size_t)q->C * 4, hipMemcpyHostToDevice));
    }
    if (pool) {
        TUNE_HIP(hipMalloc((void **)&d_pool, (size_t)(pool_bytes + 2 * OG)));
        TUNE_HIP(hipMemset(d_pool, q->sentinel & 0xFF, (size_t)(pool_bytes + 2 * OG)));
    }
    TUNE_HIP(hipDeviceSynchronize());
    if (!tap) TUNE_RC(gl_tune_pixelnorm_split(ctx, d_act + OG, positions, q->C));
    else TUNE_RC(gl_tune_tap_split(ctx, d_act + OG, q->n_img, q->H, q->W, q->C, d_coef, d_V + OG, q->tap_ldv, q->tap_off, pool ? d_pool + OG : nullptr, q->tap_fmt,
                                   q->tap_eps, q->tap_row0));
    TUNE_HIP(hipStreamSynchronize(ctx->stream));
    {
        char *g = reinterpret_cast<char *>(q->guards);
        std::memset(g, q->sentinel & 0xFF, (size_t)(6 * OG));
        char *bufs[3] = {d_act, d_V, d_pool};
        void *host[3] = {q->act_out, q->tap_V, q->pool_out};
        const int64_t bytes[3] = {act_bytes, v_bytes, pool_bytes};
        for (int b = 0; b < 3; ++b) {
            if (!bufs[b]) continue;
            TUNE_HIP(hipMemcpy(g + (2 * b) * OG, bufs[b], (size_t)OG, hipMemcpyDeviceToHost));
            TUNE_HIP(hipMemcpy(g + (2 * b + 1) * OG, bufs[b] + OG + bytes[b], (size_t)OG, hipMemcpyDeviceToHost));
            TUNE_HIP(hipMemcpy(host[b], bufs[b] + OG, (size_t)bytes[b], hipMemcpyDeviceToHost));
        }
    }
#undef TUNE_HIP
#undef TUNE_RC
    cleanup();
    return GL_OK;
}

// gl_tune_attention: ONE launch of launch_attention_core<64 | 128> (csrc/gl_dcgan.hip) on plain host arrays, for tests/test_gpu_attention.py.
// qkv fp32 [n_img][256][2 C / 8 + C]; x and y are RAW bytes, n_img * 256 * C * 4 of them: fp32 NHWC, or with `split` the split-fp16 layout the
// kernel reads and writes (encoding and decoding it is the test's job, so the layout is under test as well).  Same treatment as above: qkv and x
// each sit between 4 KiB guards of `poison` (fp32 values; fp16 halves of the same value around a split x), y is pre-filled with `sentinel` and
// sits between 4 KiB sentinel guards, which come back.
struct GlTuneAttention {                 // mirrored field by field in tests/attention_common.py
    int32_t C, split;
    int64_t n_img;
    float gamma, poison;
    int32_t sentinel, reserved_i;
    const float *qkv;
    const void *x;
    void *y;                             // <- n_img * 256 * C * 4 bytes
    void *out_guards;                    // <- 2 * 4096 bytes: below | above y
    int64_t sat_delta;                   // <- change of the context's split-store saturation counter
};

int gl_tune_attention_core(gl_ctx *ctx, int C, int split, const float *qkv, const float *x, float *y, int64_t images, float gamma);   // gl_dcgan.hip

extern "C" int gl_tune_attention(gl_ctx *ctx, GlTuneAttention *q)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx && q && q->qkv && q->x && q->y && q->out_guards, "gl_tune_attention: NULL argument");
    GL_REQUIRE((q->C == 64 || q->C == 128) && q->n_img > 0 && q->n_img <= 4096, "gl_tune_attention: C must be 64 or 128, n_img in 1..4096");
    constexpr int64_t G = 4096;
    const int64_t qkv_bytes = q->n_img * 256 * (2 * (q->C / 8) + q->C) * 4, x_bytes = q->n_img * 256 * q->C * 4;
    char *d_qkv = nullptr, *d_x = nullptr, *d_y = nullptr;
    auto cleanup = [&]() {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(d_qkv); (void)hipFree(d_x); (void)hipFree(d_y);
    };
#define TUNE_HIP(e) do { if ((e) != hipSuccess) { gl_set_error("gl_tune_attention: %s failed", #e); cleanup(); return GL_ERR_HIP; } } while (0)
#define TUNE_RC(e) do { const int rc_ = (e); if (rc_ != GL_OK) { cleanup(); return rc_; } } while (0)
    TUNE_HIP(hipMalloc((void **)&d_qkv, (size_t)(qkv_bytes + 2 * G)));
    TUNE_HIP(hipMalloc((void **)&d_x, (size_t)(x_bytes + 2 * G)));
    TUNE_HIP(hipMalloc((void **)&d_y, (size_t)(x_bytes + 2 * G)));
    {
        std::vector<float> gf((size_t)(G / 4), q->poison);
        std::vector<_Float16> gh((size_t)(G / 2), (_Float16)q->poison);
        const void *gx = q->split ? (const void *)gh.data() : (const void *)gf.data();
        TUNE_HIP(hipMemcpy(d_qkv, gf.data(), (size_t)G, hipMemcpyHostToDevice));
        TUNE_HIP(hipMemcpy(d_qkv + G, q->qkv, (size_t)qkv_bytes, hipMemcpyHostToDevice));
        TUNE_HIP(hipMemcpy(d_qkv + G + qkv_bytes, gf.data(), (size_t)G, hipMemcpyHostToDevice));
        TUNE_HIP(hipMemcpy(d_x, gx, (size_t)G, hipMemcpyHostToDevice));
        TUNE_HIP(hipMemcpy(d_x + G, q->x, (size_t)x_bytes, hipMemcpyHostToDevice));
        TUNE_HIP(hipMemcpy(d_x + G + x_bytes, gx, (size_t)G, hipMemcpyHostToDevice));
    }
    TUNE_HIP(hipMemset(d_y, q->sentinel & 0xFF, (size_t)(x_bytes + 2 * G)));
    int sat0 = 0, sat1 = 0;
    TUNE_HIP(hipDeviceSynchronize());
    TUNE_HIP(hipMemcpy(&sat0, ctx->h3_sat, 4, hipMemcpyDeviceToHost));
    TUNE_RC(gl_tune_attention_core(ctx, q->C, q->split, reinterpret_cast<const float *>(d_qkv + G), reinterpret_cast<const float *>(d_x + G),
                                   reinterpret_cast<float *>(d_y + G), q->n_img, q->gamma));
    TUNE_HIP(hipStreamSynchronize(ctx->stream));
    TUNE_HIP(hipMemcpy(&sat1, ctx->h3_sat, 4, hipMemcpyDeviceToHost));
    q->sat_delta = (int64_t)sat1 - sat0;
    TUNE_HIP(hipMemcpy(q->out_guards, d_y, (size_t)G, hipMemcpyDeviceToHost));
    TUNE_HIP(hipMemcpy(reinterpret_cast<char *>(q->out_guards) + G, d_y + G + x_bytes, (size_t)G, hipMemcpyDeviceToHost));
    TUNE_HIP(hipMemcpy(q->y, d_y + G, (size_t)x_bytes, hipMemcpyDeviceToHost));
#undef TUNE_HIP
#undef TUNE_RC
    cleanup();
    return GL_OK;
}

// gl_tune_attention_grad: ONE launch sequence of the attention backward (gl_launch_attention_grad, csrc/gl_attention_grad.hip: the row kernel, then the
// column kernel) on plain host arrays, for tests/test_gpu_attention_grad.py.  qkv fp32 [n_img][256][2 C / 8 + C] and dY fp32 [n_img][256][C] each sit
// between 4 KiB guards of `poison`; dqkv [n_img][256][cols] (cols = 2 C / 8 + C rounded up to a multiple of 32: the zero columns of the projection
// GEMM come back as well) and stats [n_img][3][256] (m, 1 / l, D) are pre-filled with `sentinel` and sit between 4 KiB sentinel guards, which come back.
struct GlTuneAttentionGrad {             // mirrored field by field in tests/attention_grad_common.py
    int32_t C, cols;                     // cols <- the row length of dqkv
    int64_t n_img;
    float gamma, poison;
    int32_t sentinel, reserved_i;
    const float *qkv, *dY;
    float *dqkv;                         // <- n_img * 256 * cols floats
    float *stats;                        // <- n_img * 3 * 256 floats
    void *out_guards;                    // <- 4 * 4096 bytes: below | above dqkv, below | above stats
};

int gl_attention_grad_cols(int C);                                                                                                      // gl_attention_grad.hip
int gl_launch_attention_grad(gl_ctx *ctx, int C, const float *qkv, const float *dY, float gamma, int64_t images, float *dqkv, float *stats);

extern "C" int gl_tune_attention_grad(gl_ctx *ctx, GlTuneAttentionGrad *q)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx && q && q->qkv && q->dY && q->dqkv && q->stats && q->out_guards, "gl_tune_attention_grad: NULL argument");
    GL_REQUIRE((q->C == 64 || q->C == 128) && q->n_img > 0 && q->n_img <= 4096, "gl_tune_attention_grad: C must be 64 or 128, n_img in 1..4096");
    constexpr int64_t G = 4096;
    q->cols = gl_attention_grad_cols(q->C);
    const int64_t in_bytes[2] = {q->n_img * 256 * (2 * (q->C / 8) + q->C) * 4, q->n_img * 256 * q->C * 4};
    const int64_t out_bytes[2] = {q->n_img * 256 * q->cols * 4, q->n_img * 3 * 256 * 4};
    const void *in_host[2] = {q->qkv, q->dY};
    void *out_host[2] = {q->dqkv, q->stats};
    char *d_in[2] = {nullptr, nullptr}, *d_out[2] = {nullptr, nullptr};
    auto cleanup = [&]() {
        (void)hipStreamSynchronize(ctx->stream);
        for (int b = 0; b < 2; ++b) { (void)hipFree(d_in[b]); (void)hipFree(d_out[b]); }
    };
#define TUNE_HIP(e) do { if ((e) != hipSuccess) { gl_set_error("gl_tune_attention_grad: %s failed", #e); cleanup(); return GL_ERR_HIP; } } while (0)
#define TUNE_RC(e) do { const int rc_ = (e); if (rc_ != GL_OK) { cleanup(); return rc_; } } while (0)
    std::vector<float> gf((size_t)(G / 4), q->poison);
    for (int b = 0; b < 2; ++b) {
        TUNE_HIP(hipMalloc((void **)&d_in[b], (size_t)(in_bytes[b] + 2 * G)));
        TUNE_HIP(hipMalloc((void **)&d_out[b], (size_t)(out_bytes[b] + 2 * G)));
        TUNE_HIP(hipMemcpy(d_in[b], gf.data(), (size_t)G, hipMemcpyHostToDevice));
        TUNE_HIP(hipMemcpy(d_in[b] + G, in_host[b], (size_t)in_bytes[b], hipMemcpyHostToDevice));
        TUNE_HIP(hipMemcpy(d_in[b] + G + in_bytes[b], gf.data(), (size_t)G, hipMemcpyHostToDevice));
        TUNE_HIP(hipMemset(d_out[b], q->sentinel & 0xFF, (size_t)(out_bytes[b] + 2 * G)));
    }
    TUNE_HIP(hipDeviceSynchronize());
    TUNE_RC(gl_launch_attention_grad(ctx, q->C, reinterpret_cast<const float *>(d_in[0] + G), reinterpret_cast<const float *>(d_in[1] + G), q->gamma, q->n_img,
                                     reinterpret_cast<float *>(d_out[0] + G), reinterpret_cast<float *>(d_out[1] + G)));
    TUNE_HIP(hipStreamSynchronize(ctx->stream));
    for (int b = 0; b < 2; ++b) {
        char *og = reinterpret_cast<char *>(q->out_guards) + 2 * b * G;
        TUNE_HIP(hipMemcpy(og, d_out[b], (size_t)G, hipMemcpyDeviceToHost));
        TUNE_HIP(hipMemcpy(og + G, d_out[b] + G + out_bytes[b], (size_t)G, hipMemcpyDeviceToHost));
        TUNE_HIP(hipMemcpy(out_host[b], d_out[b] + G, (size_t)out_bytes[b], hipMemcpyDeviceToHost));
    }
#undef TUNE_HIP
#undef TUNE_RC
    cleanup();
    return GL_OK;
}

// gl_tune_grad_op: ONE launch of one element-wise or per-position kernel of the white-box backward passes (csrc/gl_dcgan_grad.hip, gl_pggan_grad.hip,
// gl_lpips_grad.hip) on plain host arrays, for tests/test_gpu_grad_kernels.py.  family 0 / 1 / 2 names the file, `op` the kernel and ip / f0 its
// arguments as the file's launcher at its end lists them; the launch goes through the function the production pass calls, so the grid, its cap and the
// template instance are the production ones.  Every input given sits between 4 KiB guards of `poison` (fp32 values); every output is pre-filled with
// `sentinel` bytes and sits between 4 KiB sentinel guards, which come back.  copy_in >= 0: out[0] starts as a copy of that input (a kernel that works
// in place).  A NULL input or output slot reaches the kernel as NULL.
struct GlTuneGradOp {                    // mirrored field by field in tests/grad_kernels_common.py
    int32_t family, op;
    int32_t sentinel, copy_in;
    float poison, f0;
    int64_t ip[12];
    const void *in[4];
    int64_t in_bytes[4];
    void *out[2];                        // <- out_bytes[k] bytes each
    int64_t out_bytes[2];
    void *out_guards;                    // <- 4 * 4096 bytes: below | above out[0], below | above out[1]
};
static_assert(sizeof(GlTuneGradOp) == 224 && offsetof(GlTuneGradOp, ip) == 24 && offsetof(GlTuneGradOp, in) == 120 && offsetof(GlTuneGradOp, in_bytes) == 152 &&
                  offsetof(GlTuneGradOp, out) == 184 && offsetof(GlTuneGradOp, out_bytes) == 200 && offsetof(GlTuneGradOp, out_guards) == 216,
              "GlTuneGradOp: tests/grad_kernels_common.py mirrors this layout");

// nb: the bytes of in[0 .. 3] and out[0 .. 1], 0 for a NULL slot: each file checks them against the shapes in ip before it launches
int gl_tune_dcgan_grad_op(gl_ctx *ctx, int op, const int64_t *ip, const int64_t *nb, void *const *in, void *const *out);                       // gl_dcgan_grad.hip
int gl_tune_pggan_grad_op(gl_ctx *ctx, int op, const int64_t *ip, const int64_t *nb, const float *fp, void *const *in, void *const *out);      // gl_pggan_grad.hip
int gl_tune_lpips_grad_op(gl_ctx *ctx, int op, const int64_t *ip, const int64_t *nb, void *const *in, void *const *out);                       // gl_lpips_grad.hip

extern "C" int gl_tune_grad_op(gl_ctx *ctx, GlTuneGradOp *q)
{
    GL_REQUIRE(ctx && q && q->out_guards && q->in[0] && q->out[0], "gl_tune_grad_op: NULL argument");
    gl_make_current(ctx);
    GL_REQUIRE(q->family >= 0 && q->family <= 2, "gl_tune_grad_op: family must be 0 (dcgan), 1 (pggan) or 2 (lpips)");
    constexpr int64_t G = 4096, kMax = 256ll << 20;
    for (int b = 0; b < 4; ++b) GL_REQUIRE(!q->in[b] || (q->in_bytes[b] > 0 && q->in_bytes[b] <= kMax), "gl_tune_grad_op: in_bytes[%d] out of range", b);
    for (int b = 0; b < 2; ++b) GL_REQUIRE(!q->out[b] || (q->out_bytes[b] > 0 && q->out_bytes[b] <= kMax), "gl_tune_grad_op: out_bytes[%d] out of range", b);
    GL_REQUIRE(q->copy_in < 4 && (q->copy_in < 0 || (q->in[q->copy_in] && q->in_bytes[q->copy_in] == q->out_bytes[0])),
               "gl_tune_grad_op: copy_in names no input of out[0]'s size");
    char *d_in[4] = {nullptr, nullptr, nullptr, nullptr}, *d_out[2] = {nullptr, nullptr};
    auto cleanup = [&]() {
        (void)hipStreamSynchronize(ctx->stream);
        for (int b = 0; b < 4; ++b) (void)hipFree(d_in[b]);
        for (int b = 0; b < 2; ++b) (void)hipFree(d_out[b]);
    };
#define TUNE_HIP(e) do { if ((e) != hipSuccess) { gl_set_error("gl_tune_grad_op: %s failed", #e); cleanup(); return GL_ERR_HIP; } } while (0)
#define TUNE_RC(e) do { const int rc_ = (e); if (rc_ != GL_OK) { cleanup(); return rc_; } } while (0)
    std::vector<float> gf((size_t)(G / 4), q->poison);
    void *k_in[4] = {nullptr, nullptr, nullptr, nullptr}, *k_out[2] = {nullptr, nullptr};
    for (int b = 0; b < 4; ++b) {
        if (!q->in[b]) continue;
        TUNE_HIP(hipMalloc((void **)&d_in[b], (size_t)(q->in_bytes[b] + 2 * G)));
        TUNE_HIP(hipMemcpy(d_in[b], gf.data(), (size_t)G, hipMemcpyHostToDevice));
        TUNE_HIP(hipMemcpy(d_in[b] + G, q->in[b], (size_t)q->in_bytes[b], hipMemcpyHostToDevice));
        TUNE_HIP(hipMemcpy(d_in[b] + G + q->in_bytes[b], gf.data(), (size_t)G, hipMemcpyHostToDevice));
        k_in[b] = d_in[b] + G;
    }
    for (int b = 0; b < 2; ++b) {
        if (!q->out[b]) continue;
        TUNE_HIP(hipMalloc((void **)&d_out[b], (size_t)(q->out_bytes[b] + 2 * G)));
        TUNE_HIP(hipMemset(d_out[b], q->sentinel & 0xFF, (size_t)(q->out_bytes[b] + 2 * G)));
        k_out[b] = d_out[b] + G;
    }
    if (q->copy_in >= 0) TUNE_HIP(hipMemcpy(d_out[0] + G, q->in[q->copy_in], (size_t)q->out_bytes[0], hipMemcpyHostToDevice));
    TUNE_HIP(hipDeviceSynchronize());
    int64_t nb[6];
    for (int b = 0; b < 4; ++b) nb[b] = q->in[b] ? q->in_bytes[b] : 0;
    for (int b = 0; b < 2; ++b) nb[4 + b] = q->out[b] ? q->out_bytes[b] : 0;
    if (q->family == 0) TUNE_RC(gl_tune_dcgan_grad_op(ctx, q->op, q->ip, nb, k_in, k_out));
    else if (q->family == 1) TUNE_RC(gl_tune_pggan_grad_op(ctx, q->op, q->ip, nb, &q->f0, k_in, k_out));
    else TUNE_RC(gl_tune_lpips_grad_op(ctx, q->op, q->ip, nb, k_in, k_out));
    TUNE_HIP(hipStreamSynchronize(ctx->stream));
    std::memset(q->out_guards, q->sentinel & 0xFF, (size_t)(4 * G));
    for (int b = 0; b < 2; ++b) {
        if (!q->out[b]) continue;
        char *og = reinterpret_cast<char *>(q->out_guards) + 2 * b * G;
        TUNE_HIP(hipMemcpy(og, d_out[b], (size_t)G, hipMemcpyDeviceToHost));
        TUNE_HIP(hipMemcpy(og + G, d_out[b] + G + q->out_bytes[b], (size_t)G, hipMemcpyDeviceToHost));
        TUNE_HIP(hipMemcpy(q->out[b], d_out[b] + G, (size_t)q->out_bytes[b], hipMemcpyDeviceToHost));
    }
#undef TUNE_HIP
#undef TUNE_RC
    cleanup();
    return GL_OK;
}
