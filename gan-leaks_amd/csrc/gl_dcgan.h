// The DCGAN / WGAN-GP generator object behind the C ABI, shared by the forward (gl_dcgan.hip) and the gradient (gl_dcgan_grad.hip).
#pragma once
#include "gl_conv.h"
#include <vector>

struct gl_dcgan {
    gl_ctx *ctx;
    int z_dim, z_pad, nc, fg;
    int cin[5], cout[5];
    float *wpack[5];           // device, packed
    float *scale[4], *shift[4];
    float *bias_out;
    bool have_w[5], have_bn[4], have_bias;
    int64_t chunk, ws_chunk;   // requested / allocated images per pass
    float *ws_z, *ws_a[4];     // z padded; outputs of layers 0..3
    float *ws_p;               // scatter-form output of layer 4: [img][H*W][16 taps * nc]
    float *ident_scale, *ident_shift;   // epilogue constants (1, 0) for the layer-4 GEMM
    // optional self-attention on the output of layer 2 (VAEGAN: gan_models/vaegan/ops.py:86-120)
    bool have_att;
    float *att_w, *att_wsplit, *att_bias, *att_ones, *att_scale_h3, att_gamma;   // [q | k | v] 1x1 convolutions as one GEMM
    int att_cols, att_cols_pad, att_wexp;
    float *ws_att, *ws_qkv;
    // split-fp16 path (gl_conv_h3.hip): weights in the split layout scaled by 2^wexp, epilogue constants folded for it
    // optional spectral normalisation of layers 0..3 (VAEGAN: gan_models/vaegan/ops.py:23-75): w_bar as [C_in][C_out * 16], the power-iteration
    // state u [C_in], v [C_out * 16] and gamma / sqrt(var + eps) per output channel stay on the device; every forward advances u, v and
    // rewrites the epilogue scale as bn_scale / sigma
    bool have_sn[4];
    float *sn_w[4], *sn_u[4], *sn_v[4], *sn_wv[4], *sn_bns[4];
    int sn_iters;
    bool sn_hold;              // next forward(s) reuse the current sigma (a re-run of the same call)
    int precision;             // 0 = fp32 MFMA (exact fp32 products), 1 = split-fp16 (three fp16 MFMAs per product, ~22-bit operands)
    float *wsplit[5];
    bool fuse_tail;            // default on (gl_dcgan_set_fuse_tail)
    void *tail_w;              // layer 4 packed for the epilogue of layer 3 (gl_pack_tail_weights_host), when layer 3 has 64 or 128 channels
    int wexp[5];
    std::vector<float> h_scale[4], h_shift[4];
    float *scale_h3[5], *shift_h3[5];
    bool h3_dirty;
    // gradient with respect to z (gl_dcgan_grad.hip).  The raw weights stay on the host so that the transposed packs can be built on the first
    // gradient call; everything on the device below is allocated by that call and not before
    std::vector<float> h_w[5];   // [C_in][C_out][4][4] as given to gl_dcgan_set_conv_weight
    int64_t fwd_last_m;          // images of the most recent forward pass: what ws_a holds
    bool grad_dirty;             // a weight changed since gw was packed
    float *gw[5];                // transposed packs: layer 0 [z cols][16 C1], layers 1..3 [phase][C_in cols][4 taps x C_out], layer 4 [C_in cols][64]
    int64_t gws_chunk;           // images the gradient workspaces hold
    float *gws_y, *gws_g4, *gws_patch;   // kept fp32 output, cot * tanh', its 4 x 4 patches [pos][64]
    float *gws_da[4], *gws_gp[4];        // dL/da_l (NHWC, mirrors ws_a) and its masked, scaled, phase-planar form
    // backward of the attention block (gl_attention_grad.hip): the [q | k | v] 1x1 convolution weights as given ([2 C/8 + C][C], rows as att_w),
    // their transposed pack [C -> cols_pad][2 C/8 + C -> a multiple of 32], the rows [dq | dk | dv | 0] and the statistics (m, 1 / l, D) per position
    std::vector<float> h_att_w;
    float *gw_att, *gws_dqkv, *gws_att_stats;
};

// gl_attention_grad.hip: [dq | dk | dv | zero columns] rows of gl_attention_grad_cols(C) floats and [image][3][256] statistics from the forward's
// qkv rows and dY, the gradient with respect to the attention block's output
int gl_attention_grad_cols(int C);
int gl_launch_attention_grad(gl_ctx *ctx, int C, const float *qkv, const float *dY, float gamma, int64_t images, float *dqkv, float *stats);
