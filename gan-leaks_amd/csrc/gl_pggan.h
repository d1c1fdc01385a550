// The progressive-GAN generator object behind the C ABI, shared by the forward (gl_pggan.hip) and the gradient (gl_pggan_grad.hip).
#pragma once
#include "gl_conv.h"
#include <vector>

constexpr int kPgBlocks = 8;
constexpr int kPgLayers = 2 + 2 * kPgBlocks;   // ConvTranspose2d, initial WSConv3x3, two WSConv3x3 per block

struct gl_pggan {
    gl_ctx *ctx;
    int z_dim, z_pad, C, nc;
    int cin[kPgBlocks], cout[kPgBlocks];
    float *w_init, *b_init, *w_i3, *b_i3;
    float *w_blk[kPgBlocks][2], *b_blk[kPgBlocks][2];
    float *w_rgb[kPgBlocks + 1], *b_rgb[kPgBlocks + 1];
    bool have_init, have_blk[kPgBlocks], have_rgb[kPgBlocks + 1];
    float *ones;
    // split-fp16 path (precision 1): per convolution the weights in the split layout (* 2^wexp) and the folded epilogue constants
    int precision;
    struct H3 { float *w, *scale, *shift; } h_init, h_i3, h_blk[kPgBlocks][2], h_rgb[kPgBlocks + 1];
    int64_t chunk, ws_imgs;
    size_t ws_act_elems, ws_rgb_elems;      // floats allocated per activation / rgb buffer
    float *ws_z, *ws_buf[3], *ws_rgb[2];
    // gradient with respect to z (gl_pggan_grad.hip).  The raw weights stay on the host so that the transposed packs can be built on the first
    // gradient call; everything on the device below is allocated by that call and not before.
    // Layer numbering: 0 = ConvTranspose2d (kept after LeakyReLU, it has no PixelNorm), 1 = initial WSConv3x3, 2 + 2 s / 3 + 2 s = conv1 / conv2 of
    // block s (all kept after PixelNorm).
    std::vector<float> h_init_w;             // [z][C][4][4]
    std::vector<float> h_conv_w[kPgLayers];  // [1..]: [C_out][C_in][3][3]
    bool grad_dirty;                         // a weight changed since gw was packed
    float *gw[kPgLayers];                    // [0]: [K chunk][z cols][K chunk]; [l >= 1]: [chunk of C_out][C_in cols][9 mirrored taps x chunk], the input scale folded in
    // keep mode of the precision-0 forward: layer l's output goes to keep_act[l] instead of a rolling buffer and the PixelNorm factor of every
    // position to keep_inv[l]; the call must then fit one pass
    bool keep;
    float *keep_act[kPgLayers], *keep_inv[kPgLayers];
    int64_t gws_imgs;                        // images the gradient workspace below holds ...
    int gws_steps;                           // ... at this depth
    float *gws_y, *gws_g, *gws_roll[3];      // kept fp32 output, cot * tanh', rolling gradient buffers of the widest layer
};

// gl_pggan_grad.hip: releases the transposed packs and the gradient workspace (gl_pggan_destroy; the stream is idle)
void gl_pggan_grad_free(gl_pggan *g);
