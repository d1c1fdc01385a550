// The LPIPS model's state, shared by the forward (gl_lpips.hip) and the image gradient of the distance (gl_lpips_grad.hip).
#pragma once
#include "gl_conv.h"
#include <vector>

constexpr int kLpNumConv = 13;          // VGG16's convolutions up to relu5_3
constexpr int kLpTaps = 5;

struct gl_lpips {
    gl_ctx *ctx;
    float *w[kLpNumConv];       // packed conv weights
    float *bias[kLpNumConv];
    float *ones;              // 512 ones (epilogue scale)
    float *lin[5];            // raw lin weights (host-checked >= 0)
    std::vector<float> lin_host[5];
    bool have_w[kLpNumConv], have_lin[5];
    // split-fp16 path: weights in the split layout scaled by 2^wexp, epilogue constants 2^-wexp and bias * kVggAct
    int precision;
    float *wsplit[kLpNumConv], *scale_h3[kLpNumConv], *bias_h3[kLpNumConv];
    int wexp[kLpNumConv];
    // the output of convolution i is stored as (value * act[i]) in the split layout; act[i] = 2^aexp[i], chosen per layer by a calibration
    // pass on fixed synthetic images the first time the split path runs (lp_calibrate), kVggAct before that.  Powers of two: a value's halves
    // only move in exponent, so wherever nothing clamps or falls into the fp16 subnormals the results do not depend on the choice.
    float act[kLpNumConv];
    std::vector<float> bias_host[kLpNumConv];
    bool calibrated, calibrate;
    unsigned *calib_max;      // device, kLpNumConv words: max |activation| per layer as float bits (set only during the calibration pass)
    // workspace for `chunk` images of H x W
    int64_t chunk, ws_imgs;
    int ws_H, ws_W;
    float *ws_a, *ws_b, *ws_coef;

    // ---- the image gradient (gl_lpips_grad.hip); everything below is built on the first gradient call and freed by gl_lpips_grad_free
    std::vector<float> w_host[kLpNumConv];      // raw weights [C_out][C_in][3][3] as gl_lpips_set_conv got them
    bool grad_dirty = true;                     // the packs below are older than the weights
    float *gw[kLpNumConv] = {};                 // conv >= 1: transposed, mirrored packs of the data gradient; conv 0: the raw weights
    float *g_lin = nullptr;                     // the five lin layers' weights, 1472 floats,
    std::vector<float> g_lin_host;              // and the values uploaded last
    float *keep[kLpNumConv] = {};               // kept activations (after ReLU) of a pass, NHWC
    float *keep_pool[4] = {};                   // their 2 x 2 max-pools: the inputs of conv 2, 4, 7, 10
    float *g_roll[2] = {};                      // rolling gradient buffers, the widest tensor of a pass each
    float *g_part = nullptr, *g_ref = nullptr;  // per-position loss terms of a pass; reference rows of a pass when the caller gave none
    int64_t g_imgs = 0;
    int g_H = 0, g_W = 0;
};

void gl_lpips_grad_free(gl_lpips *l);
