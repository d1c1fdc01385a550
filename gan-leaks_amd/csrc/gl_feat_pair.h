// Constants and helpers shared by the pairwise kernels over LPIPS feature rows: the nearest-neighbour search (gl_lpips.hip: feat_knn_kernel,
// feat_knn_h1c_kernel, feat_knn_h1s_kernel) and the kernels that reduce the same fp32 distances differently (gl_feat_count.hip: epsilon-ball
// counts, stored distance matrix).  Both files must walk K in the same slices and segments: that is what makes a distance the same bits in all
// of them.
#pragma once
#include "gl_common.h"

namespace gl_feat_pair {

typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));

constexpr float kVScale = 16384.0f;     // V is stored as halves of V * 2^14 (values of 1e-4 .. 1e-1 stay out of the fp16 subnormals)

// split rows (feat_knn_kernel): tile 128 x 128, K slices of 32 values (128 bytes per row)
constexpr int FT = 128, FROW = 128, FOPER = FT * FROW;
constexpr int kSplitSeg = 2048;          // slices (of 32 values) per accumulation segment

// fp16 search rows (feat_knn_h1*_kernel): tile 256 x 256 on gl_pair256::mainloop
constexpr int GT = 256, GOPER = GT * FROW;
constexpr int kClusters = 8, kSuperN = 4, kSuperQ = 8;
constexpr int kSegSlices = 2048;                 // 128 Ki halves of K per segment
constexpr size_t kTotalsPerWg = 8 * 32 * 64 * sizeof(v4f);     // 256 KiB: 8 waves x 32 accumulator tiles x 64 lanes x 4 floats

__device__ __forceinline__ void cluster_meet(unsigned *counter, unsigned target)
{
    // one lane arrives and polls; the counter only orders time (L2 sharing), no memory is handed over
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int spin = 0; spin < 40000; ++spin) {
            if ((int)(__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) >= 0) break;
            __builtin_amdgcn_s_sleep(32);
        }
    }
    __syncthreads();
}

// logical tile id -> (bank tile, query tile) of the 256 x 256 kernels: strips of 4 bank tiles with the bank tile fastest
__device__ __forceinline__ void strip4_order(unsigned id, int q_tiles, int n_tiles, int &qt, int &nt)
{
    constexpr int STRIP = 4;
    const unsigned per_strip = (unsigned)STRIP * (unsigned)q_tiles;
    const int strip = (int)(id / per_strip);
    const unsigned r = id % per_strip;
    const int width = n_tiles - strip * STRIP < STRIP ? n_tiles - strip * STRIP : STRIP;
    nt = strip * STRIP + (int)(r % (unsigned)width);
    qt = (int)(r / (unsigned)width);
}

// workspace of the persistent kernels on the context: 4096 bytes of cluster counters, then kTotalsPerWg per workgroup
static inline int reserve_pair_scratch(gl_ctx *ctx, int grid)
{
    const size_t need = 4096 + (size_t)grid * kTotalsPerWg;
    if (ctx->pair_scratch_bytes < need) {
        GL_HIP(hipStreamSynchronize(ctx->stream));
        (void)hipFree(ctx->pair_scratch);
        ctx->pair_scratch = nullptr; ctx->pair_scratch_bytes = 0;
        GL_HIP(gl_device_alloc(ctx, (void **)&ctx->pair_scratch, need));
        ctx->pair_scratch_bytes = need;
    }
    return GL_OK;
}

}  // namespace gl_feat_pair
