// The selection half of a top-K search, shared by its two callers: the exact-integer L2 search (gl_topk.hip, pieces of S) and the l2-lpips
// search (gl_feat_count.hip, pieces of float bits).  Both store one slice of queries x bank rows as pieces [ceil(rows / 4)][queries][4] and
// have the same kernels (gl_topk.hip: topk_select_kernel, topk_merge_kernel) fold them into the [nq][k] key lists.
#pragma once
#include "gl_common.h"

// bytes one slice of pieces may occupy: gl_topk_set_workspace, else 1 GiB
size_t gl_topk_workspace_budget(const gl_ctx *ctx);
// the largest query extent of a slice (bounds the per-segment lists next to the pieces)
constexpr int64_t GL_TOPK_MAX_QUERY_SLICE = 65536;
// row segments the selection splits a slice of at most qs queries x rs bank rows into; the per-segment lists take segs * qs * k * 8 bytes
int64_t gl_topk_segments(int64_t qs, int64_t rs);
// pieces (elem = 4: uint32 values, 8: uint64) of nqs queries x nrs bank rows -> the k smallest keys (value << shift | index0 + n) per query,
// folded into dst[q][0..k), q < nqs.  lists: scratch of segs * nqs * k keys.  Two launches on the context's stream, GL_PROF_TOPK_SELECT.
int gl_topk_select_merge(gl_ctx *ctx, const void *pieces, int elem, int64_t nrs, int64_t nqs, int k, int shift, int64_t index0,
                         unsigned long long *dst, unsigned long long *lists, int64_t segs);

struct gl_scratch_guard {       // gl_free on every way out
    gl_ctx *ctx;
    void *p[2] = {nullptr, nullptr};
    ~gl_scratch_guard() { for (void *q : p) if (q) (void)gl_free(ctx, q); }
};
