// Exact top-K nearest neighbours under the integer L2 distance: the K smallest keys (S << shift | global index) of every query.
//
// One pass over the pairs, whatever K is ("emit S, then select"):
//   1. pairwise kernels: the K loops of gl_l2knn.hip (128 x 128 tile, its 64-bit-total and wide forms, and the 256 x 256 tile on
//      gl_pair256::mainloop) with an epilogue that STORES the exact S of every (query, row) pair instead of reducing it.  A lane owns,
//      per query column, runs of 4 consecutive bank rows; it writes each run as one piece [n / 4][query][4], so the 16 lanes of a
//      column group (16 consecutive queries) write one contiguous segment.  uint32 while S < 2^32 (d <= 66051), uint64 above.
//   2. topk_select_kernel: one thread per (query, row segment) reads its pieces (a wave reads 64 consecutive queries = one contiguous
//      run per piece row), forms the keys and keeps the k smallest in an LDS column; a candidate is compared with the current k-th key
//      first, and with the k-th key the destination already holds (earlier slices / chunks), so almost all of them cost one compare.
//   3. topk_merge_kernel folds the per-segment lists into the destination rows -- the same kernel gl_topk_merge runs on the lists
//      of the other ranks.
// Keys are unique and totally ordered (the global index is part of them), every compare is a compare of whole 64-bit keys, so the result
// depends on nothing but the set of (S, index) pairs: not on the tile, the slicing, the chunking or the sharding.
//
// Workspace: the S pieces of one slice of queries x bank rows, at most ctx->topk_budget bytes (1 GiB by default); the library walks the
// slices itself and the slice shape does not depend on k.
#include "gl_common.h"
#include "gl_pair256.h"
#include "gl_topk_sel.h"
#include <type_traits>

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int TILE_N = 128;   // bank rows per workgroup
constexpr int TILE_Q = 128;   // queries per workgroup
constexpr int TILE_K = 128;   // bytes of K per slice
constexpr int THREADS = 256;
constexpr int OPER_BYTES = TILE_N * TILE_K;
constexpr int BT = 256;     // rows per operand of the 256 x 256 tile
constexpr size_t DEFAULT_BUDGET = (size_t)1 << 30;
constexpr int64_t MAX_QUERY_SLICE = GL_TOPK_MAX_QUERY_SLICE;
constexpr int SEL_THREADS = 128;
constexpr int64_t SEL_TARGET_THREADS = 262144;   // 256 CUs x 1024 selection threads

template <typename T> struct alignas(16) piece4 { T v[4]; };

// as in gl_l2knn.hip: 128 rows x 128 B per operand slice, 16-byte chunk c of row r at slot c ^ (r & 7)
__device__ __forceinline__ void stage_operand(const int8_t *__restrict__ base, int64_t row0, int64_t nrows_valid, int64_t stride, int64_t kbyte,
                                              char *lds_oper, int wave, int lane)
{
    const int rsub = lane >> 3, slot = lane & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int piece = wave * 4 + i;
        const int r = piece * 8 + rsub;
        int64_t gr = row0 + r;
        if (gr >= nrows_valid) gr = nrows_valid - 1;   // clamp: the selection masks rows beyond n_rows
        const int chunk = slot ^ (r & 7);
        gl_glds16(base + gr * stride + kbyte + chunk * 16, lds_oper + piece * 1024);
    }
}

__device__ __forceinline__ long long widen_norm(int32_t v) { return (long long)(unsigned)v; }   // int32 norms hold an unsigned value above d = 131071
__device__ __forceinline__ long long widen_norm(int64_t v) { return v; }

// The 128 x 128 tile.  BIG = false: d <= 66051, everything modulo 2^32 (S < 2^32), S stored as uint32.  BIG = true: int32 accumulators flushed
// into 64-bit totals every 64 KiB of K, S stored as uint64; NT = int32_t (d <= 262143) or int64_t (the wide form, d <= 2^24).
// out: [ceil(n_rows / 4)][nq][4] values of S; pieces that start at or beyond n_rows and queries beyond nq are not written.
template <bool BIG, typename NT>
__global__ void __launch_bounds__(THREADS, 2)
l2_topk_i8_kernel(const int8_t *__restrict__ bank, const NT *__restrict__ bank_norm, int64_t n_rows,
                  const int8_t *__restrict__ query, const NT *__restrict__ query_norm, int64_t nq, int64_t stride,
                  typename std::conditional<BIG, unsigned long long, unsigned>::type *__restrict__ out, int q_tiles, int n_tiles)
{
    typedef typename std::conditional<BIG, unsigned long long, unsigned>::type T;
    constexpr int FLUSH = 512;
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 buffers][bank 16 KiB | query 16 KiB]

    const unsigned nwg = (unsigned)q_tiles * (unsigned)n_tiles;
    const unsigned id = gl_xcd_remap(blockIdx.x, nwg);
    int qt, nt;
    gl_strip_order(id, q_tiles, n_tiles, qt, nt);
    const int64_t n0 = (int64_t)nt * TILE_N, q0 = (int64_t)qt * TILE_Q;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave >> 1, wq = wave & 1;
    const int frow = lane & 15, fk = lane >> 4;

    v4i acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (v4i){0, 0, 0, 0};
    long long tot[BIG ? 4 : 1][BIG ? 4 : 1][4] = {};
    auto flush = [&]() {
        if constexpr (BIG) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) { tot[i][j][r] += (long long)acc[i][j][r]; acc[i][j][r] = 0; }
        }
    };

    const int nk = (int)(stride / TILE_K);
    stage_operand(bank, n0, n_rows, stride, 0, smem, wave, lane);
    stage_operand(query, q0, nq, stride, 0, smem + OPER_BYTES, wave, lane);

    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();   // slice kt landed; everyone is done reading the other buffer
        char *cur = smem + (kt & 1) * 2 * OPER_BYTES;
        if (kt + 1 < nk) {
            char *nxt = smem + ((kt + 1) & 1) * 2 * OPER_BYTES;
            stage_operand(bank, n0, n_rows, stride, (int64_t)(kt + 1) * TILE_K, nxt, wave, lane);
            stage_operand(query, q0, nq, stride, (int64_t)(kt + 1) * TILE_K, nxt + OPER_BYTES, wave, lane);
        }
        const char *lb = cur + (wn * 64) * TILE_K;
        const char *lq = cur + OPER_BYTES + (wq * 64) * TILE_K;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int chunk = ks * 4 + fk;
            v4i a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = i * 16 + frow;
                a[i] = *reinterpret_cast<const v4i *>(lb + r * TILE_K + ((chunk ^ (r & 7)) << 4));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = j * 16 + frow;
                b[j] = *reinterpret_cast<const v4i *>(lq + r * TILE_K + ((chunk ^ (r & 7)) << 4));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (BIG && (kt % FLUSH) == FLUSH - 1) flush();
    }
    flush();

    // ---- epilogue.  C layout of the 16x16 tile: column (query) = lane & 15, row (bank) = (lane >> 4) * 4 + reg: the 4 registers of an
    // accumulator are 4 consecutive bank rows of one query = one piece.
    const int64_t nbase = n0 + wn * 64 + fk * 4;
    NT bn[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t n = nbase + i * 16 + r;
            bn[i][r] = n < n_rows ? bank_norm[n] : (NT)0;
        }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t q = q0 + wq * 64 + j * 16 + frow;
        const NT qn = q < nq ? query_norm[q] : (NT)0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t n4 = nbase + i * 16;
            piece4<T> p;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if constexpr (BIG) p.v[r] = (unsigned long long)(widen_norm(bn[i][r]) + widen_norm(qn) - 2ll * tot[i][j][r]);
                else p.v[r] = (unsigned)bn[i][r] + (unsigned)qn - 2u * (unsigned)acc[i][j][r];       // exact modulo 2^32, and S < 2^32
            }
            if (q < nq && n4 < n_rows) *reinterpret_cast<piece4<T> *>(out + ((n4 >> 2) * nq + q) * 4) = p;
        }
    }
}

// The 256 x 256 tile on the shared software-pipelined main loop (gl_pair256.h), d <= 66051; same output layout, uint32.
__global__ void __launch_bounds__(512, 2)
l2_topk_i8_256p_kernel(const int8_t *__restrict__ bank, const int32_t *__restrict__ bank_norm, int64_t n_rows,
                       const int8_t *__restrict__ query, const int32_t *__restrict__ query_norm, int64_t nq, int64_t stride,
                       unsigned *__restrict__ out, int q_tiles, int n_tiles)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const unsigned id = gl_xcd_remap(blockIdx.x, (unsigned)q_tiles * (unsigned)n_tiles);
    int qt, nt;
    {
        constexpr int STRIP = 4;
        const unsigned per_strip = (unsigned)STRIP * (unsigned)q_tiles;
        const int strip = (int)(id / per_strip);
        const unsigned r = id % per_strip;
        const int width = n_tiles - strip * STRIP < STRIP ? n_tiles - strip * STRIP : STRIP;
        nt = strip * STRIP + (int)(r % (unsigned)width);
        qt = (int)(r / (unsigned)width);
    }
    const int64_t n0 = (int64_t)nt * BT, q0 = (int64_t)qt * BT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave >> 2, wq = wave & 3;
    const int frow = lane & 15, fk = lane >> 4;

    const gl_pair256::Source sa = gl_pair256::make_source(reinterpret_cast<const char *>(bank), n0, n_rows, stride, wave, lane);
    const gl_pair256::Source sb = gl_pair256::make_source(reinterpret_cast<const char *>(query), q0, nq, stride, wave, lane);
    v4i acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (v4i){0, 0, 0, 0};
    gl_pair256::mainloop<v4i, 0, 8>(sa, sb, stride / TILE_K, smem, acc, wave, lane,
                              [](const v4i &a, const v4i &b, const v4i &c) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0); });

    const int64_t nbase = n0 + wn * 128 + fk * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t q = q0 + wq * 64 + j * 16 + frow;
        const unsigned qn = q < nq ? (unsigned)query_norm[q] : 0u;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int64_t n4 = nbase + i * 16;
            piece4<unsigned> p;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t n = n4 + r;
                const unsigned bn = n < n_rows ? (unsigned)bank_norm[n] : 0u;
                p.v[r] = bn + qn - 2u * (unsigned)acc[i][j][r];       // exact modulo 2^32, and S < 2^32
            }
            if (q < nq && n4 < n_rows) *reinterpret_cast<piece4<unsigned> *>(out + ((n4 >> 2) * nq + q) * 4) = p;
        }
    }
}

// A thread's ascending list of k keys is column `tid` of an LDS array [k][blockDim.x] (conflict-free: a wave touches one row at a time).
// insert(): the caller has found key smaller than the last entry, which drops out.
struct lds_list {
    unsigned long long *col;   // &lst[tid]
    int k, pitch;
    __device__ __forceinline__ unsigned long long get(int j) const { return col[j * pitch]; }
    __device__ __forceinline__ void set(int j, unsigned long long v) { col[j * pitch] = v; }
    __device__ __forceinline__ void insert(unsigned long long key)
    {
        int j = k - 1;
        while (j > 0) {
            const unsigned long long above = get(j - 1);
            if (above <= key) break;
            set(j, above);
            --j;
        }
        set(j, key);
    }
};

// S pieces [ceil(n_rows / 4)][nq][4] -> lists[seg][q][0..k): the k smallest keys (S << shift | index0 + n) among the rows of segment
// `seg` = blockIdx.y that are below the k-th key dst[q][k-1] already holds (keys at or above it cannot enter the result); ~0 fills the rest.
template <typename T>
__global__ void __launch_bounds__(SEL_THREADS)
topk_select_kernel(const T *__restrict__ pieces, int64_t n_rows, int64_t nq, int k, int shift, int64_t index0,
                   const unsigned long long *__restrict__ dst, unsigned long long *__restrict__ lists)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long lst[];
    const int tid = threadIdx.x;
    const int64_t q = (int64_t)blockIdx.x * SEL_THREADS + tid;
    if (q >= nq) return;                                  // no barrier below: every thread works on its own column
    lds_list L = {lst + tid, k, SEL_THREADS};
    for (int j = 0; j < k; ++j) L.set(j, ~0ull);
    const unsigned long long floor_key = dst[q * k + (k - 1)];
    unsigned long long thr = floor_key;

    const int64_t groups = (n_rows + 3) >> 2;
    const int64_t g_lo = groups * blockIdx.y / gridDim.y, g_hi = groups * (blockIdx.y + 1) / gridDim.y;
    const piece4<T> *src = reinterpret_cast<const piece4<T> *>(pieces) + q;
    auto take = [&](int64_t g, const piece4<T> &p) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t n = g * 4 + r;
            const unsigned long long key = ((unsigned long long)p.v[r] << shift) | (unsigned long long)(index0 + n);
            if (n < n_rows && key < thr) {
                L.insert(key);
                const unsigned long long last = L.get(k - 1);
                thr = last < floor_key ? last : floor_key;
            }
        }
    };
    constexpr int U = 4;                                  // loads in flight per thread
    int64_t g = g_lo;
    for (; g + U <= g_hi; g += U) {
        piece4<T> p[U];
#pragma unroll
        for (int u = 0; u < U; ++u) p[u] = src[(g + u) * nq];
#pragma unroll
        for (int u = 0; u < U; ++u) take(g + u, p[u]);
    }
    for (; g < g_hi; ++g) take(g, src[g * nq]);

    unsigned long long *o = lists + ((int64_t)blockIdx.y * nq + q) * k;
    for (int j = 0; j < k; ++j) o[j] = L.get(j);
}

// dst[q][0..k) = the k smallest of dst[q] and src[l][q][0..k), l < n_lists (all lists ascending, ~0 = empty slot); list l of src starts at
// src + l * list_stride.
__global__ void __launch_bounds__(SEL_THREADS)
topk_merge_kernel(unsigned long long *__restrict__ dst, const unsigned long long *__restrict__ src, int64_t list_stride, int64_t nq, int k,
                  int64_t n_lists)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long lst[];
    const int tid = threadIdx.x;
    const int64_t q = (int64_t)blockIdx.x * SEL_THREADS + tid;
    if (q >= nq) return;
    lds_list L = {lst + tid, k, SEL_THREADS};
    for (int j = 0; j < k; ++j) L.set(j, dst[q * k + j]);
    unsigned long long thr = L.get(k - 1);
    for (int64_t l = 0; l < n_lists; ++l) {
        const unsigned long long *s = src + l * list_stride + q * k;
        for (int j = 0; j < k; ++j) {
            const unsigned long long key = s[j];
            if (key >= thr) break;                        // ascending: nothing further in this list can enter (empty slots are ~0)
            L.insert(key);
            thr = L.get(k - 1);
        }
    }
    for (int j = 0; j < k; ++j) dst[q * k + j] = L.get(j);
}

template <bool INT>
__global__ void __launch_bounds__(256) topk_unpack_kernel(const uint64_t *__restrict__ keys, int64_t count, double scale, int shift,
                                                          float *__restrict__ dist, int64_t *__restrict__ idx)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint64_t key = keys[i];
    if (key == ~0ull) {                                   // empty slot: fewer than k rows were searched
        dist[i] = __builtin_inff();
        idx[i] = -1;
        return;
    }
    dist[i] = INT ? (float)((double)(key >> shift) / scale) : (float)((double)(key >> shift) * scale);   // the expression of keys_unpack_kernel
    idx[i] = (int64_t)(key & ((1ull << shift) - 1ull));
}

// keys of the l2-lpips top-K (gl_feat_topk*): float bits << 32 | global index
__global__ void __launch_bounds__(256) topk_unpack_f32_kernel(const uint64_t *__restrict__ keys, int64_t count, float *__restrict__ dist,
                                                              int64_t *__restrict__ idx)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint64_t key = keys[i];
    if (key == ~0ull) {
        dist[i] = __builtin_inff();
        idx[i] = -1;
        return;
    }
    dist[i] = __uint_as_float((unsigned)(key >> 32));
    idx[i] = (int64_t)(key & 0xFFFFFFFFull);
}

}  // namespace

size_t gl_topk_workspace_budget(const gl_ctx *ctx) { return ctx->topk_budget ? ctx->topk_budget : DEFAULT_BUDGET; }

int64_t gl_topk_segments(int64_t qs, int64_t rs)
{
    const int64_t groups = gl_ceil_div(rs, 4);
    int64_t segs = gl_ceil_div(SEL_TARGET_THREADS, qs);
    if (segs > groups / 16) segs = groups / 16;
    if (segs > 64) segs = 64;
    if (segs < 1) segs = 1;
    return segs;
}

int gl_topk_select_merge(gl_ctx *ctx, const void *pieces, int elem, int64_t nrs, int64_t nqs, int k, int shift, int64_t index0,
                         unsigned long long *dst, unsigned long long *lists, int64_t segs)
{
    gl_prof_scope prof_(ctx, GL_PROF_TOPK_SELECT);
    const dim3 sel_grid((unsigned)gl_ceil_div(nqs, SEL_THREADS), (unsigned)segs);
    const size_t sel_lds = (size_t)SEL_THREADS * k * 8;
    if (elem == 8)
        hipLaunchKernelGGL(topk_select_kernel<unsigned long long>, sel_grid, dim3(SEL_THREADS), sel_lds, ctx->stream,
                           static_cast<const unsigned long long *>(pieces), nrs, nqs, k, shift, index0, dst, lists);
    else
        hipLaunchKernelGGL(topk_select_kernel<unsigned>, sel_grid, dim3(SEL_THREADS), sel_lds, ctx->stream, static_cast<const unsigned *>(pieces),
                           nrs, nqs, k, shift, index0, dst, lists);
    GL_LAUNCH_CHECK();
    hipLaunchKernelGGL(topk_merge_kernel, dim3(sel_grid.x), dim3(SEL_THREADS), sel_lds, ctx->stream, dst, lists, nqs * k, nqs, k, segs);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

namespace {

template <typename NT>
int topk_impl(const char *fn, gl_ctx *ctx, const int8_t *bank, const NT *bank_norm, int64_t n_rows, int64_t index_base, const int8_t *query,
              const NT *query_norm, int64_t nq, int64_t d, int k, uint64_t *topk)
{
    constexpr bool WIDE = sizeof(NT) == 8;
    const int64_t max_d = WIDE ? GL_L2_WIDE_MAX_D : GL_L2_MAX_D;
    gl_make_current(ctx);
    GL_REQUIRE(ctx, "%s: NULL ctx", fn);
    GL_REQUIRE(n_rows >= 0 && nq >= 0 && d > 0 && d <= max_d, "%s: bad sizes n_rows=%lld nq=%lld d=%lld (d <= %lld)", fn, (long long)n_rows,
               (long long)nq, (long long)d, (long long)max_d);
    GL_REQUIRE(k >= 1 && k <= GL_TOPK_MAX, "%s: k=%d outside [1, %d]", fn, k, GL_TOPK_MAX);
    const int shift = gl_l2_key_shift(d);
    GL_REQUIRE(index_base >= 0 && index_base + n_rows <= (1ll << shift), "%s: global index does not fit the %d index bits of a key at d=%lld", fn, shift,
               (long long)d);
    if (n_rows == 0 || nq == 0) return GL_OK;
    GL_REQUIRE(bank && bank_norm && query && query_norm && topk, "%s: NULL device pointer", fn);
    GL_REQUIRE(((reinterpret_cast<uintptr_t>(bank) | reinterpret_cast<uintptr_t>(query)) & 15) == 0, "%s: prepared rows must be 16-byte aligned", fn);
    GL_REQUIRE((reinterpret_cast<uintptr_t>(topk) & 7) == 0, "%s: the key lists must be 8-byte aligned", fn);
    const int64_t stride = gl_l2_row_stride(d);
    const bool big = WIDE || d > 66051;                  // 65025 * 66051 < 2^32
    // the tile gl_l2_knn_i8 would take for the whole call; every slice uses it
    const int force_tile = gl_tuning_int("GL_L2_TILE", 0);
    const bool t256 = !big && force_tile != 128 && (force_tile == 256 || gl_ceil_div(nq, BT) * gl_ceil_div(n_rows, BT) >= 1024);
    const int64_t tile = t256 ? BT : TILE_N;
    const int64_t elem = big ? 8 : 4;

    // slices: qs queries x rs bank rows of S values within the budget, both multiples of the tile (or the whole extent)
    const int64_t budget = (int64_t)gl_topk_workspace_budget(ctx);
    int64_t qs = budget / (tile * elem) / tile * tile;
    if (qs < tile) qs = tile;
    if (qs > MAX_QUERY_SLICE) qs = MAX_QUERY_SLICE;
    if (qs > nq) qs = nq;
    int64_t rs = budget / (qs * elem) / tile * tile;
    if (rs < tile) rs = tile;
    if (rs > n_rows) rs = n_rows;
    const int64_t groups = gl_ceil_div(rs, 4);
    const int64_t segs = gl_topk_segments(qs, rs);

    gl_scratch_guard mem{ctx};
    int rc = gl_malloc(ctx, (size_t)(groups * qs * 4 * elem), &mem.p[0]);
    if (rc != GL_OK) return rc;
    rc = gl_malloc(ctx, (size_t)(segs * qs * k * 8), &mem.p[1]);
    if (rc != GL_OK) return rc;
    unsigned long long *lists = static_cast<unsigned long long *>(mem.p[1]);
    unsigned long long *dst = reinterpret_cast<unsigned long long *>(topk);

    const int lds128 = 4 * OPER_BYTES;
    GL_ONCE_PER_DEVICE(ctx, \
        GL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(l2_topk_i8_kernel<false, int32_t>), hipFuncAttributeMaxDynamicSharedMemorySize, lds128)); \
        GL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(l2_topk_i8_kernel<true, int32_t>), hipFuncAttributeMaxDynamicSharedMemorySize, lds128)); \
        GL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(l2_topk_i8_kernel<true, int64_t>), hipFuncAttributeMaxDynamicSharedMemorySize, lds128)); \
        GL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(l2_topk_i8_256p_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, gl_pair256::LDS_BYTES)););

    for (int64_t q_lo = 0; q_lo < nq; q_lo += qs) {
        const int64_t nqs = nq - q_lo < qs ? nq - q_lo : qs;
        const int8_t *qrows = query + q_lo * stride;
        const NT *qnorm = query_norm + q_lo;
        unsigned long long *qdst = dst + q_lo * k;
        for (int64_t r_lo = 0; r_lo < n_rows; r_lo += rs) {
            const int64_t nrs = n_rows - r_lo < rs ? n_rows - r_lo : rs;
            const int8_t *brows = bank + r_lo * stride;
            const NT *bnorm = bank_norm + r_lo;
            const int64_t qt = gl_ceil_div(nqs, tile), nt = gl_ceil_div(nrs, tile);
            GL_REQUIRE(qt * nt < (1ll << 31), "%s: grid too large", fn);
            {
                gl_prof_scope prof_(ctx, GL_PROF_L2_KNN);
                if constexpr (!WIDE) {
                    if (t256)
                        hipLaunchKernelGGL(l2_topk_i8_256p_kernel, dim3((unsigned)(qt * nt)), dim3(512), gl_pair256::LDS_BYTES, ctx->stream, brows, bnorm, nrs,
                                           qrows, qnorm, nqs, stride, static_cast<unsigned *>(mem.p[0]), (int)qt, (int)nt);
                    else if (!big)
                        hipLaunchKernelGGL((l2_topk_i8_kernel<false, int32_t>), dim3((unsigned)(qt * nt)), dim3(THREADS), lds128, ctx->stream, brows, bnorm, nrs,
                                           qrows, qnorm, nqs, stride, static_cast<unsigned *>(mem.p[0]), (int)qt, (int)nt);
                    else
                        hipLaunchKernelGGL((l2_topk_i8_kernel<true, int32_t>), dim3((unsigned)(qt * nt)), dim3(THREADS), lds128, ctx->stream, brows, bnorm, nrs,
                                           qrows, qnorm, nqs, stride, static_cast<unsigned long long *>(mem.p[0]), (int)qt, (int)nt);
                } else {
                    hipLaunchKernelGGL((l2_topk_i8_kernel<true, int64_t>), dim3((unsigned)(qt * nt)), dim3(THREADS), lds128, ctx->stream, brows, bnorm, nrs,
                                       qrows, qnorm, nqs, stride, static_cast<unsigned long long *>(mem.p[0]), (int)qt, (int)nt);
                }
                GL_LAUNCH_CHECK();
            }
            if (const int rc = gl_topk_select_merge(ctx, mem.p[0], (int)elem, nrs, nqs, k, shift, index_base + r_lo, qdst, lists, segs)) return rc;
        }
    }
    return GL_OK;
}

}  // namespace

extern "C" {

int gl_topk_set_workspace(gl_ctx *ctx, size_t bytes)
{
    GL_REQUIRE(ctx, "gl_topk_set_workspace: NULL ctx");
    ctx->topk_budget = bytes;
    return GL_OK;
}

int gl_topk_init(gl_ctx *ctx, uint64_t *topk_keys_dev, int64_t nq, int k)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx && nq >= 0, "gl_topk_init: bad ctx/nq");
    GL_REQUIRE(k >= 1 && k <= GL_TOPK_MAX, "gl_topk_init: k=%d outside [1, %d]", k, GL_TOPK_MAX);
    if (nq == 0) return GL_OK;
    GL_REQUIRE(topk_keys_dev, "gl_topk_init: NULL keys");
    GL_HIP(hipMemsetAsync(topk_keys_dev, 0xFF, (size_t)nq * k * 8, ctx->stream));
    return GL_OK;
}

int gl_l2_topk_i8(gl_ctx *ctx, const int8_t *bank_i8_dev, const int32_t *bank_norm_dev, int64_t n_rows, int64_t index_base,
                  const int8_t *query_i8_dev, const int32_t *query_norm_dev, int64_t nq, int64_t d, int k, uint64_t *topk_keys_dev)
{
    return topk_impl<int32_t>("gl_l2_topk_i8", ctx, bank_i8_dev, bank_norm_dev, n_rows, index_base, query_i8_dev, query_norm_dev, nq, d, k, topk_keys_dev);
}

int gl_l2_topk_i8_wide(gl_ctx *ctx, const int8_t *bank_i8_dev, const int64_t *bank_norm_dev, int64_t n_rows, int64_t index_base,
                       const int8_t *query_i8_dev, const int64_t *query_norm_dev, int64_t nq, int64_t d, int k, uint64_t *topk_keys_dev)
{
    return topk_impl<int64_t>("gl_l2_topk_i8_wide", ctx, bank_i8_dev, bank_norm_dev, n_rows, index_base, query_i8_dev, query_norm_dev, nq, d, k,
                              topk_keys_dev);
}

int gl_topk_merge(gl_ctx *ctx, uint64_t *dst_dev, const uint64_t *src_dev, int64_t nq, int k, int64_t n_lists)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx && nq >= 0 && n_lists >= 0, "gl_topk_merge: bad ctx/nq/n_lists");
    GL_REQUIRE(k >= 1 && k <= GL_TOPK_MAX, "gl_topk_merge: k=%d outside [1, %d]", k, GL_TOPK_MAX);
    if (nq == 0 || n_lists == 0) return GL_OK;
    GL_REQUIRE(dst_dev && src_dev, "gl_topk_merge: NULL device pointer");
    GL_REQUIRE(((reinterpret_cast<uintptr_t>(dst_dev) | reinterpret_cast<uintptr_t>(src_dev)) & 7) == 0, "gl_topk_merge: the key lists must be 8-byte aligned");
    gl_prof_scope prof_(ctx, GL_PROF_TOPK_SELECT);
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)gl_ceil_div(nq, SEL_THREADS)), dim3(SEL_THREADS), (size_t)SEL_THREADS * k * 8, ctx->stream,
                       reinterpret_cast<unsigned long long *>(dst_dev), reinterpret_cast<const unsigned long long *>(src_dev), nq * k, nq, k, n_lists);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int gl_topk_unpack(gl_ctx *ctx, const uint64_t *topk_keys_dev, int64_t nq, int k, int64_t d, int integers, float *dist_dev, int64_t *idx_dev)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx && nq >= 0 && d > 0, "gl_topk_unpack: bad ctx/nq/d");
    GL_REQUIRE(k >= 1 && k <= GL_TOPK_MAX, "gl_topk_unpack: k=%d outside [1, %d]", k, GL_TOPK_MAX);
    if (nq == 0) return GL_OK;
    GL_REQUIRE(topk_keys_dev && dist_dev && idx_dev, "gl_topk_unpack: NULL device pointer");
    const int64_t count = nq * k;
    const dim3 grid((unsigned)gl_ceil_div(count, 256));
    if (integers)
        hipLaunchKernelGGL(topk_unpack_kernel<true>, grid, dim3(256), 0, ctx->stream, topk_keys_dev, count, (double)d, gl_l2_key_shift(d), dist_dev, idx_dev);
    else
        hipLaunchKernelGGL(topk_unpack_kernel<false>, grid, dim3(256), 0, ctx->stream, topk_keys_dev, count, 4.0 / (65025.0 * (double)d), gl_l2_key_shift(d),
                           dist_dev, idx_dev);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int gl_topk_unpack_f32(gl_ctx *ctx, const uint64_t *topk_keys_dev, int64_t nq, int k, float *dist_dev, int64_t *idx_dev)
{
    gl_make_current(ctx);
    GL_REQUIRE(ctx && nq >= 0, "gl_topk_unpack_f32: bad ctx/nq");
    GL_REQUIRE(k >= 1 && k <= GL_TOPK_MAX, "gl_topk_unpack_f32: k=%d outside [1, %d]", k, GL_TOPK_MAX);
    if (nq == 0) return GL_OK;
    GL_REQUIRE(topk_keys_dev && dist_dev && idx_dev, "gl_topk_unpack_f32: NULL device pointer");
    const int64_t count = nq * k;
    hipLaunchKernelGGL(topk_unpack_f32_kernel, dim3((unsigned)gl_ceil_div(count, 256)), dim3(256), 0, ctx->stream, topk_keys_dev, count, dist_dev, idx_dev);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

}  // extern "C"
