// The pair tiles of the exact-integer kernels that reduce every query's row of S on the spot: the 128 x 128 tile (32-bit S, its 64-bit-total
// form and the wide form with int64 norms) and the 256 x 256 tile on gl_pair256::mainloop, each up to the point where the accumulators
// hold S, followed by the caller's epilogue.  Shared by the counting kernels with thresholds per query (gl_count_rows.hip) and the
// kernel-density sums (gl_kde.hip): one K loop per tile, whatever is reduced.
//
// epi.run<NI, ST>(s_of, n_left, q0, qcol0, q_left, tile_q, smem, lane): the arguments of gl_count::count_epilogue; NI 16-row groups of bank
// rows per wave, ST the unsigned type of S.  Every thread of the workgroup calls it, and the slice buffers are free after its first barrier.
#pragma once
#include "gl_common.h"
#include "gl_count_epi.h"
#include "gl_pair256.h"
#include <type_traits>

namespace gl_rows {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int TILE_N = 128;   // bank rows per workgroup
constexpr int TILE_Q = 128;   // queries per workgroup
constexpr int TILE_K = 128;   // bytes of K per slice
constexpr int THREADS = 256;
constexpr int OPER_BYTES = TILE_N * TILE_K;
constexpr int BT = 256;       // rows per operand of the 256 x 256 tile

using gl_count::rows_left;

// as in gl_topk.hip: 128 rows x 128 B per operand slice, 16-byte chunk c of row r at slot c ^ (r & 7)
__device__ __forceinline__ void stage_operand(const int8_t *__restrict__ base, int64_t row0, int64_t nrows_valid, int64_t stride, int64_t kbyte,
                                              char *lds_oper, int wave, int lane)
{
    const int rsub = lane >> 3, slot = lane & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int piece = wave * 4 + i;
        const int r = piece * 8 + rsub;
        int64_t gr = row0 + r;
        if (gr >= nrows_valid) gr = nrows_valid - 1;   // clamp: the epilogue masks rows beyond n_rows
        const int chunk = slot ^ (r & 7);
        gl_glds16(base + gr * stride + kbyte + chunk * 16, lds_oper + piece * 1024);
    }
}

__device__ __forceinline__ long long widen_norm(int32_t v) { return (long long)(unsigned)v; }   // int32 norms hold an unsigned value above d = 131071
__device__ __forceinline__ long long widen_norm(int64_t v) { return v; }

// The 128 x 128 tile (l2_count_i8_kernel of gl_count.hip up to S).  BIG = false: d <= 66051, everything modulo 2^32 (S < 2^32).  BIG = true: int32
// accumulators flushed into 64-bit totals every 64 KiB of K; NT = int32_t (d <= 262143) or int64_t (the wide form, d <= 2^24).
// smem: [2 buffers][bank 16 KiB | query 16 KiB].
template <bool BIG, typename NT, typename Epi>
__device__ __forceinline__ void tile128(const int8_t *__restrict__ bank, const NT *__restrict__ bank_norm, int64_t n_rows, const int8_t *__restrict__ query,
                                        const NT *__restrict__ query_norm, int64_t nq, int64_t stride, int q_tiles, int n_tiles, char *smem, const Epi &epi)
{
    typedef typename std::conditional<BIG, unsigned long long, unsigned>::type T;
    constexpr int FLUSH = 512;

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

    // ---- epilogue.  C layout of the 16x16 tile: column (query) = lane & 15, row (bank) = (lane >> 4) * 4 + reg.  S replaces the dot products in
    // place (exactly as the top-K epilogue forms it), so that no norm stays live next to the accumulators.
    const int64_t nbase = n0 + wn * 64 + fk * 4;
    const int n_left = rows_left(n_rows, nbase), q_left = rows_left(nq, q0);
    const NT *bnp = bank_norm + nbase, *qnp = query_norm + q0;
    NT qn[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ql = wq * 64 + j * 16 + frow;
        qn[j] = ql < q_left ? qnp[ql] : (NT)0;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const NT bn = i * 16 + r < n_left ? bnp[i * 16 + r] : (NT)0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (BIG) tot[i][j][r] = widen_norm(bn) + widen_norm(qn[j]) - 2ll * tot[i][j][r];
                else acc[i][j][r] = (int)((unsigned)bn + (unsigned)qn[j] - 2u * (unsigned)acc[i][j][r]);       // exact modulo 2^32, and S < 2^32
            }
        }
    auto s_of = [&](int i, int j, int r) -> T {
        if constexpr (BIG) return (unsigned long long)tot[i][j][r];
        else return (unsigned)acc[i][j][r];
    };
    epi.template run<4, T>(s_of, n_left, q0, wq * 64, q_left, TILE_Q, smem, lane);
}

// The 256 x 256 tile on the shared software-pipelined main loop (gl_pair256.h), d <= 66051.
template <typename Epi>
__device__ __forceinline__ void tile256(const int8_t *__restrict__ bank, const int32_t *__restrict__ bank_norm, int64_t n_rows, const int8_t *__restrict__ query,
                                        const int32_t *__restrict__ query_norm, int64_t nq, int64_t stride, int q_tiles, int n_tiles, char *smem, const Epi &epi)
{
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

    // S replaces the dot products in place (as above)
    const int64_t nbase = n0 + wn * 128 + fk * 4;
    const int n_left = rows_left(n_rows, nbase), q_left = rows_left(nq, q0);
    const int32_t *bnp = bank_norm + nbase, *qnp = query_norm + q0;
    unsigned qn[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ql = wq * 64 + j * 16 + frow;
        qn[j] = ql < q_left ? (unsigned)qnp[ql] : 0u;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned bn = i * 16 + r < n_left ? (unsigned)bnp[i * 16 + r] : 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j][r] = (int)(bn + qn[j] - 2u * (unsigned)acc[i][j][r]);   // exact modulo 2^32, and S < 2^32
        }
    auto s_of = [&](int i, int j, int r) -> unsigned { return (unsigned)acc[i][j][r]; };
    epi.template run<8, unsigned>(s_of, n_left, q0, wq * 64, q_left, BT, smem, lane);
}

}  // namespace gl_rows
