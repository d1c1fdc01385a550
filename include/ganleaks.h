/* ganleaks.h -- C ABI of libganleaks_hip.so (MI355X / gfx950).
 *
 * The reference (CarloSaccardi/GAN-Leaks) is pure Python and has no FFI of its own; the drop-in
 * boundary for its full-black-box attack path is the set of Python call signatures listed in
 * SURVEY.md 8(b).  Each entry point below names the reference interface it stands behind
 * (file:line relative to the reference tree).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - every function returns 0 on success, a negative gl_status on failure and never throws;
 *     gl_last_error() returns a thread-local, NUL-terminated description of the last failure.
 *   - plain pointers and sizes only.  Pointers named *_dev are DEVICE pointers (hipMalloc'd by the
 *     caller, by gl_malloc, or by PyTorch-ROCm: tensor.data_ptr()); *_host are host pointers.
 *   - one gl_ctx per GPU per host thread; all work of a context is enqueued on its HIP stream
 *     (private by default, or the caller's via gl_ctx_set_stream) and is asynchronous unless the
 *     function says it synchronises.
 *   - image rows are C-contiguous [count][D] with D = C*H*W in the reference's NCHW order
 *     (attack_models/fbb.py:134-135).
 */
#ifndef GANLEAKS_H
#define GANLEAKS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GL_ABI_VERSION 1

typedef enum gl_status {
    GL_OK = 0,
    GL_ERR_INVALID = -1,   /* bad argument (NULL, negative size, unsupported shape) */
    GL_ERR_HIP = -2,       /* a HIP runtime call failed */
    GL_ERR_NO_DEVICE = -3, /* no usable gfx950 device */
    GL_ERR_STATE = -4,     /* object not ready (weights missing, bank not set) */
    GL_ERR_EMPTY_BANK = -5,/* bank shorter than one BATCH_SIZE: reference raises ValueError at fbb.py:83 */
    GL_ERR_RCCL = -6       /* librccl missing, or an RCCL call failed (gl_comm_*) */
} gl_status;

typedef struct gl_ctx gl_ctx;       /* opaque: device + stream + scratch */
typedef struct gl_dcgan gl_dcgan;   /* opaque: packed DCGAN / WGAN-GP generator */
typedef struct gl_lpips gl_lpips;   /* opaque: VGG16 + LPIPS v0.1 lin layers */
typedef struct gl_pggan gl_pggan;   /* opaque: packed progressive-GAN generator */
typedef struct gl_medgan gl_medgan; /* opaque: medGAN residual-MLP generator + autoencoder decoder */
typedef struct gl_vaegan_enc gl_vaegan_enc; /* opaque: VAEGAN encoder (four strided convolutions + two heads) */
typedef struct gl_comm gl_comm;     /* opaque: one rank of an RCCL communicator, bound to a gl_ctx */

/* ---------------------------------------------------------------- library / context */
int gl_abi_version(void);
const char *gl_last_error(void);
int gl_device_count(int *out_count);
int gl_ctx_create(int device, gl_ctx **out_ctx);           /* replaces `device = torch.device("cuda")`, fbb.py:40 */
int gl_ctx_destroy(gl_ctx *ctx);
int gl_ctx_set_stream(gl_ctx *ctx, void *hip_stream);      /* NULL restores the private stream */
int gl_ctx_get_stream(gl_ctx *ctx, void **out_hip_stream);
int gl_ctx_sync(gl_ctx *ctx);                              /* hipStreamSynchronize */

/* split-fp16 kernels store activations as fp16 halves of (value * 2^k); a value beyond the fp16 range is clamped and counted.
 * Returns (and resets) the number of workgroups that clamped since the last call; synchronises.  Non-zero means the result of
 * the split path is not trustworthy for these weights: rerun with gl_*_set_precision(.., 0). */
int gl_ctx_h3_saturations(gl_ctx *ctx, int64_t *out_count);

/* device memory + copies (synchronous w.r.t. the context stream) */
int gl_malloc(gl_ctx *ctx, size_t bytes, void **out_dev);
int gl_free(gl_ctx *ctx, void *dev);
/* gl_free keeps blocks of >= 256 MiB in the context (an arena) and gl_malloc hands them out again for requests of the same size (up to 1/8
 * smaller): the 153 GiB of query rows of a 256 x 256 attack cost 2-7 s to allocate and free per call otherwise.  gl_ctx_trim returns the kept
 * blocks to the driver (the library does it itself when one of its allocations runs out of memory; gl_ctx_destroy does it too). */
int gl_ctx_trim(gl_ctx *ctx);
/* device memory of the context's GPU: *out_available = bytes a gl_malloc could get right now (hipMemGetInfo's free bytes + the blocks the arena
 * keeps), *out_total = the device's memory.  attack() sizes the resident query rows of a streamed search from it. */
int gl_mem_info(gl_ctx *ctx, size_t *out_available, size_t *out_total);
int gl_memcpy_h2d(gl_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);   /* `.to(device)`, fbb.py:135,141,145 */
int gl_memcpy_d2h(gl_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);   /* `.item()`, fbb.py:88 */
int gl_memset(gl_ctx *ctx, void *dev, int value, size_t bytes);

/* HIP events on the context stream (bench.py timing) */
int gl_event_create(void **out_event);
int gl_event_destroy(void *event);
int gl_event_record(gl_ctx *ctx, void *event);
int gl_event_elapsed_ms(void *start, void *stop, float *out_ms);   /* synchronises on `stop` */

/* per-kernel timing: while enabled, every launch of a tagged kernel is bracketed by two HIP events on
 * the context stream.  gl_prof_read synchronises and returns the summed duration and launch count
 * of one tag since the last gl_prof_reset. */
#define GL_PROF_GATHER_CONV 0   /* fp32-MFMA gather convolution (generator layers 0-3) */
#define GL_PROF_L2_KNN 1        /* int8-MFMA pairwise L2 + argmin */
#define GL_PROF_CONVT_RGB 2     /* generator tail: ConvT -> 3 channels + tanh + quantise */
#define GL_PROF_L2_PREPARE 3    /* u8 -> biased int8 + norms */
#define GL_PROF_FEAT_KNN 4      /* fp32-MFMA pairwise |V_q - V_n|^2 + argmin (l2-lpips) */
#define GL_PROF_TOPK_SELECT 5   /* top-K: selection over the stored S values + list merge (the pairwise kernel itself reports as GL_PROF_L2_KNN) */
#define GL_PROF_L2_COUNT 6      /* int8-MFMA pairwise L2 + epsilon-ball counts (gl_l2_count_i8*) */
#define GL_PROF_FEAT_COUNT 7    /* fp16-MFMA pairwise l2-lpips distance + epsilon-ball counts / stored matrix (gl_feat_count*, gl_feat_pair_dist*) */
#define GL_PROF_L2_HIST 8       /* int8-MFMA pairwise L2 + histogram of all pair distances (gl_l2_hist_i8*) */
int gl_prof_enable(gl_ctx *ctx, int on);
int gl_prof_read(gl_ctx *ctx, int tag, double *out_total_ms, int64_t *out_launches);
int gl_prof_reset(gl_ctx *ctx);

/* ---------------------------------------------------------------- 8-bit image codec */
/* float images in [-1,1] -> u8 codes, exactly when x == fl32(2*(u/255.)-1)
 * (attack_models/utils.py:82 followed by fbb.py:134 `.float()`).  *off_lattice_dev (int32, device,
 * caller-zeroed) is incremented for every element that is not on that lattice. */
int gl_encode_lattice_f32(gl_ctx *ctx, const float *x_dev, int64_t count, uint8_t *u8_dev, int32_t *off_lattice_dev);
/* u8 -> float32 2*(u/255.)-1 (float64 arithmetic, utils.py:82) */
int gl_decode_u8(gl_ctx *ctx, const uint8_t *u8_dev, int64_t count, float *x_dev);
/* generator output -> u8 as the generate branches write it: mode 0 = Normalize(-1,2) then
 * ToPILImage mul(255).byte() (gan_models/dcgan/train_torch.py:154-158,172); mode 1 = x*0.5+0.5
 * (gan_models/pggan/train.py:238). */
int gl_quantize_f32(gl_ctx *ctx, const float *x_dev, int64_t count, int mode, uint8_t *u8_dev);

/* ---------------------------------------------------------------- L2 nearest neighbour (the hot path) */
/* bytes one prepared row occupies: D rounded up to the kernel's K tile of 128 bytes; above 262143 (the wide pair) an odd number of tiles,
 * one zero tile more when needed, so that the rows of a search tile do not share one L2 set */
int64_t gl_l2_row_stride(int64_t d);
/* u8 rows -> biased int8 rows (u-128, zero padded to gl_l2_row_stride(d)) and per-row sum (u-128)^2.
 * rows_i8_dev: [count][gl_l2_row_stride(d)] bytes; norms_dev: [count] int32 (the bit pattern of an unsigned value when d > 131071).
 * d <= 262143 (3 x 256 x 256 = 196608 fits); larger images: gl_l2_prepare_wide. */
int gl_l2_prepare(gl_ctx *ctx, const uint8_t *rows_u8_dev, int64_t count, int64_t d, int8_t *rows_i8_dev, int32_t *norms_dev);
/* keys[q] = UINT64_MAX */
int gl_keys_init(gl_ctx *ctx, uint64_t *keys_dev, int64_t nq);
/* keys[q] = min(keys[q], (S(q,n) << shift) | (index_base + n)) over n in [0, n_rows):
 *   S = sum_k (uq_k - ub_k)^2, exact integers (d <= 66051: modulo 2^32 with S < 2^32; up to d = 262143: int32 segments of 64 KiB of K
 *   summed in 64 bits; larger d: gl_l2_knn_i8_wide below).  shift = 32 for d <= 33025 and one bit less per doubling of d beyond (31 at
 *   3x128x128, 29 at 3x256x256, 27 at 3x512x512, 25 at 3x1024x1024, 23 at 2^24) so that keys stay below 2^63 for the int64
 *   all-reduce(min); index_base + n_rows <= 2^shift.  gl_keys_unpack derives the same shift from d, for any d.
 *   Replaces the loop body + torch.min of custom_knn
 *   (attack_models/fbb.py:77-86) with Loss('l2') (attack_models/utils.py:163,169,176) for the whole
 *   query set at once.  The caller applies the BATCH_SIZE truncation (fbb.py:77) by passing
 *   n_rows = n_eff.  index_base is the global index of bank row 0 (bank shards). */
int gl_l2_knn_i8(gl_ctx *ctx, const int8_t *bank_i8_dev, const int32_t *bank_norm_dev, int64_t n_rows, int64_t index_base,
                 const int8_t *query_i8_dev, const int32_t *query_norm_dev, int64_t nq, int64_t d, uint64_t *keys_dev);
/* Images larger than 262143 values (3x512x512, 3x1024x1024, up to gl_l2_max_d(1) = 2^24 = 3x2048x2048 and a bit beyond): the same exact
 * search with int64 row norms (sum (u-128)^2 <= 16384 d < 2^38).  gl_l2_prepare_wide writes the same int8 rows as gl_l2_prepare and
 * norms_dev [count] int64; gl_l2_knn_i8_wide takes them and gives the keys gl_l2_knn_i8 gives wherever both apply (d <= 262143), with the
 * same checks.  Loss('l2') (attack_models/utils.py:163) and custom_knn (attack_models/fbb.py:73-88) at --resolution 512 and above. */
int gl_l2_prepare_wide(gl_ctx *ctx, const uint8_t *rows_u8_dev, int64_t count, int64_t d, int8_t *rows_i8_dev, int64_t *norms_dev);
int gl_l2_knn_i8_wide(gl_ctx *ctx, const int8_t *bank_i8_dev, const int64_t *bank_norm_dev, int64_t n_rows, int64_t index_base,
                      const int8_t *query_i8_dev, const int64_t *query_norm_dev, int64_t nq, int64_t d, uint64_t *keys_dev);
/* largest d of the exact-integer search: 262143 for gl_l2_prepare / gl_l2_knn_i8 (wide = 0), 2^24 for the wide pair (wide != 0) */
int64_t gl_l2_max_d(int wide);
/* keys -> (distance fp32 = fl32(S * 4/(255^2 d)), index int64).  `min_distance.item(), indices[min_index].item()`, fbb.py:88 */
int gl_keys_unpack(gl_ctx *ctx, const uint64_t *keys_dev, int64_t nq, int64_t d, float *dist_dev, int64_t *idx_dev);
/* The same exact path for tables of small non-negative integers (x == (float)u, u in 0..255: binary / count rows such as medGAN's thresholded
 * output, gan_models/medgan/train.py:306-312): encode to bytes, gl_l2_prepare + gl_l2_knn_i8 as for images, and
 * dist = fl32(S / d) = what an fp32 mean((y-x)^2) gives while its sum is exact (S < 2^24).  off_lattice_dev counts values that are not such integers. */
int gl_encode_integers_f32(gl_ctx *ctx, const float *x_dev, int64_t count, uint8_t *u8_dev, int32_t *off_lattice_dev);
int gl_decode_u8_integers(gl_ctx *ctx, const uint8_t *u8_dev, int64_t count, float *x_dev);
int gl_keys_unpack_integers(gl_ctx *ctx, const uint64_t *keys_dev, int64_t nq, int64_t d, float *dist_dev, int64_t *idx_dev);

/* ---- the K nearest bank rows of every query under the same exact distance, 1 <= k <= GL_TOPK_MAX.
 * topk_keys_dev is [nq][k] keys, ascending per query: the k smallest keys (S << shift | global index, as gl_l2_knn_i8 packs them) seen so
 * far, UINT64_MAX in slots that are still empty.  Keys are unique and totally ordered, so ties in S go to the smaller global index in
 * every column and the lists do not depend on tile, slicing, chunking or sharding; column 0 is the key gl_l2_knn_i8 gives.
 * This is custom_knn (attack_models/fbb.py:73-88) keeping the args.K nearest samples (fbb.py:35) instead of one. */
#define GL_TOPK_MAX 32
/* every slot = UINT64_MAX (empty) */
int gl_topk_init(gl_ctx *ctx, uint64_t *topk_keys_dev, int64_t nq, int k);
/* row q of topk_keys_dev = the k smallest of (what it held) and the keys of bank rows [0, n_rows): accumulates like gl_l2_knn_i8, so a
 * streamed bank is searched chunk by chunk into one list.  Unlike gl_l2_knn_i8's minimum this is not idempotent: every global index
 * (index_base + n) may be folded into a list at most once, searching the same rows twice leaves duplicate keys in it.
 * Arguments and checks as gl_l2_knn_i8 / gl_l2_knn_i8_wide.  The pairwise
 * contraction runs once whatever k is: the kernel stores the exact S of every pair, a selection kernel keeps the k smallest keys.  The S
 * values of one slice of queries x bank rows live in a workspace from gl_malloc of at most 1 GiB (gl_topk_set_workspace); the library walks
 * the slices itself and the result does not depend on them.  Synchronises when it returns its workspace (gl_free). */
int gl_l2_topk_i8(gl_ctx *ctx, const int8_t *bank_i8_dev, const int32_t *bank_norm_dev, int64_t n_rows, int64_t index_base,
                  const int8_t *query_i8_dev, const int32_t *query_norm_dev, int64_t nq, int64_t d, int k, uint64_t *topk_keys_dev);
int gl_l2_topk_i8_wide(gl_ctx *ctx, const int8_t *bank_i8_dev, const int64_t *bank_norm_dev, int64_t n_rows, int64_t index_base,
                       const int8_t *query_i8_dev, const int64_t *query_norm_dev, int64_t nq, int64_t d, int k, uint64_t *topk_keys_dev);
/* dst[q] = the k smallest of dst[q] and src[l][q], l < n_lists; src_dev is [n_lists][nq][k] (e.g. what gl_allgather_rows delivers from the
 * ranks of a sharded bank).  Key-agnostic: any lists of ascending unique 64-bit keys. */
int gl_topk_merge(gl_ctx *ctx, uint64_t *dst_dev, const uint64_t *src_dev, int64_t nq, int k, int64_t n_lists);
/* [nq][k] keys -> dist_dev [nq][k] fp32, idx_dev [nq][k] int64: gl_keys_unpack (integers = 0) or gl_keys_unpack_integers (integers != 0)
 * per slot; an empty slot gives +inf and -1. */
int gl_topk_unpack(gl_ctx *ctx, const uint64_t *topk_keys_dev, int64_t nq, int k, int64_t d, int integers, float *dist_dev, int64_t *idx_dev);
/* bytes of S values one slice of gl_l2_topk_i8* may occupy (0 = the default of 1 GiB; never less than one tile).  For tests of the slicing
 * and for hosts that are short of memory; the result does not depend on it. */
int gl_topk_set_workspace(gl_ctx *ctx, size_t bytes);

/* ---- epsilon-ball counts under the same exact distance: how many bank rows lie within each of T thresholds of every query.  The score of
 * the Monte-Carlo membership attack (Hilprecht et al., PoPETs 2019) is counts / n over the bank custom_knn searches
 * (attack_models/fbb.py:73-88) and the per-sample distance of Loss('l2') (attack_models/utils.py:161-164); several thresholds in one pass give
 * the per-query distance CDF.  counts_dev is [nq][n_thr] uint64.  Counts are integers of an exact S: they do not depend on tile, chunking or
 * sharding. */
#define GL_COUNT_MAX_T 16
/* every counter = 0 */
int gl_counts_init(gl_ctx *ctx, uint64_t *counts_dev, int64_t nq, int n_thr);
/* counts[q][t] += #{ n in [0, n_rows) : S(q, n) <= thr_host[t] }, S as in gl_l2_knn_i8.  thr_host: n_thr (1..GL_COUNT_MAX_T) thresholds on S in
 * HOST memory, ascending (equal neighbours allowed); a negative value means "no pair qualifies", a value above 65025 d "every pair".
 * Accumulates, so a streamed bank is counted chunk by chunk into one table; counting the same rows twice counts them twice.  No bank index is
 * involved (no index_base).  Other arguments and checks as gl_l2_knn_i8 / gl_l2_knn_i8_wide; n_rows == 0 or nq == 0 is GL_OK.  One kernel, no
 * workspace: no pairwise value is written to memory.  Asynchronous on the context's stream. */
int gl_l2_count_i8(gl_ctx *ctx, const int8_t *bank_i8_dev, const int32_t *bank_norm_dev, int64_t n_rows, const int8_t *query_i8_dev,
                   const int32_t *query_norm_dev, int64_t nq, int64_t d, const int64_t *thr_host, int n_thr, uint64_t *counts_dev);
/* the same for rows prepared by gl_l2_prepare_wide (int64 norms, d <= gl_l2_max_d(1)); equal to gl_l2_count_i8 wherever both apply */
int gl_l2_count_i8_wide(gl_ctx *ctx, const int8_t *bank_i8_dev, const int64_t *bank_norm_dev, int64_t n_rows, const int8_t *query_i8_dev,
                        const int64_t *query_norm_dev, int64_t nq, int64_t d, const int64_t *thr_host, int n_thr, uint64_t *counts_dev);
/* thresholds PER QUERY: counts[q][t] += #{ n in [0, n_rows) : S(q, n) <= thr_dev[q][t] }.  thr_dev: [nq][n_thr] int64 in DEVICE memory, 8-byte
 * aligned, n_thr in 1..GL_COUNT_MAX_T, ascending within each row (the caller's contract: the rows are not read on the host); a negative value
 * means "no pair of this query qualifies", a value >= 65025 d "every pair".  The kernels, tile rule, accumulation and checks of gl_l2_count_i8
 * (sizes, alignment, NULLs, n_thr); the result is a function of the multiset of S alone.  The primitive under counts with one radius per query
 * and under the exact k-th smallest S per query for any k (a host search over these counts, 16 thresholds per query and pass).  Profiled
 * under GL_PROF_L2_COUNT.  Asynchronous on the context's stream. */
int gl_l2_count_rows_i8(gl_ctx *ctx, const int8_t *bank_i8_dev, const int32_t *bank_norm_dev, int64_t n_rows, const int8_t *query_i8_dev,
                        const int32_t *query_norm_dev, int64_t nq, int64_t d, const int64_t *thr_dev, int n_thr, uint64_t *counts_dev);
/* the same for rows prepared by gl_l2_prepare_wide (int64 norms); equal to gl_l2_count_rows_i8 wherever both apply */
int gl_l2_count_rows_i8_wide(gl_ctx *ctx, const int8_t *bank_i8_dev, const int64_t *bank_norm_dev, int64_t n_rows, const int8_t *query_i8_dev,
                             const int64_t *query_norm_dev, int64_t nq, int64_t d, const int64_t *thr_dev, int n_thr, uint64_t *counts_dev);
/* ---- kernel-density (soft-min) sums under the same exact distance: the Parzen estimate P(x|G) ~ 1/n sum_i phi(x, G(z_i)) behind the
 * full-black-box score (attack_models/fbb.py:73-88 keeps its largest term, the nearest sample) with a Gaussian kernel, for n_coef
 * bandwidths in one pass over the bank:
 *     sums[q][t] += sum over n in [0, n_rows) of kde_weight(S(q, n) - S0[q], coef[t]),  S as in gl_l2_knn_i8.
 * kde_weight(delta, c) is a fixed-point stand-in for 2^(-delta c) in units of 2^-40, defined once in csrc/gl_kde_epi.h (gl_kde_weight) from
 * integer operations and individually rounded fp32 multiplies and adds: x = fl32(fl32(delta) c); 0 for x >= 41; else with n = floor(x),
 * f = x - n the truncation of p(f) 2^(40 - n), p a degree-6 polynomial for 2^-f with p(0) = 1.  kde_weight(0, c) == 2^40 exactly and no
 * weight is larger.  Accuracy against 2^(-delta c): the truncation costs at most one unit of 2^-40, on top of a relative error of at most
 * 2 x 2^-24 ln 2 (the two fp32 roundings behind x; 3.3e-6 at x = 40) plus the polynomial's 1.9e-7.  Measured (tests/test_kde_cpu.py): 4.4e-7
 * relative for x <= 8, and 9.77e-4 = 2^-10 relative over all weights of at least 2^-30, where the truncation dominates.
 * S0_dev: [nq] int64 in DEVICE memory, 8-byte aligned, the offset of every query -- the exact S of its nearest row over everything that
 *   will be summed (chunks and shards together), so that the largest weight is 2^40.  A pair with S < S0[q] is the caller's error: the
 *   kernel raises a device flag, the call returns GL_ERR_INVALID with the reason in gl_last_error(), and the sums of that call are
 *   unspecified (nothing is clamped); the flag is cleared, the context stays usable.
 * coef_host: n_coef (1..GL_COUNT_MAX_T) fp32 values in HOST memory, finite, >= 0, descending (bandwidths ascending); for the bandwidth h in
 *   units of the distance D = S / s_unit, coef = log2(e) / (h s_unit).  coef = 0 gives 2^40 per pair.
 * sums_dev: [nq][n_coef] uint64 (gl_counts_init); accumulated into with 64-bit integer adds only, so a streamed bank adds up chunk by
 *   chunk, shards are summed with gl_counts_add, and the result is a function of the multiset of S - S0 alone: it does not depend on tile,
 *   chunking, query slicing, bank order or sharding.  No overflow while fewer than 2^23 rows are summed per query (2^23 2^40 < 2^64): the
 *   caller's duty.
 * The kernels and the tile rule of gl_l2_count_rows_i8 (the same K loops) with another epilogue: one compare per pair against
 * S0[q] + cut(coef[n_coef - 1]) (gl_kde_cut: from there on every weight is 0), workgroups and waves without a pair inside leave; the others
 * reduce per (query, t) in registers, across lanes, through a 64-bit LDS table, and add one value per non-zero entry and workgroup.  Sizes,
 * alignment and NULL checks as gl_l2_count_rows_i8; n_rows == 0 or nq == 0 is GL_OK and touches nothing.  One kernel, no workspace, no
 * pairwise value is written to memory.  Profiled under GL_PROF_L2_COUNT.  Synchronises: the flag is read back before the call returns. */
int gl_l2_kde_rows_i8(gl_ctx *ctx, const int8_t *bank_i8_dev, const int32_t *bank_norm_dev, int64_t n_rows, const int8_t *query_i8_dev,
                      const int32_t *query_norm_dev, int64_t nq, int64_t d, const int64_t *S0_dev, const float *coef_host, int n_coef,
                      uint64_t *sums_dev);
/* the same for rows prepared by gl_l2_prepare_wide (int64 norms); equal to gl_l2_kde_rows_i8 wherever both apply */
int gl_l2_kde_rows_i8_wide(gl_ctx *ctx, const int8_t *bank_i8_dev, const int64_t *bank_norm_dev, int64_t n_rows, const int8_t *query_i8_dev,
                           const int64_t *query_norm_dev, int64_t nq, int64_t d, const int64_t *S0_dev, const float *coef_host, int n_coef,
                           uint64_t *sums_dev);
/* The float sibling of the cut-off under gl_l2_kde_rows_i8, for the kernel-density sums on float distances (gl_l2_kde_rows_f32,
 * gl_feat_kde_rows*): out[i] = the smallest uint32 pattern b in [bits(D0[i]), 0x7F800000] at which fl32(fl32(float(b) - D0[i]) c) is not below
 * 41, i.e. from which on every pair of query i has the weight 0 under the coefficient c (csrc/gl_kde_epi.h gl_kde_cut_bits, with the
 * monotonicity argument).  Host arrays, no context, no GPU: D0 finite and >= 0, c finite and >= 0 (else GL_ERR_INVALID). */
int gl_kde_cut_bits_rows(const float *D0, int64_t n, float c, uint32_t *out);
/* dst[q][t] += sum over l < n_lists of src[l][q][t]; src_dev is [n_lists][nq][n_thr] (e.g. what gl_allgather_rows delivers from the ranks of a
 * sharded bank): the cross-shard sum, the counterpart of gl_topk_merge. */
int gl_counts_add(gl_ctx *ctx, uint64_t *dst_dev, const uint64_t *src_dev, int64_t nq, int n_thr, int64_t n_lists);

/* ---- histogram of ALL pair distances under the same exact S: the primitive under an exact quantile of the nq x n_rows distances (the
 * percentile heuristic for the radius of the Monte-Carlo attack, Hilprecht et al., PoPETs 2019: a small quantile of all d(x_i, g_j)).
 * For a window (lo >= 0, 0 <= shift <= 40, 1 <= n_bins <= GL_HIST_MAX_BINS):
 *     hist[b] += #{ q < nq, n < n_rows : lo <= S(q, n) and (S(q, n) - lo) >> shift == b },  b < n_bins;
 * pairs outside the window are not counted.  hist_dev is [n_bins] uint64; the adds are integer adds of an exact S, so the histogram is a
 * function of the multiset of pair distances alone: it does not depend on tile, chunking or sharding.  A host radix-select (zoom into the
 * bin that holds the rank: attack.select_ranks) finds the exact S at any rank in 3 passes for S < 2^32, 4 for the wide form. */
#define GL_HIST_MAX_BINS 2048
/* every bin = 0 */
int gl_hist_init(gl_ctx *ctx, uint64_t *hist_dev, int n_bins);
/* Accumulates, so a streamed bank is binned chunk by chunk into one histogram; binning the same rows twice counts them twice.  Rows, norms and
 * their checks as gl_l2_count_i8 (16-byte aligned prepared rows, d <= gl_l2_max_d(0)); hist_dev 8-byte aligned; n_rows == 0 or nq == 0 is
 * GL_OK and touches nothing.  Shards are summed with gl_counts_add(dst, src, nq = n_bins, n_thr = 1, n_lists).  One kernel (the pair loop of
 * gl_l2_count_i8 with a binning epilogue), no workspace: no pairwise value is written to memory.  Asynchronous on the context's stream.
 * Reports as GL_PROF_L2_HIST. */
int gl_l2_hist_i8(gl_ctx *ctx, const int8_t *bank_i8_dev, const int32_t *bank_norm_dev, int64_t n_rows, const int8_t *query_i8_dev,
                  const int32_t *query_norm_dev, int64_t nq, int64_t d, int64_t lo, int shift, int n_bins, uint64_t *hist_dev);
/* the same for rows prepared by gl_l2_prepare_wide (int64 norms, d <= gl_l2_max_d(1)); equal to gl_l2_hist_i8 wherever both apply */
int gl_l2_hist_i8_wide(gl_ctx *ctx, const int8_t *bank_i8_dev, const int64_t *bank_norm_dev, int64_t n_rows, const int8_t *query_i8_dev,
                       const int64_t *query_norm_dev, int64_t nq, int64_t d, int64_t lo, int shift, int n_bins, uint64_t *hist_dev);

/* out[i] = fl32(S(x_hat[i], x_gt[b_gt == 1 ? 0 : i]) * 4/(255^2 d)), i < b: the per-sample loss vector
 * Loss('l2').forward(x_hat, x_gt) returns (attack_models/utils.py:163,169,171-177; x_gt broadcasts
 * when it holds one image, fbb.py:79).  u8 rows on the device, d <= gl_l2_max_d(1). */
int gl_l2_rows_u8(gl_ctx *ctx, const uint8_t *x_hat_u8_dev, int64_t b, const uint8_t *x_gt_u8_dev, int64_t b_gt, int64_t d, float *out_dev);

/* ---- arbitrary fp32 images (values off the 8-bit lattice): fixed-order fp32 evaluation of
 * mean((y - x)**2) (attack_models/utils.py:163): four interleaved fmaf chains over k, summed pairwise, divided by
 * d (exact definition in gan-leaks_amd/csrc/gl_l2f32.hip, shared bit for bit with the oracle).
 * keys[q] = min(keys[q], (float_bits(dist) << 32) | (index_base + n)); rows are [count][d] fp32, 16-byte aligned. */
int gl_l2_knn_f32(gl_ctx *ctx, const float *bank_dev, int64_t n_rows, int64_t index_base, const float *query_dev, int64_t nq, int64_t d,
                  uint64_t *keys_dev);
int gl_keys_unpack_f32(gl_ctx *ctx, const uint64_t *keys_dev, int64_t nq, float *dist_dev, int64_t *idx_dev);
/* The other two reductions over the same D32(q, n) -- the K loop of gl_l2_knn_f32 with another epilogue, so the value is the same bits and a
 * function of the two rows alone (no tile, slice, chunk or shard shows in it).  Finite rows; D32 >= +0.
 * gl_l2_topk_f32: custom_knn (attack_models/fbb.py:73-88) keeping the args.K nearest samples for rows off the lattices.  topk_keys_dev [nq][k]
 *   as for gl_l2_topk_i8 (gl_topk_init, folds into what the lists hold, every global index at most once), keys float_bits(D32) << 32 |
 *   (index_base + n): column 0 is gl_l2_knn_f32's key, ties go to the smaller index.  Merge with gl_topk_merge, unpack with
 *   gl_topk_unpack_f32.  Slices of D32 pieces live in the workspace of gl_topk_set_workspace; synchronises when it returns it.
 * gl_l2_count_f32: counts[q][t] += #{ n in [0, n_rows) : D32(q, n) <= thr_host[t] }, a float32 compare of mean((y - x)**2)
 *   (attack_models/utils.py:163); thr_host: n_thr (1..GL_COUNT_MAX_T) radii in HOST memory, ascending, not NaN; a negative radius counts
 *   nothing, +inf every row.  counts_dev [nq][n_thr] uint64 (gl_counts_init, gl_counts_add across shards).  One kernel, asynchronous. */
int gl_l2_topk_f32(gl_ctx *ctx, const float *bank_dev, int64_t n_rows, int64_t index_base, const float *query_dev, int64_t nq, int64_t d, int k,
                   uint64_t *topk_keys_dev);
int gl_l2_count_f32(gl_ctx *ctx, const float *bank_dev, int64_t n_rows, const float *query_dev, int64_t nq, int64_t d, const float *thr_host,
                    int n_thr, uint64_t *counts_dev);
/* gl_l2_count_f32 with thresholds PER QUERY, on the uint32 pattern of D32:
 *     counts_dev[q * n_thr + t] += #{ n in [0, n_rows) : bits(D32(q, n)) <= thr_dev[q][t] }.
 * thr_dev: [nq][n_thr] int64 in DEVICE memory, 8-byte aligned, n_thr in 1..GL_COUNT_MAX_T, ascending within each row (the caller's contract,
 * as for gl_l2_count_rows_i8); a negative value counts nothing, a value >= 0x7F800000 (+inf) every pair whose D32 is not NaN; NaN patterns
 * exceed every bound, as a float compare would have it.  D32 >= +0, so the compare of the patterns is the float32 compare
 * D32 <= float(thr) of mean((y - x)**2) (attack_models/utils.py:163): one radius per query (a k-NN density score), and under a host search
 * over these counts the exact k-th smallest D32 per query for any k (custom_knn, attack_models/fbb.py:73-88, beyond GL_TOPK_MAX).  Sizes,
 * alignment and NULL checks of gl_l2_count_f32; n_rows == 0 or nq == 0 is GL_OK and touches nothing.  One kernel (the K loop of
 * gl_l2_knn_f32), asynchronous; like gl_l2_count_f32 it reports under no profiling id. */
int gl_l2_count_rows_f32(gl_ctx *ctx, const float *bank_dev, int64_t n_rows, const float *query_dev, int64_t nq, int64_t d, const int64_t *thr_dev,
                         int n_thr, uint64_t *counts_dev);
/* Kernel-density (soft-min) sums on fp32 rows, gl_l2_kde_rows_i8 on the float32 distance of gl_l2_knn_f32:
 *     sums_dev[q * n_coef + t] += sum over n in [0, n_rows) of gl_kde_weight_f32(D32(q, n), D0_dev[q], coef_host[t]),
 * the fixed-point weight 2^(-(D32 - D0) coef) in units of 2^-40 (csrc/gl_kde_epi.h: one rounded subtraction, one rounded product, then the
 * integer path's arithmetic; a pure function of (D32, D0, coef), so the sums are a function of the multiset of distances: tile, chunking,
 * bank order and sharding do not matter).  D0_dev: [nq] float32 in DEVICE memory, the distance of every query's nearest row (finite, >= 0);
 * bound_dev: [nq] uint32 in DEVICE memory, gl_kde_cut_bits_rows(D0, coef_host[n_coef - 1]): a pair takes part when bits(D32) < bound, so a
 * pair at +inf weighs nothing; both 4-byte aligned.  coef_host: n_coef in 1..GL_COUNT_MAX_T finite values >= 0, DESCENDING.  sums_dev
 * [nq][n_coef] uint64 of gl_counts_init, 8-byte aligned; fewer than 2^23 rows per query in all (the caller's duty).
 * Two errors are found by the kernel and reported through a device flag that the call reads back and clears (so the next call on the
 * context is unaffected; the sums of the failing call are unspecified): a pair with bits(D32) < bits(D0) (GL_ERR_INVALID, "below the offset":
 * its weight would exceed 2^40) and a pair whose D32 is NaN (GL_ERR_INVALID, "NaN").  Other checks as gl_l2_count_rows_f32; n_rows == 0 or
 * nq == 0 is GL_OK and touches nothing.  One kernel (the K loop of gl_l2_knn_f32).  Synchronises. */
int gl_l2_kde_rows_f32(gl_ctx *ctx, const float *bank_dev, int64_t n_rows, const float *query_dev, int64_t nq, int64_t d, const float *D0_dev,
                       const uint32_t *bound_dev, const float *coef_host, int n_coef, uint64_t *sums_dev);
/* The histogram of ALL pair distances on fp32 rows: the primitive under an exact quantile of the nq x n_rows values D32(q, n) (the K loop of
 * gl_l2_knn_f32 with a binning epilogue, so D32 is the same bits again).  D32 >= +0, so the unsigned order of the uint32 patterns
 * bits(D32) is the order of the floats and a radix-select over windows of patterns finds the exact D32 at any rank.  For a window
 * (lo: uint32, 0 <= shift <= 31, 1 <= n_bins <= GL_HIST_MAX_BINS):
 *     hist[b] += #{ q < nq, n < n_rows : lo <= bits(D32(q, n)) <= 0x7F800000 and (bits(D32(q, n)) - lo) >> shift == b },  b < n_bins.
 * 0x7F800000 is +inf: a pair at +inf is counted, NaN patterns lie outside every window (a first level over [0, 2^31) that holds fewer than
 * nq * n_rows pairs shows them).  A window above 0x7F800000 returns at once.  hist_dev [n_bins] uint64, 8-byte aligned, zeroed by
 * gl_hist_init; accumulates like gl_l2_hist_i8; shards are summed with gl_counts_add(dst, src, nq = n_bins, n_thr = 1, n_lists).
 * n_rows == 0 or nq == 0 is GL_OK and touches nothing.  One kernel, no workspace, asynchronous; like gl_l2_count_f32 it reports under no
 * profiling id. */
int gl_l2_hist_f32(gl_ctx *ctx, const float *bank_dev, int64_t n_rows, const float *query_dev, int64_t nq, int64_t d, uint32_t lo, int shift,
                   int n_bins, uint64_t *hist_dev);
/* Loss('l2').forward for fp32 inputs: out[i] = dist(x_hat[i], x_gt[b_gt == 1 ? 0 : i]) */
int gl_l2_rows_f32(gl_ctx *ctx, const float *x_hat_dev, int64_t b, const float *x_gt_dev, int64_t b_gt, int64_t d, float *out_dev);

/* One-call form for host callers: u8 images in HOST memory, results in HOST memory; applies the
 * truncation n_eff = (n_bank / batch_size) * batch_size itself.  Equals
 * [custom_knn(bank, q, Loss('l2'), args) for q in queries]  (attack_models/fbb.py:73-88,156-159).
 * Synchronises. Returns GL_ERR_EMPTY_BANK when n_bank < batch_size. */
int gl_fbb_knn_l2_host(gl_ctx *ctx, const uint8_t *bank_u8_host, int64_t n_bank, const uint8_t *queries_u8_host, int64_t nq,
                       int64_t d, int64_t batch_size, float *dist_host, int64_t *idx_host);

/* ---------------------------------------------------------------- partial-black-box attack: gradient-free latent search
 * GAN-Leaks' second attack (section 5.3 of the paper; the reference fork ships only fbb.py): the attacker holds the generator, searches
 * z* = argmin_z L(x, G(z)) without gradients and scores the query by L(x, G(z*)).  Built as a (1 + lambda) evolution strategy per query:
 * a round is gl_pbb_candidates -> the generator on all nq * lambda latents -> gl_pbb_group_min -> gl_pbb_accept, with everything resident on
 * the device.  Under 0.2 LPIPS + L2, the distance fbb.main hard-wires, the third step is the candidates' search rows (gl_lpips_*_features_*),
 * gl_feat_pair_dist* per tile of 256 queries against the tile's own candidates and gl_pbb_group_min_keys over the stored block; the other
 * steps are the same.  All four run on the context's stream, do not synchronise, return GL_OK for nq == 0 and read no tuning variable. */
/* the bit pattern of C = float32(1 / (65536 sqrt(8/3))) = 9.344062e-06, the scale of the noise below */
#define GL_PBB_NOISE_SCALE_BITS 0x371CC471u
/* out[(q * lambda + j) * nz + c] = clamp(fl32(z[q * nz + c] + fl32(sigma[q] * eps)), -z_max, z_max), each operation rounded on its own (no
 * fma).  eps(seed, round, query_base + q, j, c) is a pure function of its five indices, from integer arithmetic only: ONE Philox4x32-10
 * call with key (seed & 0xffffffff, seed >> 32) and counter (c, j, (query_base + q) & 0xffffffff, round); its four words are cut into eight
 * 16-bit halves h0..h7; t = 2 (h0 + ... + h7) - 524280, an int32 with |t| < 2^24; eps = fl32(float(t) * C).  That is Irwin-Hall with n = 8:
 * mean 0, variance 1, support +-4.9.  Candidates therefore do not depend on how the queries are blocked or sharded (query_base is the
 * global index of query 0 of this call).  z_dev [nq][nz], sigma_dev [nq], out_dev [nq * lambda][nz], fp32.  query_base + nq <= 2^32;
 * z_max finite and positive. */
int gl_pbb_candidates(gl_ctx *ctx, const float *z_dev, const float *sigma_dev, int64_t nq, int64_t nz, int64_t lambda, uint64_t seed, uint32_t round,
                      int64_t query_base, float z_max, float *out_dev);
/* Every query against its OWN lambda candidate images (a grouped distance, not all pairs): S(q, j) = sum_k (queries[q][k] -
 * cand[q * lambda + j][k])^2 exactly, out_S[q] = min_j S(q, j), out_j[q] = the smallest j that attains it.  Raw image codes on both sides: no
 * prepare step, no norms.  queries_u8_dev [nq][d], cand_u8_dev [nq * lambda][d], d <= gl_l2_max_d(1); out_S_dev [nq] uint64 (8-byte
 * aligned), out_j_dev [nq] int32.  A streaming kernel: workgroup (q, g) takes GL_PBB_GROUP candidates of query q, the query row goes
 * through LDS in chunks, each wave owns whole candidates, reads them once with 16-byte loads (bytes when d is no multiple of 16 or a base
 * pointer is not 16-byte aligned) and squares with the 8-bit dot instruction into 64-bit totals; no pairwise value reaches memory.
 * workspace_dev: GL_PBB_PARTIAL_BYTES * nq * ceil(lambda / GL_PBB_GROUP) bytes, 16-byte aligned, holding one (S, j) per workgroup, which a
 * second small kernel of the same call combines in ascending j (no atomics). */
#define GL_PBB_GROUP 16
#define GL_PBB_PARTIAL_BYTES 16
int gl_pbb_group_min(gl_ctx *ctx, const uint8_t *queries_u8_dev, const uint8_t *cand_u8_dev, int64_t nq, int64_t lambda, int64_t d, uint64_t *out_S_dev,
                     int32_t *out_j_dev, void *workspace_dev);
/* The grouped minimum under 0.2 LPIPS + L2, the distance fbb.main hard-wires (attack_models/fbb.py:148), over a stored block of pair
 * distances: M_dev is what gl_feat_pair_dist / gl_feat_pair_dist_h1_scaled wrote for nq queries against their nq * lambda candidate rows
 * (leading dimension ld >= nq * lambda floats), query i's own candidates in columns i * lambda .. i * lambda + lambda - 1.
 *     keys_dev[i] = min_j bits(M[i * ld + i * lambda + j]), zero-extended;  j_dev[i] = the smallest j that attains it.
 * The uint32 patterns are compared as unsigned integers: D32 >= +0 and never NaN, so that is the order of the floats (+inf included), and
 * the result is the form gl_wb_diag_keys writes (lambda = 1 is the diagonal) and gl_pbb_accept reads.  Going through the search's own pair
 * kernels is what makes the score the bits attack(distance='l2-lpips') reports for the pair.  1 <= lambda < 2^31, nq < 2^31; keys_dev [nq]
 * uint64 (8-byte aligned), j_dev [nq] int32.  One wave per query, lanes striding over j, a 64-bit minimum of (pattern << 32) | j across
 * the wave; no atomics, no workspace. */
int gl_pbb_group_min_keys(gl_ctx *ctx, const float *M_dev, int64_t nq, int64_t lambda, int64_t ld, uint64_t *keys_dev, int32_t *j_dev);
/* The elitist (1 + lambda) step.  Where S_new[q] < S_cur[q], strictly: z[q] = cand_z[q * lambda + j_new[q]], S_cur[q] = S_new[q],
 * sigma[q] = fl32(sigma[q] * up), accepted[q] = 1; otherwise sigma[q] = fl32(sigma[q] * down), accepted[q] = 0 and z, S_cur stay.  Then
 * sigma[q] is clamped to [sigma_min, sigma_max].  z_dev [nq][nz], sigma_dev [nq], cand_z_dev [nq * lambda][nz] fp32; S_cur_dev, S_new_dev
 * [nq] uint64; j_new_dev [nq] int32 in [0, lambda) (a value outside is not accepted); accepted_dev [nq] bytes.  up, down, sigma_min <=
 * sigma_max finite and positive. */
int gl_pbb_accept(gl_ctx *ctx, float *z_dev, float *sigma_dev, uint64_t *S_cur_dev, const float *cand_z_dev, const uint64_t *S_new_dev,
                  const int32_t *j_new_dev, int64_t nq, int64_t nz, int64_t lambda, float up, float down, float sigma_min, float sigma_max,
                  uint8_t *accepted_dev);

/* ---------------------------------------------------------------- reconstruction attack (VAE-type models)
 * The second attack of Hilprecht et al. (the paper of the Monte-Carlo attacks): the attacker holds the whole VAEGAN and scores a query x by how
 * well the model reconstructs it, |x - G(z)| for z at the encoder's posterior mean and over draws from the posterior.  A block of queries is
 * gl_vaegan_enc_encode -> gl_recon_latents -> the generator on all nq * lambda latents -> gl_pbb_group_S.  Both calls below follow the
 * conventions of the partial-black-box calls: the context's stream, no synchronisation, GL_OK for nq == 0, no tuning variable, no atomics. */
/* out[(q * lambda + j) * nz + c] = clamp(fl32(mu[q * nz + c] + fl32(std[q * nz + c] * eps)), -z_max, z_max), each operation rounded on its own
 * (no fma): gl_pbb_candidates with a width per coordinate.  eps = 0 for j = 0, so row 0 of every query is the clamped mean itself; for j >= 1
 * eps = eps(seed, round = 0, query_base + q, j, c), the noise gl_pbb_candidates documents above.  mu_dev, std_dev [nq][nz], out_dev
 * [nq * lambda][nz], fp32; lambda = draws + 1.  std is an input: the caller computes it on the host (float32 exp), which keeps a device expf
 * out of the contract.  NOTE the reference's quirk: Encoder.reparametrize (gan_models/vaegan/train.py:98-101) computes
 * std = logvar.mul(1.0).exp_(), that is exp(logvar) and not exp(logvar / 2); callers that follow the reference pass exp(logvar). */
int gl_recon_latents(gl_ctx *ctx, const float *mu_dev, const float *std_dev, int64_t nq, int64_t nz, int64_t lambda, uint64_t seed, int64_t query_base,
                     float z_max, float *out_dev);
/* gl_pbb_group_min's sibling that keeps every value: out_S_dev[q * lambda + j] = S(q, j) = sum_k (queries[q][k] - cand[q * lambda + j][k])^2,
 * the exact integer, uint64 (8-byte aligned).  The same kernel body and the same constraints (any d >= 1, byte loads where d is no multiple of
 * 16 or a base pointer is not 16-byte aligned, 64-bit totals), so for a table generator's 0 / 1 rows it counts what gl_pbb_group_min counts.
 * No workspace: every wave stores the S of its own candidates. */
int gl_pbb_group_S(gl_ctx *ctx, const uint8_t *queries_u8_dev, const uint8_t *cand_u8_dev, int64_t nq, int64_t lambda, int64_t d, uint64_t *out_S_dev);

/* ---------------------------------------------------------------- white-box attack: gradient descent on the latent
 * GAN-Leaks' third attack (section 5.4 of the paper): z* = argmin_z L(x, G(z)) by gradient descent with the generator's weights in hand.
 * A step is gl_dcgan_l2_grad_z -> gl_wb_adam_step -> the generator's 8-bit images of the new iterate -> gl_pbb_group_min (lambda = 1) ->
 * gl_pbb_accept (lambda = 1) into a separate best-so-far (z, S), so that the reported score is the exact integer S of the other attacks. */
/* One Adam update per element, fp32, every operation rounded on its own (no fma; correctly rounded quotient and square root):
 *   m = fl(fl(beta1 m) + fl(fl(1 - beta1) g)),  v = fl(fl(beta2 v) + fl(fl(fl(1 - beta2) g) g)),
 *   z = clamp(fl(z - fl(fl(lr fl(m c1)) / fl(sqrt(fl(v c2)) + eps))), -z_max, z_max)
 * with c1 = 1 / (1 - beta1^t), c2 = 1 / (1 - beta2^t) computed by the caller in double and passed as floats.  z, m, v, grad [nq][nz]. */
int gl_wb_adam_step(gl_ctx *ctx, float *z_dev, float *m_dev, float *v_dev, const float *grad_dev, int64_t nq, int64_t nz, float lr, float beta1,
                    float beta2, float eps, float c1, float c2, float z_max);
/* keys[i] = the uint32 pattern of M[i * ld + i], zero-extended, i < n: the scores of n queries against their own images, taken from the diagonal
 * of a block of pair distances (gl_feat_pair_dist*), in the form gl_pbb_accept compares.  The distances are >= +0, so the unsigned order of the
 * patterns is the order of the floats.  Asynchronous. */
int gl_wb_diag_keys(gl_ctx *ctx, const float *M_dev, int64_t n, int64_t ld, uint64_t *keys_dev);

/* ---------------------------------------------------------------- white-box attack: L-BFGS with a parallel line search
 * The paper's optimiser (section 5.4 minimises over z with L-BFGS).  The line search is a ladder: every query scores L step widths along its
 * direction in one batched forward, with the kernels of the partial-black-box attack.  A step, for all queries of a block:
 *   g = the gradient at z -> gl_wb_lbfgs_push -> gl_wb_lbfgs_direction -> gl_wb_lbfgs_candidates -> the generator's 8-bit images of the
 *   nq * L candidates -> gl_pbb_group_min (lambda = L; under 0.2 LPIPS + L2: gl_feat_pair_dist* and gl_pbb_group_min_keys) ->
 *   gl_pbb_accept (lambda = L, its sigma a dummy) straight into z and S_cur -> gl_wb_lbfgs_advance.
 * The iterate is itself the best so far.  Per-query state: z, z_prev, g_prev [nq][nz]; the ring S_hist, Y_hist [nq][m][nz] with count, head
 * int32 [nq] (head: the slot the next pair goes to; the i-th newest pair sits in slot (head - 1 - i) mod m); the trial width t fp32 [nq]; a
 * flag byte [nq].  A query whose t is 0, negative or not finite is FINISHED: all four calls leave its state alone, its direction is 0 and
 * its candidates are copies of z (never strictly closer, so never accepted).  Start: count = head = flag = 0, t = 1 (any live value).
 * All four run on the context's stream, do not synchronise, return GL_OK for nq == 0 without touching a pointer, read no tuning variable
 * and use no atomics.  1 <= m <= GL_WB_LBFGS_MAX_M, 1 <= L <= GL_WB_LBFGS_MAX_LADDER, 1 <= nz < 2^31, nq < 2^31.
 * Arithmetic: fp32, every product, sum and quotient rounded on its own (no fma, correctly rounded quotient and square root).  Every dot
 * product a.b over nz elements has ONE order: lane l of the query's wave adds fl(a[c] b[c]) for c = l, l + 64, ... in ascending order
 * into a sum that starts at +0, then the 64 sums go through the butterfly v = fl(v + v[lane ^ o]), o = 32, 16, 8, 4, 2, 1.  A host
 * restatement in float32 reproduces the ring, p and t bit for bit. */
#define GL_WB_LBFGS_MAX_M 16
#define GL_WB_LBFGS_MAX_LADDER 32
#define GL_WB_LBFGS_STEEPEST 1 /* flag bit: the direction of this step is -g */
#define GL_WB_LBFGS_DROPPED 2  /* flag bit: -H g was no descent direction (g.p >= 0 or a value not finite): the ring was dropped */
/* Where moved[q] != 0 (gl_pbb_accept's accepted[q] of the step before): s = fl(z - z_prev), y = fl(grad - g_prev); the pair goes into slot
 * head iff s.y > 0 and fl(1 / s.y) is finite (the cautious update), head = (head + 1) mod m, count = min(count + 1, m).  Then, for every
 * query, z_prev = z and g_prev = grad.  One wave per query. */
int gl_wb_lbfgs_push(gl_ctx *ctx, const float *z_dev, const float *grad_dev, float *z_prev_dev, float *g_prev_dev, float *S_hist_dev, float *Y_hist_dev,
                     int32_t *count_dev, int32_t *head_dev, const uint8_t *moved_dev, int64_t nq, int64_t nz, int64_t m);
/* p = -H grad by the two-loop recursion over the query's count pairs; callable on its own on rings and gradients the caller uploaded.
 *   q = grad; for i = 0 .. count-1 (newest first): rho_i = fl(1 / s_i.y_i), alpha_i = fl(rho_i (s_i.q)), q = fl(q - fl(alpha_i y_i));
 *   r = fl(gamma q), gamma = fl(s_0.y_0 / y_0.y_0); for i = count-1 .. 0: beta = fl(rho_i (y_i.r)), r = fl(r + fl(s_i fl(alpha_i - beta)));
 *   p = -r, flag = 0, t = 1.
 * With count == 0: p = -grad, flag = GL_WB_LBFGS_STEEPEST.  If grad.p >= 0 or grad.p or an element of p is not finite: count = head = 0,
 * p = -grad, flag = GL_WB_LBFGS_STEEPEST | GL_WB_LBFGS_DROPPED.  In both steepest-descent cases t stays as it is where the flag byte on
 * entry had GL_WB_LBFGS_STEEPEST set (consecutive steepest-descent steps carry the width gl_wb_lbfgs_advance left), and is
 * fl(step0 / fl(sqrt(grad.grad))) otherwise: a first trial of length step0 in latent space.  A zero gradient therefore finishes the query.
 * count_dev, head_dev, t_dev, flag_dev are read and written; p_dev [nq][nz] also serves as the recursion's working vector.  step0 finite
 * and positive.  One wave per query; the ring rows are read once per loop. */
int gl_wb_lbfgs_direction(gl_ctx *ctx, const float *grad_dev, const float *S_hist_dev, const float *Y_hist_dev, int32_t *count_dev, int32_t *head_dev,
                          float *t_dev, uint8_t *flag_dev, int64_t nq, int64_t nz, int64_t m, float step0, float *p_dev);
/* out[(q * L + j) * nz + c] = clamp(fl(z[q][c] + fl(fl(t[q] 2^-j) p[q][c])), -z_max, z_max), j < L: the ladder of trial points, the per-query
 * width read from the device array t_dev.  out_dev [nq * L][nz].  z_max finite and positive. */
int gl_wb_lbfgs_candidates(gl_ctx *ctx, const float *z_dev, const float *p_dev, const float *t_dev, int64_t nq, int64_t nz, int64_t ladder, float z_max,
                           float *out_dev);
/* After gl_pbb_accept (accepted_dev, j_new_dev as it left and read them; flag_dev as gl_wb_lbfgs_direction left it):
 *   accepted, steepest descent : t = fl(fl(2 t) 2^-j_new)      the next ladder starts one rung above the rung that won
 *   accepted, quasi-Newton     : nothing (the next direction sets t = 1 again)
 *   rejected, steepest descent : t = fl(t 2^-L)                the next ladder goes on below where this one ended
 *   rejected, quasi-Newton     : count = head = 0              the ring is dropped; the next step is steepest descent at length step0
 * A t that reaches 0 or leaves the finite range finishes the query. */
int gl_wb_lbfgs_advance(gl_ctx *ctx, float *t_dev, int32_t *count_dev, int32_t *head_dev, const uint8_t *flag_dev, const uint8_t *accepted_dev,
                        const int32_t *j_new_dev, int64_t nq, int64_t ladder);

/* ---------------------------------------------------------------- partial-black-box attack: Powell's method with a parallel line search
 * The paper's optimiser (section 5.3 runs Powell's conjugate-direction method per query).  All queries of a block advance in lock-step, and
 * every line search is a two-sided ladder: a query scores L step widths along one direction in one batched forward, with the kernels of
 * the evolution strategy.  Per-query state, all of it on the device: z [nq][nz]; the direction rows U [nq][nz + 1][nz] fp32 (rows 0 ..
 * nz - 1 the direction set, row nz the current sweep's displacement); the trial widths t [nq][nz + 1] fp32, one per row; z0 [nq][nz], the
 * latent at the sweep's start; the keys S_cur, S_prev, f0, S_e uint64 [nq]; drop_best double [nq], the largest decrease on one line in
 * this sweep, and i_best int32 [nq], the line where it happened; a flag byte [nq].  A key is what gl_pbb_accept compares: the exact integer
 * S (kind 0), or the uint32 pattern of the float32 distance, zero-extended (kind 1).  f(key) is its conversion to double: exact for S <
 * 2^53 and for every float32.  A sweep, for all queries of a block:
 *   gl_pbb_powell_begin -> for line = 0 .. nz - 1 { gl_pbb_powell_candidates -> the generator's 8-bit images of the nq * L candidates ->
 *   gl_pbb_group_min (lambda = L; under 0.2 LPIPS + L2: gl_feat_pair_dist* and gl_pbb_group_min_keys) -> gl_pbb_accept (lambda = L, its
 *   sigma a dummy of ones, up = down = 1) straight into z and S_cur -> gl_pbb_powell_advance } -> gl_pbb_powell_extrapolate -> the key of
 *   z_e (lambda = 1) into S_e -> gl_pbb_powell_decide -> line nz as the lines before it -> gl_pbb_powell_replace.
 * All seven run on the context's stream, do not synchronise, return GL_OK for nq == 0 without touching a pointer, read no tuning variable,
 * use no atomics and draw no noise: the results are a pure function of the inputs.  1 <= nz < 2^31 - 1, nq < 2^31, nq (nz + 1) nz floats
 * addressable; L even, 2 <= L <= GL_PBB_POWELL_MAX_LADDER; 0 <= line <= nz; float arrays and int32 arrays 4-byte, uint64 and double arrays
 * 8-byte aligned.  Arithmetic: fp32 (fp64 in the test of gl_pbb_powell_decide and for drop), every product, sum and difference rounded on
 * its own (no fma), so a host restatement reproduces U, t, z, flag and i_best bit for bit. */
#define GL_PBB_POWELL_MAX_LADDER 32
/* U[q][i][c] = 1 where i == c, else 0 (row nz is 0); t[q][i] = step0 for i < nz, t[q][nz] = 0.  Nothing is uploaded.  step0 finite and
 * positive. */
int gl_pbb_powell_init(gl_ctx *ctx, float *U_dev, float *t_dev, int64_t nq, int64_t nz, float step0);
/* The start of a sweep: z0 = z, f0 = S_prev = S_cur, drop_best = 0, i_best = 0. */
int gl_pbb_powell_begin(gl_ctx *ctx, const float *z_dev, const uint64_t *S_cur_dev, float *z0_dev, uint64_t *f0_dev, uint64_t *S_prev_dev,
                        double *drop_best_dev, int32_t *i_best_dev, int64_t nq, int64_t nz);
/* The ladder of line `line`: rung r < L has width a = fl(w_r t[q][line]), w_r = +2^-(r >> 1) for even r and -2^-(r >> 1) for odd r (a
 * gradient-free line search looks both ways), and
 *   out[(q * L + r) * nz + c] = clamp(fl(z[q][c] + fl(a U[q][line][c])), -z_max, z_max).
 * With t[q][line] == 0 every candidate equals z[q] and is never strictly closer.  gl_pbb_group_min takes ties to the smaller r: the wider
 * step, and of two equal widths the positive one.  out_dev [nq * L][nz]; z_max finite and positive.  One thread per value. */
int gl_pbb_powell_candidates(gl_ctx *ctx, const float *z_dev, const float *U_dev, const float *t_dev, int64_t nq, int64_t nz, int64_t line,
                             int64_t ladder, float z_max, float *out_dev);
/* After gl_pbb_accept (accepted_dev, j_new_dev as it left and read them; S_cur_dev as it left it), with w = t[q][line]:
 *   accepted at rung r = j_new[q] : t[q][line] = min(t_max, fl(fl(2 w) 2^-(r >> 1)))   the next ladder starts one rung above the one that won
 *   rejected                      : t[q][line] = max(t_min, fl(w 2^-(L / 2)))           the next ladder goes on below where this one ended
 * and for line < nz: drop = f(S_prev) - f(S_cur), one rounded difference in double; where drop > drop_best, strictly, drop_best = drop and
 * i_best = line; then S_prev = S_cur.  For line == nz, S_prev, drop_best and i_best are left alone.  kind: 0 or 1, how f reads a key.
 * 0 < t_min <= t_max, both finite.  One thread per query. */
int gl_pbb_powell_advance(gl_ctx *ctx, float *t_dev, const uint8_t *accepted_dev, const int32_t *j_new_dev, const uint64_t *S_cur_dev,
                          uint64_t *S_prev_dev, double *drop_best_dev, int32_t *i_best_dev, int64_t nq, int64_t nz, int64_t line, int64_t ladder,
                          int kind, float t_min, float t_max);
/* The sweep's displacement and the extrapolated point: U[q][nz][c] = dz = fl(z[q][c] - z0[q][c]), z_e[q][c] = clamp(fl(z[q][c] + dz),
 * -z_max, z_max).  z_e_dev [nq][nz]; the caller scores it with lambda = 1 into S_e. */
int gl_pbb_powell_extrapolate(gl_ctx *ctx, const float *z_dev, const float *z0_dev, float *U_dev, int64_t nq, int64_t nz, float z_max, float *z_e_dev);
/* Whether the displacement joins the direction set (Numerical Recipes' test).  With f0 = f(f0_dev[q]), fN = f(S_cur_dev[q]), fE =
 * f(S_e_dev[q]), D = drop_best[q], in double and each operation rounded on its own in this order:
 *   A = fl(fl(f0 - fl(2 fN)) + fE),  B = fl(fl(f0 - fN) - D),  C = fl(f0 - fE),  lhs = fl(fl(2 A) fl(B B)),  rhs = fl(D fl(C C))
 * flag[q] = 1 iff row nz of U has an element != 0 and fE < f0 and lhs < rhs, both strictly; else 0.  Then t[q][nz] = 2 where the flag is
 * set and 0 where it is clear, so that line nz moves only the queries whose test held.  One wave per query. */
int gl_pbb_powell_decide(gl_ctx *ctx, const float *U_dev, float *t_dev, const uint64_t *f0_dev, const uint64_t *S_cur_dev, const uint64_t *S_e_dev,
                         const double *drop_best_dev, uint8_t *flag_dev, int64_t nq, int64_t nz, int kind);
/* Where flag[q] != 0: U[q][i_best] = U[q][nz - 1] and t[q][i_best] = t[q][nz - 1], then U[q][nz - 1] = U[q][nz] and t[q][nz - 1] =
 * t[q][nz]: the direction of the largest decrease leaves, the displacement comes last, and a row and its width move together (t[q][nz] is
 * what gl_pbb_powell_advance left after line nz).  An i_best outside 0 .. nz - 1 is clamped into it.  One wave per query, lane l owning
 * elements l, l + 64, ... */
int gl_pbb_powell_replace(gl_ctx *ctx, float *U_dev, float *t_dev, const uint8_t *flag_dev, const int32_t *i_best_dev, int64_t nq, int64_t nz);

/* ---------------------------------------------------------------- sharded bank: the cross-GPU minimum (RCCL over xGMI) */
/* The reference runs on one device (attack_models/fbb.py:40) and takes the minimum over the whole bank with torch.min (fbb.py:86).  With the bank
 * sharded over GPUs every rank holds keys[q] = min over ITS rows, global indices inside; the minimum over ranks of the unsigned
 * 64-bit keys is the single-device result bit for bit (smallest distance, then smallest global index).  One communicator rank per gl_ctx;
 * librccl is bound at run time on the first gl_comm_* call (GL_ERR_RCCL if absent).
 *   one process per GPU : rank 0 calls gl_comm_unique_id, the launcher carries the GL_COMM_ID_BYTES bytes to every rank (any out-of-band
 *                         channel: torch.distributed's store, MPI, a file), every rank calls gl_comm_init_rank (collective, blocking);
 *   one process, N GPUs : gl_comm_init_all on N contexts of N different devices; a thread per context may then call gl_allreduce_min_keys,
 *                         or one thread issues all N calls between gl_comm_group_start / gl_comm_group_end. */
#define GL_COMM_ID_BYTES 128
int gl_comm_unique_id(void *id_out_host);                                                     /* ncclGetUniqueId */
int gl_comm_init_rank(gl_ctx *ctx, const void *id_host, int rank, int nranks, gl_comm **out);  /* ncclCommInitRank on ctx's device */
int gl_comm_init_all(gl_ctx *const *ctxs, int n, gl_comm **out_comms);                         /* ncclCommInitAll; out_comms[n] */
int gl_comm_destroy(gl_comm *comm);
/* ncclCommAbort: ends the communicator and whatever collective of it is still queued or running on ANY of its ranks' streams, without waiting.
 * For the error path of a multi-rank job: a rank that fails before its gl_allreduce_min_keys leaves the other ranks' reduce kernels waiting on the
 * GPU for ever; aborting every local communicator (from any host thread) lets their streams drain.  The handle is freed, as by gl_comm_destroy. */
int gl_comm_abort(gl_comm *comm);
int gl_comm_rank(const gl_comm *comm, int *out_rank, int *out_nranks);
/* keys_dev[q] = min over ranks of keys_dev[q], in place: ncclAllReduce(ncclMin, ncclUint64) queued on the context's stream -- behind the search
 * kernel that wrote the keys, ahead of gl_keys_unpack*; no host synchronisation.  Q x 8 bytes (80 KB at Q = 10^4): latency-bound. */
int gl_allreduce_min_keys(gl_comm *comm, uint64_t *keys_dev, int64_t nq);
/* recv_dev[r * bytes_per_rank ...] = rank r's send block, for every r: ncclAllGather on the context's stream (bytes as ncclUint8).  In place when
 * send_dev == recv_dev + rank * bytes_per_rank.  Used to shard the one part of the path that is replicated otherwise, the VGG16 features of the
 * queries (SURVEY.md 8e "shard it and all-gather if it shows up"): rank r featurises queries [r Q/N, (r+1) Q/N) and the search rows (1.02 MB
 * each at 64 x 64) are gathered; measured on one-rank shares, configs[2] projects to 5.8 x at 8 GPUs with replicated query features. */
int gl_allgather_rows(gl_comm *comm, const void *send_dev, void *recv_dev, int64_t bytes_per_rank);
int gl_comm_group_start(void);                                                                 /* ncclGroupStart */
int gl_comm_group_end(void);                                                                   /* ncclGroupEnd */

/* ---------------------------------------------------------------- DCGAN / WGAN-GP generator */
/* gan_models/dcgan/model_torch.py:75-96 == gan_models/wgangp/model.py:37-58:
 * 4 x [ConvTranspose2d(k4, bias=False) -> BatchNorm2d(eval) -> ReLU] (s1p0 then s2p1 x3),
 * ConvTranspose2d(k4,s2,p1)+bias -> tanh.  Output 64x64. */
int gl_dcgan_create(gl_ctx *ctx, int z_dim, int channels_img, int features_g, gl_dcgan **out);
int gl_dcgan_destroy(gl_dcgan *g);
/* weights in the reference's state_dict layouts, HOST pointers (PyTorch only reads the .pth):
 * layer 0..3: gen.{layer}.0.weight [C_in][C_out][4][4]; layer 4: gen.4.weight */
int gl_dcgan_set_conv_weight(gl_dcgan *g, int layer, const float *w_host);
/* gen.{layer}.1.{weight,bias,running_mean,running_var}, eps = 1e-5 (nn.BatchNorm2d default) */
int gl_dcgan_set_bn(gl_dcgan *g, int layer, const float *gamma_host, const float *beta_host, const float *mean_host,
                    const float *var_host, float eps);
int gl_dcgan_set_out_bias(gl_dcgan *g, const float *bias_host);   /* gen.4.bias */
/* z_dev [n][z_dim] fp32.  Either output may be NULL: out_f32_dev [n][C][64][64] (what
 * Generator.forward returns) and out_u8_dev [n][C][64][64] (the PNG bytes of the generate branch,
 * quantised as gl_quantize_f32 mode 0). */
int gl_dcgan_forward(gl_dcgan *g, const float *z_dev, int64_t n, float *out_f32_dev, uint8_t *out_u8_dev);
/* images per internal pass (activations for that many images stay resident); 0 = default */
int gl_dcgan_set_chunk(gl_dcgan *g, int64_t images_per_pass);
/* arithmetic of the ConvTranspose stack: 0 = fp32 MFMA (every product exact in fp32); 1 (default) = split-fp16: operands are
 * carried as hi + lo halves (~22 mantissa bits), three fp16 MFMAs per product, fp32 accumulation -- same error class,
 * 2-3x faster.  Stacks with the attention block (VAEGAN) always run mode 0. */
int gl_dcgan_set_precision(gl_dcgan *g, int mode);
/* 1 (default): in split-fp16 mode, when the last hidden layer has 64 or 128 channels (features_g = 32 or 64), the 3-channel output layer is computed in that
 * layer's epilogue and its 32 x 32 x C activations are never written to HBM (-9 % on the DCGAN-64 step); 0: separate launches.  Same values up to fp32
 * summation order. */
int gl_dcgan_set_fuse_tail(gl_dcgan *g, int on);
/* VAEGAN generator (gan_models/vaegan/train.py:109-135) = the same ConvTranspose stack with features_g = d/2, plus:
 * the epilogue of layers 0..3 set directly (the caller folds 1/sigma of SpectralNorm, the ConvTranspose bias and
 * BatchNorm into scale/shift), and SelfAttention (gan_models/vaegan/ops.py:86-120) on the 16 x 16 output of layer 2. */
int gl_dcgan_set_affine(gl_dcgan *g, int layer, const float *scale_host, const float *shift_host);
/* SpectralNorm(ConvTranspose2d) of layer 0..3 (gan_models/vaegan/ops.py:23-75): w_bar [C_in][C_out][4][4] (also installs the layer's weights), power-iteration
 * vectors u [C_in] and v [C_out * 16], bn_scale = gamma / sqrt(var + eps) and shift = (conv bias - mean) * bn_scale + beta per output channel.  Every
 * gl_dcgan_forward then advances u, v by `power_iterations` steps ON THE DEVICE and divides the layer's epilogue scale by sigma = u . W v, as the reference does
 * on every forward (also in eval mode).  gl_dcgan_get_spectral_state copies the current u, v back (state_dict). */
int gl_dcgan_set_spectral_norm(gl_dcgan *g, int layer, const float *w_bar_host, const float *u_host, const float *v_host, const float *bn_scale_host,
                               const float *shift_host, int power_iterations);
int gl_dcgan_get_spectral_state(gl_dcgan *g, int layer, float *u_host, float *v_host);
/* hold != 0: forwards reuse the current u, v, sigma (re-running the SAME call, e.g. in the other arithmetic mode) */
int gl_dcgan_set_spectral_hold(gl_dcgan *g, int hold);
/* `times` >= 0 steps of the spectral-norm state on the device, each exactly what one gl_dcgan_forward does before its first layer (the same
 * kernels through the same function), held or not.  A generator loaded with another's weights and current u, v, advanced k times and then
 * held for good is a FIXED function of z, equal bit for bit to that generator's k-th next forward in both precisions: what the
 * partial-black-box and the white-box attack search (gan_models/vaegan/train.py Generator.frozen).  GL_ERR_STATE before the weights are loaded. */
int gl_dcgan_advance_spectral(gl_dcgan *g, int times);
int gl_dcgan_set_attention(gl_dcgan *g, const float *wq_host, const float *bq_host, const float *wk_host, const float *bk_host, const float *wv_host,
                           const float *bv_host, float gamma);
/* The generator's gradient with respect to its latent input (the white-box attack's hot path, csrc/gl_dcgan_grad.hip).  Both calls run
 * their OWN forward with fp32 products, whatever gl_dcgan_set_precision says, keep its post-ReLU activations and go backwards through the
 * same fp32 tap-gather GEMMs: tanh', then per layer the ReLU mask and the BatchNorm scale followed by Conv2d(k4 s2 p1) with the layer's own
 * weights (the data gradient of ConvTranspose2d(k4 s2 p1)), then one GEMM to z_dim columns.  All products are fp32; every output element is
 * one fixed-order sum (no atomics, no split K), so the gradient row of an image does not depend on which images share the call or the pass.
 * Passes honour gl_dcgan_set_chunk and the 3 GiB-per-tensor cap.  The transposed weight packs and the gradient workspaces are allocated on
 * the first gradient call, not before; precision, fuse_tail and chunk are left as found.  n = 0 returns GL_OK; on the context's stream, no
 * synchronisation.
 * Generators with self-attention or spectral normalisation (VAEGAN) are differentiated exactly when their spectral-norm state is held
 * (gl_dcgan_set_spectral_hold): the epilogue scale of a layer is then the constant bn_scale / sigma, and the attention block between layers 2 and 3
 * goes backwards through csrc/gl_attention_grad.hip -- P rebuilt from the forward's q, k rows with the forward's instructions, all products on
 * the fp32 matrix cores, fixed-order in-wave sums, the 1x1 convolutions as one GEMM added to dY in place; the biases and gamma get no gradient.
 * While every forward advances the state, G is no fixed function of z and both calls return GL_ERR_STATE. */
/* vector-Jacobian product: grad_z[n][z_dim] = (dG/dz)^T cot, cot [n][3][64][64] fp32 (NCHW, 16-byte aligned).  out_f32_dev (may be NULL;
 * 16-byte aligned) receives G(z) of the fp32-product forward: the values gl_dcgan_forward gives under precision 0 */
int gl_dcgan_vjp_z(gl_dcgan *g, const float *z_dev, int64_t n, const float *cot_dev, float *grad_z_dev, float *out_f32_dev);
/* loss[i] = sum over the image of (G(z_i) - x_i)^2, x = 2 u/255 - 1 of target_u8 [n][3][64][64] (4-byte aligned); grad_z = d loss / d z.
 * The cotangent 2 (y - x) is formed between the forward and the backward of each pass and never stored for the whole call; the squares
 * are added in double */
int gl_dcgan_l2_grad_z(gl_dcgan *g, const float *z_dev, const uint8_t *target_u8_dev, int64_t n, float *grad_z_dev, float *loss_dev);

/* ---------------------------------------------------------------- PGGAN generator */
/* gan_models/pggan/model_torch.py:49-88 Generator(z_dim, in_channels, img_channels).forward(x, steps, alpha)
 * (WSConv2d :8-22, PixelNorm :25-31, ConvBlock :33-47).  in_channels must be a multiple of 32 and every block that
 * is used must keep >= 32 channels (steps <= 6 at in_channels = 512).  Weights are HOST pointers in the
 * reference's state_dict layouts. */
int gl_pggan_create(gl_ctx *ctx, int z_dim, int in_channels, int img_channels, gl_pggan **out);
int gl_pggan_destroy(gl_pggan *g);
/* initial.1.{weight [z][C][4][4], bias [C]}, initial.3.{conv.weight [C][C][3][3], bias [C]} */
int gl_pggan_set_initial(gl_pggan *g, const float *convt_w_host, const float *convt_b_host, const float *ws_w_host, const float *ws_b_host);
/* prog_blocks.{block}.conv1.{conv.weight, bias}, .conv2.{conv.weight, bias}; block 0..7 */
int gl_pggan_set_block(gl_pggan *g, int block, const float *conv1_w_host, const float *conv1_b_host, const float *conv2_w_host, const float *conv2_b_host);
/* rgb_layers.{j}.{conv.weight [nc][C_j][1][1], bias [nc]}; j = 0 is initial_rgb */
int gl_pggan_set_rgb(gl_pggan *g, int j, const float *w_host, const float *b_host);
int gl_pggan_set_chunk(gl_pggan *g, int64_t images_per_pass);
/* 1 (default) = split-fp16 convolutions (three fp16 MFMAs per product), 0 = fp32 MFMA */
int gl_pggan_set_precision(gl_pggan *g, int mode);
/* z_dev [n][z_dim] -> [n][nc][R][R], R = 4 * 2^steps.  out_f32_dev: what forward() returns; out_u8_dev: the bytes the
 * generate branch writes (gan_models/pggan/train.py:238-246: x*0.5+0.5, ToPILImage).  Either may be NULL. */
int gl_pggan_forward(gl_pggan *g, const float *z_dev, int64_t n, int steps, float alpha, float *out_f32_dev, uint8_t *out_u8_dev);
/* The white-box attack on PGGAN (csrc/gl_pggan_grad.hip): the derivative of Generator.forward(z, steps, alpha) with respect to z [n][z_dim],
 * through the PixelNorm of the latent.  Each call runs the forward with fp32 products itself, whatever gl_pggan_set_precision says, and leaves
 * that setting and gl_pggan_set_chunk's as it found them; the kept activations of one pass (gl_pggan_set_chunk images, by default what fits
 * 1.5 GiB) and the transposed weight packs are allocated by the first gradient call and freed by gl_pggan_destroy.  Every output is one
 * fixed-order fp32 sum: a row does not depend on the images that share the call or the pass.  Depths gl_pggan_forward refuses are refused the
 * same way, unloaded weights with GL_ERR_STATE.  n = 0 returns GL_OK; on the context's stream, no synchronisation. */
/* vector-Jacobian product: grad_z[n][z_dim] = (dG/dz)^T cot, cot [n][nc][R][R] fp32 (NCHW), R = 4 * 2^steps.  out_f32_dev (may be NULL)
 * receives G(z) of the fp32-product forward: the values gl_pggan_forward gives under precision 0 */
int gl_pggan_vjp_z(gl_pggan *g, const float *z_dev, int64_t n, int steps, float alpha, const float *cot_dev, float *grad_z_dev, float *out_f32_dev);
/* loss[i] = sum over the image of (G(z_i) - x_i)^2, x = 2 u/255 - 1 of target_u8 [n][nc][R][R]; grad_z = d loss / d z.  The squares are
 * added in double */
int gl_pggan_l2_grad_z(gl_pggan *g, const float *z_dev, const uint8_t *target_u8_dev, int64_t n, int steps, float alpha, float *grad_z_dev,
                       float *loss_dev);

/* ---------------------------------------------------------------- medGAN (tabular) */
/* gan_models/medgan/model.py:44-73 Generator(z_dim, hidden_size) and :13-41 Autoencoder(input_size, hidden_size, binary).decode,
 * used together at gan_models/medgan/train.py:306-312.  z_dim == hidden_size == 128 (forced by the residual adds). */
int gl_medgan_create(gl_ctx *ctx, int z_dim, int hidden_size, int input_size, int binary, gl_medgan **out);
int gl_medgan_destroy(gl_medgan *g);
/* block 0/1 = gen_block{1,2}: .0.{weight [128][in], bias}, .1.{weight, bias, running_mean, running_var}; eps = 1e-3 (model.py:52,57) */
int gl_medgan_set_gen_block(gl_medgan *g, int block, const float *lin_w_host, const float *lin_b_host, const float *gamma_host, const float *beta_host,
                            const float *mean_host, const float *var_host, float eps);
/* decoder.0.{weight [input_size][hidden], bias [input_size]} */
int gl_medgan_set_decoder(gl_medgan *g, const float *w_host, const float *b_host);
/* Generator.forward: z_dev [n][128] -> hidden_out_dev [n][128] */
int gl_medgan_generate(gl_medgan *g, const float *z_dev, int64_t n, float *hidden_out_dev);
/* Autoencoder.decode: hidden_dev [n][128] -> decoded_dev [n][input_size]; binary_dev (may be NULL) = (decoded >= 0.5), train.py:311-312 */
int gl_medgan_decode(gl_medgan *g, const float *hidden_dev, int64_t n, float *decoded_dev, float *binary_dev);
/* The partial-black-box attack on tables.  gen: a handle with both generator blocks loaded, dec: a handle with the decoder loaded (the same handle where it carries
 * both), both on one context (GL_ERR_INVALID otherwise, GL_ERR_STATE for missing weights); n == 0 returns GL_OK.
 * gl_medgan_codes: codes_u8_dev [n][input_size] = (gl_medgan_decode(dec, gl_medgan_generate(gen, z)) >= 0.5) as bytes 0 / 1 -- the rows the
 * generate branch writes, through the forward's own launches, so bit for bit what gl_medgan_decode's binary_dev holds. */
int gl_medgan_codes(gl_medgan *gen, gl_medgan *dec, const float *z_dev, int64_t n, uint8_t *codes_u8_dev);

/* ---------------------------------------------------------------- VAEGAN encoder (csrc/gl_vaegan_enc.hip) */
/* gan_models/vaegan/train.py:61-96 Encoder(z_dim, d).encode for inference: four Conv2d(k4, s2, p1) + BatchNorm2d + ReLU (3 -> 64 -> 128 ->
 * 256 -> 512 channels, 64 x 64 -> 4 x 4) and two heads Linear(8192, 4 z) + BatchNorm1d + ReLU + Linear(4 z, z).  d must be 64: the reference
 * hard-wires 512 * 4 * 4 inputs to the heads (train.py:79,83), so nothing else loads; 1 <= z_dim <= 4096.
 * Arithmetic: BatchNorm in eval mode with eps 1e-5, folded on the host in double together with the bias, y = s (conv + b - mean) + beta,
 * s = gamma / sqrt(var + eps); fp32 products; every output is one sum in a fixed order that depends on its own image alone, not on the images
 * that share a call or a pass (no atomics, no split K).  A byte u is read as fl32(2 * (u / 255.) - 1) with the expression in float64 -- the lattice of
 * gl_decode_u8 / gl_encode_lattice_f32 --, so the u8 path gives bit for bit what the f32 path gives for those values.  Zero padding pads each layer's input. */
int gl_vaegan_enc_create(gl_ctx *ctx, int z_dim, int d, gl_vaegan_enc **out);
int gl_vaegan_enc_destroy(gl_vaegan_enc *e);
/* images per pass of gl_vaegan_enc_encode (0 = the default, 512: 384 KiB of activations per image); results do not depend on it */
int gl_vaegan_enc_set_chunk(gl_vaegan_enc *e, int64_t images_per_pass);
/* layer 0..3 = cv1 / bn1 .. cv4 / bn4: w_host [Co][Ci][4][4], bias_host [Co], the BatchNorm2d vectors [Co] */
int gl_vaegan_enc_set_conv(gl_vaegan_enc *e, int layer, const float *w_host, const float *bias_host, const float *bn_weight_host, const float *bn_bias_host,
                           const float *bn_running_mean_host, const float *bn_running_var_host);
/* head 0 = fc1 / bn6 / fc1_1 (z_mu), head 1 = fc2 / bn7 / fc2_1 (z_var): fc_w_host [4 z][8192] in the reference's layout (ChannelsToLinear
 * flattens NCHW: column c * 16 + y * 4 + x; repacked here), fc_b_host and the BatchNorm1d vectors [4 z], out_w_host [z][4 z], out_b_host [z] */
int gl_vaegan_enc_set_head(gl_vaegan_enc *e, int head, const float *fc_w_host, const float *fc_b_host, const float *bn_weight_host,
                           const float *bn_bias_host, const float *bn_running_mean_host, const float *bn_running_var_host, const float *out_w_host,
                           const float *out_b_host);
/* images [n][3][64][64], exactly one of images_u8_dev / images_f32_dev non-NULL -> mu_dev, logvar_dev [n][z_dim] fp32 (the reference's z_mu
 * and z_var).  GL_ERR_STATE, naming the missing part, before all six parts are loaded; n == 0 returns GL_OK and touches nothing.  On the
 * context's stream, no synchronisation (the first call, and a call with more images per pass than any before, allocate the workspace). */
int gl_vaegan_enc_encode(gl_vaegan_enc *e, const uint8_t *images_u8_dev, const float *images_f32_dev, int64_t n, float *mu_dev, float *logvar_dev);

/* ---------------------------------------------------------------- LPIPS (0.2 * LPIPS + L2, the reference's fbb distance) */
/* PerceptualLoss(model='net-lin', net='vgg') (attack_models/lpips_pytorch/__init__.py:9-32) -> PNetLin
 * (models/networks_basic.py:134-181) on torchvision's VGG16 `features` (models/pretrained_networks.py:96-134).
 * Features are computed once per image into a vector V with |V_q - V_n|^2 = 0.2*LPIPS(q,n) + mean((q-n)^2)
 * (attack_models/utils.py:176); see gan-leaks_amd/csrc/gl_lpips.hip. */
int gl_lpips_create(gl_ctx *ctx, gl_lpips **out);
int gl_lpips_destroy(gl_lpips *l);
/* conv_index 0..12 = torchvision vgg16().features convs {0,2,5,7,10,12,14,17,19,21,24,26,28}: weight [C_out][C_in][3][3], bias [C_out]; HOST pointers */
int gl_lpips_set_conv(gl_lpips *l, int conv_index, const float *w_host, const float *bias_host);
/* layer 0..4 = lin{layer}.model.1.weight of pretrained_models/v0.1/vgg.pth, [C] floats, all >= 0; HOST pointer */
int gl_lpips_set_lin(gl_lpips *l, int layer, const float *w_host);
int gl_lpips_set_chunk(gl_lpips *l, int64_t images_per_pass);
/* arithmetic of the 13 VGG16 convolutions: 1 (default) = split-fp16 (three fp16 MFMAs per product), 0 = fp32 MFMA */
int gl_lpips_set_precision(gl_lpips *l, int mode);
/* split-fp16 mode only: how activations are scaled into the fp16 halves.  1 (default) = one power of two per layer, chosen when the split path
 * first runs from a calibration pass of the fp32 pipeline over 16 fixed synthetic images (the same scales in every process and context for the
 * same weights; the layer's largest calibration activation lands in [1024, 2048) of the fp16 range 65504: 32-64 x headroom, full 22-bit
 * operands down to ~6e-5 of that maximum); 0 = the fixed factor 4 for every layer (rounds 1-2: fine while activations are O(1), saturates
 * beyond 16 376).  A store that still has to clamp is counted either way (gl_ctx_h3_saturations). */
int gl_lpips_set_calibration(gl_lpips *l, int enabled);
/* length of V for H x W images: sum_l C_l H_l W_l + 3 H W  (512 000 at 64 x 64); -1 if H or W is not a multiple of 16 */
int64_t gl_lpips_feature_dim(int H, int W);
/* images [n][3][H][W] (8-bit codes, or fp32 in [-1,1]) -> V_dev [n][K] feature rows of 4*K bytes each (opaque: every 32 values are
 * stored as 32 hi + 32 lo halves of V * 2^14, see csrc/gl_lpips.hip) and norms_dev [n] = |V|^2 */
int gl_lpips_features_u8(gl_lpips *l, const uint8_t *img_u8_dev, int64_t n, int H, int W, float *V_dev, float *norms_dev);
int gl_lpips_features_f32(gl_lpips *l, const float *img_f32_dev, int64_t n, int H, int W, float *V_dev, float *norms_dev);
/* The image gradient of the distance (csrc/gl_lpips_grad.hip): for y [n][3][H][W] fp32 and targets x = 2 u / 255 - 1 of 8-bit codes,
 *   loss[i] = 0.2 * LPIPS(y_i, x_i) + mean_k (y_i - x_i)^2   (Loss('l2-lpips'), attack_models/utils.py:166-176)   and   cot = d loss / d y,
 * [n][3][H][W] fp32.  The call runs VGG16 with fp32 products whatever gl_lpips_set_precision says (precision, calibration and chunk stay as
 * they are), keeps every activation of a pass and goes backwards through the taps, the max-pools, the ReLUs and the convolutions; every output
 * is one fixed-order fp32 sum, so a row depends on its image alone.  A pass is gl_lpips_set_chunk's images, by default what fits 4 GiB of kept
 * activations (4.9 MB per 64 x 64 image).  Where all channels of a tap position are zero the projection term of the normalisation's gradient
 * is taken as 0.  ref_dev: the targets' normalised tap values from gl_lpips_ref_rows_u8, [n][gl_lpips_ref_dim(H, W)] fp32 -- the targets of a
 * descent do not change, so their forward runs once; NULL: the call computes them itself, with the same result bit for bit.
 * gl_lpips_ref_dim: sum_l C_l H_l W_l floats per image (499 712 at 64 x 64), -1 where gl_lpips_feature_dim is -1.
 * n == 0 returns GL_OK; NULL pointers (ref_dev apart) and H, W that are no multiples of 16: GL_ERR_INVALID; weights not loaded: GL_ERR_STATE.
 * Asynchronous on the context's stream. */
int64_t gl_lpips_ref_dim(int H, int W);
int gl_lpips_ref_rows_u8(gl_lpips *l, const uint8_t *target_u8_dev, int64_t n, int H, int W, float *ref_dev);
int gl_lpips_grad_image(gl_lpips *l, const float *y_f32_dev, const uint8_t *target_u8_dev, const float *ref_dev, int64_t n, int H, int W,
                        float *cot_dev, float *loss_dev);
/* keys[q] = min(keys[q], (float_bits(max(|V_q|^2 + |V_n|^2 - 2 V_q.V_n, 0)) << 32) | (index_base + n)), n < n_rows.
 * custom_knn (attack_models/fbb.py:73-88) with Loss('l2-lpips'); unpack with gl_keys_unpack_f32.  The contraction runs as three
 * fp16 MFMAs per product on the hi/lo halves (fp32 accumulation). */
int gl_feat_knn(gl_ctx *ctx, const float *bank_V_dev, const float *bank_norm_dev, int64_t n_rows, int64_t index_base, const float *query_V_dev,
                    const float *query_norm_dev, int64_t nq, int64_t K, uint64_t *keys_dev);
/* Search rows: the same V with ONE half per LPIPS value (V * 2^14 rounded once; measured effect on a distance <= 3e-7) and the image part kept
 * as hi/lo halves in three segments (query rows [hi|hi|lo], bank rows [hi|lo|hi], each padded to a multiple of 64), so that a plain fp16 dot of a
 * query row and a bank row is the split-fp16 product for the L2 term.  Row length gl_lpips_search_dim(H, W) halves (536 576 at 64 x 64 = 1.07 MB per
 * image instead of 2.05 MB).  role: 0 = query rows, 1 = bank rows.  norms_dev [n] = |row|^2 of the values the rows actually hold. */
int64_t gl_lpips_search_dim(int H, int W);
int gl_lpips_search_features_u8(gl_lpips *l, const uint8_t *img_u8_dev, int64_t n, int H, int W, int role, void *V16_dev, float *norms_dev);
int gl_lpips_search_features_f32(gl_lpips *l, const float *img_f32_dev, int64_t n, int H, int W, int role, void *V16_dev, float *norms_dev);
/* Lattice search rows, for 8-bit images on BOTH sides of the search (what fbb reads from PNG files, utils.py:60-84): a pixel 2 c / 255 - 1
 * is (2 c - 255) / 255, so with the row scale u = gl_lpips_lattice_scale(H, W) = 255 sqrt(3 H W) 2^e the image part of a row is the exact
 * fp16 integer (2 c - 255) 2^e: one K segment instead of the three of the hi / lo form, row length gl_lpips_lattice_dim(H, W) =
 * K_lpips + 3 H W halves (512 000 at 64 x 64), the L2 term exact up to the fp32 accumulation.  Queries and bank rows have the same
 * layout.  Search with gl_feat_knn_h1_scaled(..., K1 = gl_lpips_lattice_dim, row_scale = gl_lpips_lattice_scale). */
int64_t gl_lpips_lattice_dim(int H, int W);
float gl_lpips_lattice_scale(int H, int W);
/* MEMORY LAYOUT of fp16 search rows (both forms: gl_lpips_search_dim / gl_lpips_lattice_dim halves per row = K1), decided by K1 alone so that the
 * writers (gl_lpips_*_features_*) and the search (gl_feat_knn_h1*) agree without a flag:
 *   K1 * 2 <  2 MiB (images up to ~80 x 80) : row-major, V16_dev[row * K1 + k]
 *   K1 * 2 >= 2 MiB (96 x 96 and larger)   : K-blocked, half k of row r at byte ((r / 256) * (K1 / 64) + k / 64) * 32768 + (r % 256) * 128 + (k % 64) * 2
 *     -- the search reads the same 128-byte K slice of a tile's 256 + 256 rows together; with 16 MiB rows that is 512 different 2 MiB pages per slice
 *     (measured: 44 % of the TLB lookups missed, the kernel ran 17 % below its 64 x 64 rate); blocked, it is two contiguous 32 KiB pieces.
 * A buffer for n rows must hold gl_lpips_search_rows_capacity(n, K1) rows (n, or n rounded up to a multiple of 256), and V16_dev must point at a
 * multiple of 256 rows of its buffer when blocked.  Rows are opaque to callers either way (only |row|^2 and the keys come back). */
int64_t gl_lpips_search_rows_capacity(int64_t n, int64_t K1);
int gl_lpips_lattice_features_u8(gl_lpips *l, const uint8_t *img_u8_dev, int64_t n, int H, int W, void *V16_dev, float *norms_dev);

/* gl_feat_knn on search rows: same keys, one fp16 MFMA per product, 256 x 256 tiles.  K1 = gl_lpips_search_dim.
 * gl_feat_knn_h1_scaled: rows stored as V * row_scale (gl_feat_knn_h1: 2^14, the scale of gl_lpips_search_features_*). */
int gl_feat_knn_h1_scaled(gl_ctx *ctx, const void *bank_V16_dev, const float *bank_norm_dev, int64_t n_rows, int64_t index_base, const void *query_V16_dev,
                          const float *query_norm_dev, int64_t nq, int64_t K1, uint64_t *keys_dev, float row_scale);
int gl_feat_knn_h1(gl_ctx *ctx, const void *bank_V16_dev, const float *bank_norm_dev, int64_t n_rows, int64_t index_base, const void *query_V16_dev,
                   const float *query_norm_dev, int64_t nq, int64_t K1, uint64_t *keys_dev);
/* ---- epsilon-ball counts and the distance matrix under 0.2 LPIPS + L2, the distance fbb.main hard-wires (attack_models/fbb.py:148,
 * Loss('l2-lpips'), attack_models/utils.py:166-176).  The kernels are the searches above with another epilogue -- same main loop, K segments and
 * order of the segment totals -- so the fp32 value they reduce,
 *     D32(q, n) = fmaxf(fmaf(-2 / row_scale^2, dot(q, n), |q|^2 + |n|^2), 0),
 * is bit for bit the distance gl_feat_knn_h1_scaled / gl_feat_knn pack into keys[q] for that pair (what gl_keys_unpack_f32 returns).
 *
 * gl_feat_count_h1_scaled (fp16 search rows, either layout, row-major or K-blocked) / gl_feat_count (split rows):
 *     counts_dev[q * pitch + col0 + t] += #{ n in [0, n_rows) : D32(q, n) <= thr_host[t] },  t < n_thr
 * thr_host: n_thr (1..GL_COUNT_MAX_T) fp32 thresholds in HOST memory, ascending (equal neighbours and +inf allowed), none negative or NaN -- a
 * caller with negative radii leaves their columns out (nothing meets them) and passes the rest through col0.  counts_dev is a [nq][pitch] uint64
 * table of gl_counts_init (col0 + n_thr <= pitch <= GL_COUNT_MAX_T); gl_counts_add is the cross-shard sum.  Accumulates, so a streamed bank is
 * counted chunk by chunk; counting the same rows twice counts them twice.  No bank index is involved.  Row, norm, size and scale arguments and
 * their checks as gl_feat_knn_h1_scaled / gl_feat_knn (K1 % 64 == 0, K % 32 == 0, rows 16-byte aligned, K-blocked rows at a multiple of 256 rows of
 * their buffer); n_rows == 0 or nq == 0 is GL_OK.  One kernel, no pairwise value is written to memory; the counts do not depend on tile position,
 * chunking, query slicing, sharding or on which of the two persistent kernels the device gets.  Asynchronous on the context's stream. */
int gl_feat_count_h1_scaled(gl_ctx *ctx, const void *bank_V16_dev, const float *bank_norm_dev, int64_t n_rows, const void *query_V16_dev,
                            const float *query_norm_dev, int64_t nq, int64_t K1, float row_scale, const float *thr_host, int n_thr, int col0, int pitch,
                            uint64_t *counts_dev);
int gl_feat_count(gl_ctx *ctx, const float *bank_V_dev, const float *bank_norm_dev, int64_t n_rows, const float *query_V_dev, const float *query_norm_dev,
                  int64_t nq, int64_t K, const float *thr_host, int n_thr, int col0, int pitch, uint64_t *counts_dev);
/* The same counts with thresholds PER QUERY, on the uint32 pattern of D32 (D32 >= +0: the unsigned order of the patterns is the order of the
 * floats, so the compare is the float32 compare D32 <= float(thr)):
 *     counts_dev[q * n_thr + t] += #{ n in [0, n_rows) : bits(D32(q, n)) <= thr_dev[q][t] },  t < n_thr
 * thr_dev: [nq][n_thr] int64 in DEVICE memory, 8-byte aligned, n_thr in 1..GL_COUNT_MAX_T, ascending within each row (the caller's contract, as
 * for gl_l2_count_rows_i8: the rows are not read on the host); a negative value counts nothing, a value >= 0x7F800000 (+inf) every pair.
 * counts_dev [nq][n_thr] uint64 of gl_counts_init, 8-byte aligned.  The primitive under one radius per query and under the exact k-th
 * smallest distance per query for any k under the distance fbb.main hard-wires (attack_models/fbb.py:148; custom_knn, fbb.py:73-88, beyond
 * GL_TOPK_MAX): a host search over these counts, 16 thresholds per query and pass.  Row, norm, size and scale arguments, their checks and
 * the choice between the three kernels as gl_feat_count_h1_scaled / gl_feat_count; n_rows == 0 or nq == 0 is GL_OK and touches nothing.
 * One kernel (the count's main loop with gl_l2_count_rows_i8's epilogue); the counts do not depend on tile, chunking, query slicing, sharding
 * or kernel.  Asynchronous.  Reports as GL_PROF_FEAT_COUNT. */
int gl_feat_count_rows_h1_scaled(gl_ctx *ctx, const void *bank_V16_dev, const float *bank_norm_dev, int64_t n_rows, const void *query_V16_dev,
                                 const float *query_norm_dev, int64_t nq, int64_t K1, float row_scale, const int64_t *thr_dev, int n_thr,
                                 uint64_t *counts_dev);
int gl_feat_count_rows(gl_ctx *ctx, const float *bank_V_dev, const float *bank_norm_dev, int64_t n_rows, const float *query_V_dev,
                       const float *query_norm_dev, int64_t nq, int64_t K, const int64_t *thr_dev, int n_thr, uint64_t *counts_dev);
/* Kernel-density (soft-min) sums under 0.2 LPIPS + L2, the distance fbb.main hard-wires (attack_models/fbb.py:148):
 *     sums_dev[q * n_coef + t] += sum over n in [0, n_rows) of gl_kde_weight_f32(D32(q, n), D0_dev[q], coef_host[t]),
 * D32 the float32 distance gl_feat_knn* minimises and gl_feat_count* counts, bit for bit (the same main loop with another epilogue).
 * D0_dev, bound_dev, coef_host, sums_dev, the below-offset error, the flag and the synchronisation: as gl_l2_kde_rows_f32 (D32 is never NaN
 * here).  Row, norm, size and scale arguments, their checks and the choice between the three kernels as gl_feat_count_rows_h1_scaled /
 * gl_feat_count_rows; n_rows == 0 or nq == 0 is GL_OK and touches nothing.  The sums do not depend on tile, chunking, query slicing,
 * sharding or kernel.  Reports as GL_PROF_FEAT_COUNT. */
int gl_feat_kde_rows_h1_scaled(gl_ctx *ctx, const void *bank_V16_dev, const float *bank_norm_dev, int64_t n_rows, const void *query_V16_dev,
                               const float *query_norm_dev, int64_t nq, int64_t K1, float row_scale, const float *D0_dev, const uint32_t *bound_dev,
                               const float *coef_host, int n_coef, uint64_t *sums_dev);
int gl_feat_kde_rows(gl_ctx *ctx, const float *bank_V_dev, const float *bank_norm_dev, int64_t n_rows, const float *query_V_dev,
                     const float *query_norm_dev, int64_t nq, int64_t K, const float *D0_dev, const uint32_t *bound_dev, const float *coef_host,
                     int n_coef, uint64_t *sums_dev);
/* The histogram of ALL pair distances under 0.2 LPIPS + L2 (the primitive under an exact quantile of the nq x n_rows values D32(q, n): the
 * percentile heuristic for the radius of the Monte-Carlo attack under the reference's fbb distance).  D32 >= +0 and never NaN, so the
 * unsigned order of the uint32 patterns bits(D32) is the order of the floats.  For a window (lo: uint32, 0 <= shift <= 31,
 * 1 <= n_bins <= GL_HIST_MAX_BINS):
 *     hist_dev[b] += #{ q < nq, n < n_rows : lo <= bits(D32(q, n)) and (bits(D32(q, n)) - lo) >> shift == b },  b < n_bins;
 * pairs outside the window are not counted; the window is cut at 0x7F800000 (+inf, which is inside) and one above it returns at once.
 * hist_dev [n_bins] uint64 of gl_hist_init, 8-byte aligned; accumulates, so a streamed bank is binned chunk by chunk; shards are summed with
 * gl_counts_add(dst, src, nq = n_bins, n_thr = 1, n_lists).  Row, norm, size and scale arguments, their checks and the choice between the
 * three kernels as gl_feat_count_h1_scaled / gl_feat_count; n_rows == 0 or nq == 0 is GL_OK.  One kernel (the count's main loop with
 * gl_l2_hist_i8's binning epilogue), no pairwise value is written to memory; integer adds of a value that does not depend on where a pair
 * sits, so the histogram does not depend on tile, chunking, query slicing, sharding or kernel.  Asynchronous.  Reports as
 * GL_PROF_FEAT_COUNT, the id of the other reductions over the same pair loop. */
int gl_feat_hist_h1_scaled(gl_ctx *ctx, const void *bank_V16_dev, const float *bank_norm_dev, int64_t n_rows, const void *query_V16_dev,
                           const float *query_norm_dev, int64_t nq, int64_t K1, float row_scale, uint32_t lo, int shift, int n_bins,
                           uint64_t *hist_dev);
int gl_feat_hist(gl_ctx *ctx, const float *bank_V_dev, const float *bank_norm_dev, int64_t n_rows, const float *query_V_dev, const float *query_norm_dev,
                 int64_t nq, int64_t K, uint32_t lo, int shift, int n_bins, uint64_t *hist_dev);
/* out_dev[q * ld + n] = D32(q, n) for q < nq, n < n_rows (ld >= n_rows floats per query): the matrix itself, for small cases -- the distance
 * histogram a radius is chosen from, and an exact handle on the per-pair values (its row minimum is the search's distance). */
int gl_feat_pair_dist_h1_scaled(gl_ctx *ctx, const void *bank_V16_dev, const float *bank_norm_dev, int64_t n_rows, const void *query_V16_dev,
                                const float *query_norm_dev, int64_t nq, int64_t K1, float row_scale, float *out_dev, int64_t ld);
int gl_feat_pair_dist(gl_ctx *ctx, const float *bank_V_dev, const float *bank_norm_dev, int64_t n_rows, const float *query_V_dev,
                      const float *query_norm_dev, int64_t nq, int64_t K, float *out_dev, int64_t ld);
/* ---- the K nearest bank rows of every query under 0.2 LPIPS + L2: custom_knn (attack_models/fbb.py:73-88) under the distance fbb.main
 * hard-wires (fbb.py:148) keeping the args.K nearest samples (fbb.py:32) instead of one.  Row q of topk_keys_dev ([nq][k] keys of gl_topk_init,
 * 1 <= k <= GL_TOPK_MAX) becomes the k smallest of what it held and the keys
 *     float_bits(D32(q, n)) << 32 | (index_base + n),  n < n_rows,
 * D32 as above: the bits gl_feat_knn_h1_scaled / gl_feat_knn pack for that pair, so column 0 is their key and the lists are ordered by
 * (D32, global index) -- D32 >= +0, where the order of the bit patterns is the order of the floats.  A function of the set of keys alone: no
 * dependence on tile, slicing, chunking or sharding, and gl_topk_merge folds the lists of other shards.  Accumulates across calls like
 * gl_l2_topk_i8 and like it is not idempotent: a global index may be folded in at most once.  index_base >= 0, index_base + n_rows <= 2^32.
 * Row, norm, size and scale arguments and their checks as gl_feat_count_h1_scaled / gl_feat_count; n_rows == 0 or nq == 0 is GL_OK.
 * The pair kernels run once whatever k is, storing D32 of one slice of queries x bank rows (whole tiles: 256 for fp16 rows, 128 for split rows;
 * whole super-tiles of 1024 x 2048 on the clustered kernel when they fit) in a workspace from gl_malloc of at most 1 GiB
 * (gl_topk_set_workspace); the selection of gl_l2_topk_i8 keeps the k smallest keys.  Reports as GL_PROF_FEAT_COUNT (pairs) and
 * GL_PROF_TOPK_SELECT (selection).  Synchronises when it returns its workspace (gl_free). */
int gl_feat_topk_h1_scaled(gl_ctx *ctx, const void *bank_V16_dev, const float *bank_norm_dev, int64_t n_rows, int64_t index_base,
                           const void *query_V16_dev, const float *query_norm_dev, int64_t nq, int64_t K1, float row_scale, int k,
                           uint64_t *topk_keys_dev);
int gl_feat_topk(gl_ctx *ctx, const float *bank_V_dev, const float *bank_norm_dev, int64_t n_rows, int64_t index_base, const float *query_V_dev,
                 const float *query_norm_dev, int64_t nq, int64_t K, int k, uint64_t *topk_keys_dev);
/* [nq][k] keys of gl_feat_topk* -> dist_dev [nq][k] fp32 = the float whose bits are key >> 32, idx_dev [nq][k] int64 = key & 0xFFFFFFFF
 * (gl_keys_unpack_f32 per slot); an empty slot gives +inf and -1. */
int gl_topk_unpack_f32(gl_ctx *ctx, const uint64_t *topk_keys_dev, int64_t nq, int k, float *dist_dev, int64_t *idx_dev);
/* mean((y-x)^2) + argmin for ARBITRARY fp32 rows on the matrix cores (an alternative to the bit-reproducible VALU path gl_l2_knn_f32; ~15-60x
 * faster; distances agree to ~3e-6 * mean(x^2), i.e. ~1e-6 absolute for rows in [-1,1]): rows are stored as hi + lo halves of x * 2^e with a per-row power of two,
 * dist = |y|^2/d + |x|^2/d - 2 y.x/d with three fp16 MFMAs per product and fp32 accumulation.  V_dev: [n][gl_rows_split_dim(d)] 4-byte slots,
 * norms_dev [n] = |x|^2 / d, scales_dev [n] = 2^-e.  Keys as gl_l2_knn_f32 (unpack with gl_keys_unpack_f32). */
int64_t gl_rows_split_dim(int64_t d);
int gl_rows_split_f32(gl_ctx *ctx, const float *rows_f32_dev, int64_t n, int64_t d, void *V_dev, float *norms_dev, float *scales_dev);
int gl_rows_knn_split(gl_ctx *ctx, const void *bank_V_dev, const float *bank_norm_dev, const float *bank_scale_dev, int64_t n_rows, int64_t index_base,
                      const void *query_V_dev, const float *query_norm_dev, const float *query_scale_dev, int64_t nq, int64_t d, uint64_t *keys_dev);
/* custom_knn with Loss('l2-lpips') -- the reference's default fbb distance (attack_models/fbb.py:148) -- for host-resident 8-bit images in ONE call:
 * BATCH_SIZE truncation (fbb.py:77), search rows, the bank streamed through HBM so that about max_device_bytes (0 = 64 GiB) of feature rows are
 * resident at a time.  Returns GL_ERR_EMPTY_BANK where the reference raises at fbb.py:83. */
int gl_fbb_knn_lpips_host(gl_ctx *ctx, gl_lpips *l, const uint8_t *bank_u8_host, int64_t n_bank, const uint8_t *queries_u8_host, int64_t nq, int H, int W,
                          int64_t batch_size, int64_t max_device_bytes, float *dist_host, int64_t *idx_host);
/* Loss('l2-lpips').forward: per row, out_lpips = LPIPS and out_l2 = mean((y-x)^2) between V_hat[i] and V_gt[b_gt == 1 ? 0 : i];
 * K_lp = K - 3 H W is the length of the LPIPS part of V */
int gl_feat_rows_dist(gl_ctx *ctx, const float *V_hat_dev, int64_t b, const float *V_gt_dev, int64_t b_gt, int64_t K, int64_t K_lp, float *out_lpips_dev,
                      float *out_l2_dev);

#ifdef __cplusplus
}
#endif
#endif /* GANLEAKS_H */
