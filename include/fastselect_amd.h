/*
 * fastselect_amd.h -- C ABI of the MI355X Relief-family scoring engine.
 *
 * The reference (GavinLynch04/FastSelect v0.2.0) has no native FFI: its
 * hot-path boundary is the private Python "host callers" that each estimator's
 * fit() invokes once per fit.  The one-shot entry points below replace those
 * callers one-for-one (same arguments and meaning, plus a backend selector),
 * so the Python estimators call exactly one C function per fit:
 *
 *   fs_multisurf_score  replaces _multisurf_cpu_host_caller  (MultiSURF.py:256-270)
 *                       and      _multisurf_gpu_host_caller  (MultiSURF.py:147-162)
 *   fs_relieff_score    replaces _relieff_cpu_host_caller    (ReliefF.py:222-236)
 *                       and      _relieff_gpu_host_caller    (ReliefF.py:127-134)
 *   fs_surf_score       replaces _surf_cpu_host_caller       (SURF.py:198-218)
 *                       and      _surf_gpu_host_caller       (SURF.py:117-128)
 *
 * Every one-shot call is synchronous, takes caller-owned host arrays that must
 * stay valid for the duration of the call, and writes scores ALREADY DIVIDED
 * BY n (as the host callers return them).  Device memory is allocated and
 * freed inside the call; no pointer to caller memory is retained.
 *
 * The fs_plan_* entry points expose the same MultiSURF path split at its
 * three exchange points (per-row distance moments, per-row neighbour counts,
 * per-feature score sums) so that one process per GPU can shard the pair
 * tiles across ranks and sum those three small vectors with a collective
 * (RCCL all-reduce over xGMI, driven by torch.distributed in
 * fastselect_amd/parallel.py).  With world == 1 the stages compose to exactly
 * fs_multisurf_score.
 *
 * Errors: every function returns FS_OK (0) or a negative FS_E* code; a
 * thread-local human-readable message is available from fs_last_error().
 * The Python layer maps FS_EINVAL -> ValueError, FS_ENODEV / FS_EHIP /
 * FS_ENOTSUP -> RuntimeError, FS_EOOM -> MemoryError.
 *
 * Backends: FS_BACKEND_GPU runs the hand-written HIP kernels for gfx950
 * (MI355X) and fails with FS_ENODEV when no HIP device is visible -- it never
 * falls back to the CPU.  FS_BACKEND_CPU runs the native multithreaded CPU
 * implementation of the same pipeline (the reference's backend='cpu').
 */
#ifndef FASTSELECT_AMD_H
#define FASTSELECT_AMD_H

#include <stdint.h>

#if defined(__GNUC__)
#define FS_API __attribute__((visibility("default")))
#else
#define FS_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define FS_OK 0
#define FS_EINVAL (-1)   /* bad argument (shape, pointer, parameter) */
#define FS_ENODEV (-2)   /* GPU backend requested but no HIP device visible */
#define FS_EOOM (-3)     /* host or device allocation failed */
#define FS_EHIP (-4)     /* HIP runtime / kernel launch error */
#define FS_ENOTSUP (-5)  /* combination not supported by this build */

#define FS_BACKEND_CPU 0
#define FS_BACKEND_GPU 1

#define FS_ACCUM_FAST 0       /* default: symmetric pair weights, float64 partial sums */
#define FS_ACCUM_REFERENCE 1  /* the reference's float32 per-sample chains and column sums */

/*
 * Accumulation mode of the calling thread's subsequent scoring calls and
 * plan creations (a plan keeps the mode it was created with).  No reference
 * counterpart: the reference has one arithmetic, its kernels' float32 sums
 * (MultiSURF.py:198-253, ReliefF.py:181-220).
 *   FS_ACCUM_FAST       the default pass 2: each pair's two directed weights
 *                       folded into one, float32 streams summed in float64.
 *                       10-60x closer to the exact (float64) sums than the
 *                       reference's own float32 sums (DESIGN.md §The oracle).
 *   FS_ACCUM_REFERENCE  MultiSURF / MultiSURF*: every focal sample's hit and
 *                       miss diffs summed in float32 in ascending j, divided,
 *                       temp = miss - hit in float32, then each feature's
 *                       float32 sequential column sum; ReliefF: float32 temp of
 *                       the float64 update over argsort-ordered neighbours and
 *                       the same column sums.  MultiSURF then runs pass 1 on
 *                       32-bit operands with exact thresholds for every
 *                       flagged row.  SURF / SURF*: the reference's order at
 *                       n_jobs = 1 (its one fixed order; with more numba
 *                       threads it adds per-thread rows in schedule order,
 *                       SURF.py:195, 216): four float32 chains per sample in
 *                       ascending j, score_update in float32, one sequential
 *                       float32 sum over the samples (SURF.py:139-218).  The
 *                       scores are then bit-identical to the oracle's
 *                       sequential restatement of the reference's float32
 *                       order (oracle/relief_oracle.c; tests/test_refacc*.py).
 *                       The reference kernels are @njit(fastmath=True), which
 *                       lets LLVM reassociate its float64 distance sums; no
 *                       reference-produced fixture pins that level, so parity
 *                       with numba's own bits is unpinned.  The
 *                       one-shot calls and fs_*_score_devices with more than
 *                       one device run on one device (FS_ENOTSUP otherwise);
 *                       GPU MultiSURF plans with world > 1 run pass 2 as
 *                       fs_plan_ref_masks / fs_plan_ref_pass2 /
 *                       fs_plan_ref_sums, row plans (ReliefF, SURF) as
 *                       fs_plan_ref_temp / fs_plan_ref_sums (CPU backend:
 *                       FS_ENOTSUP).
 * previous (nullable) receives the mode in force before the call.  The mode
 * is per thread: a caller that scores from several threads passes it per
 * call instead (fs_*_score_ex below).
 */
FS_API int fs_set_accumulation(int mode, int* previous);
FS_API int fs_get_accumulation(void);

/*
 * TEST-ONLY: override one internal choice of the library for the calls that
 * follow, process-wide (tests/ uses it to reach routes the automatic choices
 * take only at other sizes; no product code calls it).  name = "reset"
 * restores every default; the others are listed in INTEGRATION.md §4
 * ("ksplit", "q16", "sparse", "shards", "q16_guard_off", "thr_exact_all",
 * "exact_gather", "row_panel",
 * "rf_xlds", "rf_fcap", "ties_1w", "ties_coop", "rf_ref_replay", "ref_q16", "surf_f64",
 * "colsort_bins12", "colsort_global", "star_split", "colsort_star", "mi_tiles",
 * "list_cap", "cfs_rows_cap", "seg_len", "pass2_generic", "mdr_top_cap",
 * "mdr_ranks", "mdr_blocks", "mdr_labels", "pair_tiles", "pair_cap", "pair_labels",
 * "pair_lab_ranks", "stir_chunk", "stir_seg_len", "star_dense_ranks").  FS_EINVAL for an unknown name.
 * Not thread-safe against concurrent scoring calls.
 */
FS_API int fs_test_hook(const char* name, int64_t value);

/* Library identity and device discovery. */
FS_API const char* fs_version(void);
FS_API const char* fs_last_error(void);
/* Number of visible HIP devices (0 when none, never negative). */
FS_API int fs_device_count(void);
/* Free the device blocks the library keeps between calls.  Plans and the
 * column statistics return their device buffers to a per-device cache (up to
 * an eighth of the device's memory, FS_DEVICE_CACHE_MB overrides, 0
 * disables), so that the next fit skips hipMalloc's page mapping (190-310 ms
 * for a cfg4 plan).  Returns FS_OK. */
FS_API int fs_device_cache_release(void);
/* Pinned host memory for the float32 copy of X a fit makes (GPU backend):
 * the host threads cast into pinned, already-mapped pages and the upload of
 * X is a DMA from them.  Blocks are cached between calls (two at most;
 * fs_device_cache_release frees them).  FS_ENODEV without a GPU. */
FS_API int fs_host_alloc(uint64_t bytes, void** out);
FS_API int fs_host_free(void* p);
/* Stage X for one fit: upload the n x p row-major matrix (float32, or
 * float64 when x_is_f64) to `device` once.  Until fs_unstage_x, the GPU
 * backend's fs_column_stats and scoring calls given the same host pointer,
 * shape and dtype, made from the thread that staged it, read the staged copy
 * instead of uploading X again; the caller must not modify x in between.
 * *staged receives the handle. */
FS_API int fs_stage_x(int device, const void* x, int x_is_f64, int64_t n, int64_t p,
                      uint64_t* staged);
/* As fs_stage_x, but X is already on `device` (x_device: n x p row-major,
 * caller-owned, valid until fs_unstage_x, which does not free it): the
 * multi-GPU path uploads each rank's rows and all-gathers the rest over RCCL
 * (fastselect_amd/parallel.py), then registers the gathered copy under the
 * host array's key so that the column statistics and the plan read it. */
FS_API int fs_stage_x_device(int device, const void* x, const void* x_device, int x_is_f64,
                             int64_t n, int64_t p, uint64_t* staged);
/* The float64 -> float32 cast of X (round to nearest, as numpy's astype;
 * x_is_f64 = 0: a float32 X is copied as is) into the caller's `out`
 * (n x p, row-major; pinned memory from
 * fs_host_alloc makes the upload a DMA), fused with the finiteness check of
 * the result (*finite as fs_all_finite) and with fs_stage_x of `out`: row
 * blocks are uploaded while later ones are cast.  *staged = 0 when the device
 * had no room for the copy or a value is not finite (the cast is done either
 * way).  Replaces the cast in scikit-learn's validate_data(dtype=np.float32)
 * that MultiSURF.fit starts with (MultiSURF.py:384-386) plus the upload of
 * the cast array. */
FS_API int fs_stage_x_cast(int device, const void* x, int x_is_f64, int64_t n, int64_t p,
                           int n_jobs, float* out, int* finite, uint64_t* staged);
FS_API int fs_unstage_x(uint64_t staged);
/* *finite = 1 if every element of the n x p float32 / float64 matrix is
 * finite, else 0 (host threads; n_jobs as the scoring calls).  The
 * estimators call it in place of scikit-learn's single-threaded scan and fall
 * back to scikit-learn's own validation, and its error, when it reports 0. */
FS_API int fs_all_finite(const void* x, int x_is_f64, int64_t n, int64_t p, int n_jobs,
                         int* finite);

/*
 * MultiSURF / MultiSURF* feature scores.
 *   x            [n][p] float32, row-major (validated X, MultiSURF.py:384-386)
 *   y            [n] labels as float64; samples are hits when y[i] == y[j]
 *   recip        [p] float32 reciprocal feature ranges (MultiSURF.py:409-412)
 *   feat_idx     [n_kept] feature indices to score, or NULL for all p
 *                (the reference's feat_idx argument, MultiSURF.py:147,256)
 *   use_star     nonzero: MultiSURF* (far misses subtract, MultiSURF.py:236-243)
 *   is_discrete  [p] 0/1 (MultiSURF.py:416-420)
 *   n_jobs       CPU threads (-1 = all); ignored by the GPU backend
 *   device       HIP device ordinal for the GPU backend
 *   scores_out   [n_kept] float32, scores / n
 */
FS_API int fs_multisurf_score(int backend, int device, const float* x, int64_t n, int64_t p,
                       const double* y, const float* recip, const int64_t* feat_idx,
                       int64_t n_kept, int use_star, const uint8_t* is_discrete, int n_jobs,
                       float* scores_out);

/*
 * The decision check of this thread's last GPU fs_multisurf_score call
 * (new; the reference has no quantised pass).  MultiSURF (not MultiSURF*)
 * scored on 16-bit pass-1 operands estimates how far the near/far decisions
 * its quantised thresholds could change move the scores, relative to their
 * largest magnitude (risk_out; -1 when not evaluated: 32-bit operands,
 * MultiSURF*, the q16 test hook set, CPU backend); above 5e-6 the call scores again on
 * 32-bit operands and rerun_out is 1.  Signal-free inputs (scores at the
 * noise floor of the decisions) are what trips it.
 */
FS_API int fs_multisurf_last_guard(double* risk_out, int* rerun_out);

/*
 * MultiSURF / MultiSURF* score SUMS (not divided by n) of the focal samples
 * [row_begin, row_end) only, written to sums_out[n_kept] (host memory).
 * The reference's kernel is a prange over focal samples whose rows are
 * independent once each sample's threshold is known (MultiSURF.py:174-251):
 * thresholds and neighbour counts stay those of the whole fit, and each pair
 * contributes only the side of its focal sample inside the range.  Summing
 * the vectors of a partition of [0, n) and dividing by n gives the one-shot
 * scores up to float64 summation order; [0, 384) of the reference's
 * per-sample rows is the same as oracle i_range=(0, 384).  Other arguments as
 * fs_multisurf_score.
 */
FS_API int fs_multisurf_score_rows(int backend, int device, const float* x, int64_t n,
                                   int64_t p, const double* y, const float* recip,
                                   const int64_t* feat_idx, int64_t n_kept, int use_star,
                                   const uint8_t* is_discrete, int n_jobs, int64_t row_begin,
                                   int64_t row_end, double* sums_out);

/*
 * ReliefF feature scores (ReliefF.py:137-236).
 *   x            [n][p] float32 (the float32 cast of the float64-validated X, ReliefF.py:400)
 *   y_enc        [n] int32 class codes in [0, n_classes) (ReliefF.py:375)
 *   recip        [p] float32 (discrete and zero ranges forced to 1, ReliefF.py:377-380)
 *   is_discrete  [p] 0/1
 *   k            n_neighbors (>= 1)
 *   class_probs  [n_classes] float32 class priors (ReliefF.py:373-374)
 *   scores_out   [p] float32, scores / n
 * Neighbours are chosen as the reference chooses them: by its float32
 * distance key, ties at the k-th key in numba's quicksort order.
 */
FS_API int fs_relieff_score(int backend, int device, const float* x, int64_t n, int64_t p,
                     const int32_t* y_enc, const float* recip, const uint8_t* is_discrete,
                     int64_t k, const float* class_probs, int64_t n_classes, int n_jobs,
                     float* scores_out);

/*
 * SURF / SURF* feature scores (SURF.py:131-218).
 *   x            [n][p] float64, row-major (SURF.py:330-332)
 *   y            [n] int32 labels (y.astype(int32), SURF.py:371)
 *   recip        [p] float32 (SURF.py:352-355)
 *   use_star     nonzero: SURF* (far hits add, far misses subtract)
 *   scores_out   [p] float32, scores / n
 */
FS_API int fs_surf_score(int backend, int device, const double* x, int64_t n, int64_t p,
                  const int32_t* y, const float* recip, int use_star,
                  const uint8_t* is_discrete, int n_jobs, float* scores_out);

/*
 * The three one-shot calls with the accumulation mode as an argument
 * (FS_ACCUM_FAST / FS_ACCUM_REFERENCE, as fs_set_accumulation documents),
 * for that call only: the calling thread's fs_set_accumulation mode is
 * neither read nor changed.  Other arguments as fs_multisurf_score /
 * fs_relieff_score / fs_surf_score, which they replace for callers that do
 * not own the thread they score on (the reference's host callers take no
 * such mode: MultiSURF.py:256, ReliefF.py:222, SURF.py:198).
 */
FS_API int fs_multisurf_score_ex(int backend, int device, const float* x, int64_t n, int64_t p,
                                 const double* y, const float* recip, const int64_t* feat_idx,
                                 int64_t n_kept, int use_star, const uint8_t* is_discrete,
                                 int n_jobs, int accumulation, float* scores_out);
FS_API int fs_relieff_score_ex(int backend, int device, const float* x, int64_t n, int64_t p,
                               const int32_t* y_enc, const float* recip,
                               const uint8_t* is_discrete, int64_t k, const float* class_probs,
                               int64_t n_classes, int n_jobs, int accumulation,
                               float* scores_out);
FS_API int fs_surf_score_ex(int backend, int device, const double* x, int64_t n, int64_t p,
                            const int32_t* y, const float* recip, int use_star,
                            const uint8_t* is_discrete, int n_jobs, int accumulation,
                            float* scores_out);

/*
 * Row-sharded ReliefF / SURF: the float64 score SUMS (not
 * divided by n) of the focal samples [row_begin, row_end) only, written to
 * sums_out[p] (host memory).  Other arguments as fs_relieff_score /
 * fs_surf_score.  Neighbour selection is row-local in both algorithms
 * (ReliefF's k nearest per class, ReliefF.py:144-175; SURF's per-sample mean
 * threshold, SURF.py:146-163), so one process per GPU scores a slice of the
 * samples and a single SUM all-reduce of p doubles combines the slices:
 * summing the vectors of a partition of [0, n) and dividing by n gives the
 * one-shot scores up to float64 summation order.  The GPU computes every
 * distance tile that touches the slice's 128-sample blocks, so slices on
 * 128-sample boundaries (fastselect_amd.parallel.shard_rows) balance best.
 */
FS_API int fs_relieff_score_rows(int backend, int device, const float* x, int64_t n, int64_t p,
                                 const int32_t* y_enc, const float* recip,
                                 const uint8_t* is_discrete, int64_t k, const float* class_probs,
                                 int64_t n_classes, int n_jobs, int64_t row_begin,
                                 int64_t row_end, double* sums_out);
FS_API int fs_surf_score_rows(int backend, int device, const double* x, int64_t n, int64_t p,
                              const int32_t* y, const float* recip, int use_star,
                              const uint8_t* is_discrete, int n_jobs, int64_t row_begin,
                              int64_t row_end, double* sums_out);

/*
 * Single-process multi-GPU scoring (the estimators' `devices=`; SURVEY.md
 * §5 "Config / flags", §8(b) "Threading: one host thread per device").  One
 * host thread per entry of devices[0 .. n_devices) -- ordinals may repeat
 * (several plans share one device) -- with the partitions of the
 * one-process-per-GPU path (fastselect_amd/parallel.py): MultiSURF deals the
 * upper-triangle pair tiles round-robin (tile t -> thread t % N) and sums its
 * three exchange vectors (row moments, neighbour counts, score sums) on the
 * host in thread order after each stage, where the multi-process path
 * all-reduces them over RCCL; ReliefF / SURF give each thread whole 128-sample
 * blocks of the focal range and sum the score vectors once.  Write the
 * float64 score SUMS of the focal samples [row_begin, row_end) (not divided
 * by n; [0, n) for a whole fit) to sums_out.  Other arguments as the
 * one-shot calls; the reference's fit is one call on one device
 * (MultiSURF.py:393-440, ReliefF.py:382-403, SURF.py:339-372).
 */
FS_API int fs_multisurf_score_devices(const int* devices, int n_devices, const float* x, int64_t n,
                                      int64_t p, const double* y, const float* recip,
                                      const int64_t* feat_idx, int64_t n_kept, int use_star,
                                      const uint8_t* is_discrete, int n_jobs, int64_t row_begin,
                                      int64_t row_end, double* sums_out);
FS_API int fs_relieff_score_devices(const int* devices, int n_devices, const float* x, int64_t n,
                                    int64_t p, const int32_t* y_enc, const float* recip,
                                    const uint8_t* is_discrete, int64_t k, const float* class_probs,
                                    int64_t n_classes, int n_jobs, int64_t row_begin,
                                    int64_t row_end, double* sums_out);
FS_API int fs_surf_score_devices(const int* devices, int n_devices, const double* x, int64_t n,
                                 int64_t p, const int32_t* y, const float* recip, int use_star,
                                 const uint8_t* is_discrete, int n_jobs, int64_t row_begin,
                                 int64_t row_end, double* sums_out);

/*
 * Per-column statistics of X: the preprocessing each reference fit() runs on
 * the host before scoring -- x.min(axis=0), x.max(axis=0) and, per column,
 * np.unique(x[:, f]).size compared with discrete_limit (MultiSURF.py:141-144,
 * 409-420; ReliefF.py:366-380; SURF.py:347-355).
 *   x            [n][p] row-major, float32 (x_is_f64 = 0) or float64 (1)
 *   count_cap    distinct values are counted exactly up to count_cap (pass
 *                discrete_limit); a column with more reports count_cap + 1.
 *                The GPU backend supports count_cap <= 8191 (FS_ENOTSUP above)
 *   colmin_out, colmax_out  [p] in x's dtype
 *   ndistinct_out           [p] min(distinct values, count_cap + 1)
 * Equality is numpy's: -0.0 and +0.0 are one value; X must be finite (the
 * estimators validate it first, as the reference does).
 */
FS_API int fs_column_stats(int backend, int device, const void* x, int x_is_f64, int64_t n,
                           int64_t p, int64_t count_cap, void* colmin_out, void* colmax_out,
                           int64_t* ndistinct_out);

/* ---- Sharded MultiSURF plan (one plan per rank) ------------------------ */

typedef struct fs_plan fs_plan;

/*
 * Create a plan and upload its inputs (host arrays, same meaning as
 * fs_multisurf_score).  rank/world select which upper-triangle pair tiles
 * this plan computes (tile t belongs to rank t % world).  `stream` is a
 * hipStream_t (0 = the plan's own stream) on which every GPU stage is
 * enqueued; stages do not synchronise the host unless `stream` is 0.
 */
FS_API int fs_plan_create(fs_plan** plan_out, int backend, int device, const float* x, int64_t n,
                   int64_t p, const double* y, const float* recip, const int64_t* feat_idx,
                   int64_t n_kept, int use_star, const uint8_t* is_discrete, int rank, int world,
                   int n_jobs, uint64_t stream);

/*
 * Re-target the plan to another feature subset of the same samples
 * (feat_idx[n_kept] into the original columns, NULL = all), keeping X and
 * its column ranges resident: the next pass1/select/pass2 score the subset
 * exactly as a fresh plan on X[:, feat_idx] would (the reference scores such
 * subsets through feat_idx, MultiSURF.py:147,256; TuRF refits on them,
 * TuRF.py:93-115).  The scores vector of pass2 then has n_kept entries.
 */
FS_API int fs_plan_set_features(fs_plan* plan, const int64_t* feat_idx, int64_t n_kept);

/*
 * Stage 1: quantise the resident X, compute this rank's distance tiles and
 * write this rank's partials to rowstats[3n]: per row sum D, sum D^2 (D in the
 * plan's integer distance unit) and this rank's share of the mean correction
 * (its slice of the continuous features).  Pointers live in the plan's memory
 * space: device memory for the GPU backend, host memory for the CPU backend.
 */
FS_API int fs_plan_pass1(fs_plan* plan, double* rowstats);
/* Stage 2: thresholds from the all-reduced rowstats[3n], exact recomputation of this rank's ambiguous pairs (pairs whose
 * quantised distance lies so close to a threshold that the near/far decision
 * is not certain), then partial per-row (near hits, near misses) -> counts[2n]. */
FS_API int fs_plan_select(fs_plan* plan, const double* rowstats, double* counts);
/* Stage 3: pair weights from the all-reduced counts[2n]; partial per-feature
 * score sums (NOT divided by n) -> scores[n_kept], in feat_idx order. */
FS_API int fs_plan_pass2(fs_plan* plan, const double* counts, double* scores);
/* STIR ("STatistical Inference Relief", Le, Urbanowicz, Moore and McKinney,
 * Bioinformatics 35(8), 2019): t-statistics for MultiSURF scores from the
 * near pairs of a fit, without permutations.  H is the multiset of ordered
 * pairs (i, j) with j in MultiSURF's near set of focal sample i and
 * y_j == y_i, M the same with y_j != y_i (the plan's own decisions, the ones
 * pass 2 weighs; a pair near from both sides counts twice); per feature the
 * diffs over M and over H are compared with a pooled two-sample t-test
 * (definitions: fastselect_amd/csrc/fs_stir.h).  The test treats the
 * |H| + |M| pairs as independent, which they are not (every sample occurs in
 * many pairs): that is the published method's approximation.
 *
 * fs_plan_stir: sums[4 * n_kept] in the plan's memory space (device memory
 * for the GPU backend, host memory for the CPU backend), sums[q * n_kept + k]
 * with q = 0..3 for S1H, S2H (sum of diff, of diff^2 over H), S1M, S2M, k in
 * feat_idx order.  Like the score sums of fs_plan_pass2 they are this plan's
 * partial sums, not normalised: its pairs are those of its owned tiles, and a
 * side of a pair counts only when its focal sample lies in the
 * fs_plan_set_rows range.  The partials of all (rank, world) plans, of all
 * tile shards and of disjoint row ranges add up to the whole.  Needs a
 * fs_plan_select on the plan's current shard and feature set since the last
 * re-targeting or pass1 (else FS_EINVAL).  MultiSURF* plans: FS_ENOTSUP (no
 * STIR definition); ReliefF / SURF plans: FS_EINVAL.  Works in both
 * accumulation modes (it reads the distances, thresholds and labels only);
 * enqueued on the plan's stream, the host waits only when the stream is the
 * plan's own.  Pass 2's state is untouched: the next fs_plan_pass2 returns
 * the bits it returned before.  The GPU backend sums fixed-point terms
 * exactly: its error is absolute, 1.2e-7 of the plan's largest scaled feature
 * range per diff (and of its square per squared diff), so squares below that
 * count as 0 (fs_stir.h, "Error of the GPU sums").
 *
 * fs_stir_statistics: the host epilogue on the summed sums[4 * n_kept] with
 * |H| = n_hit_pairs (the sum of counts[2i] over the focal rows in use) and
 * |M| = n_miss_pairs (of counts[2i + 1]): per feature the hit and miss means,
 * t = (Mbar - Hbar) / (sp sqrt(1/|M| + 1/|H|)) with the pooled deviation sp
 * (variances clamped at 0; sp == 0: t = +inf, -inf or 0 by the sign of
 * Mbar - Hbar), and *df = |M| + |H| - 2.  All float64; any output may be
 * NULL.  The one-sided p-value P(T_df >= t) is left to the caller.
 * |H| < 2 or |M| < 2: FS_EINVAL. */
FS_API int fs_plan_stir(fs_plan* plan, double* sums);
FS_API int fs_stir_statistics(const double* sums, int64_t n_kept, double n_hit_pairs,
                              double n_miss_pairs, double* hit_mean, double* miss_mean,
                              double* t, double* df);
/* The same, and pooled_sd[n_kept] = sp per feature (or NULL): where it is 0,
 * t is +inf, -inf or 0 by definition and the p-value is 0, 1 or 1 instead of
 * the t distribution's. */
FS_API int fs_stir_statistics_ex(const double* sums, int64_t n_kept, double n_hit_pairs,
                                 double n_miss_pairs, double* hit_mean, double* miss_mean,
                                 double* t, double* df, double* pooled_sd);
/* Summed HIP-event time in milliseconds of the last fs_plan_stir's kernels
 * over its chunks of tiles (GPU only; -1 when unavailable).  which: 0 = the
 * pair-multiplicity kernel, 1 = the score kernel; 2 = k_rf_stir of the last
 * fs_plan_score_stir on a ReliefF plan (-1 when no such call ran). */
FS_API double fs_plan_stir_kernel_ms(const fs_plan* plan, int which);
/* MultiSURF permutation test: many labellings on one plan's decisions.
 *
 * Pass 1 and fs_plan_select do not read the labels: the distances, the
 * thresholds and so the near sets N_i = { j : D_ij < thr_i } hold for every
 * labelling of the samples.  Labels enter the near hit / miss counts H_i, M_i
 * and the pair weights only (near hit -1/H_i, near miss +1/M_i), so the score
 * sums of B labellings are one contraction of the near pairs' diffs with a
 * B-wide weight vector per pair (fastselect_amd/csrc/fs_labels.hip).
 *
 * fs_plan_score_labels: after fs_plan_pass1 + fs_plan_select on a MultiSURF
 * plan, the score sums (not divided by n) of B labellings of the plan's
 * samples on its distances, thresholds and decisions.  labels[b * n + i]:
 * host memory, any int32, compared by equality only (any number of classes).
 * scores[b * n_kept + k], k in feat_idx order, in the plan's memory space
 * like fs_plan_pass2's (device memory for the GPU backend).  The call is
 * synchronous.  The plan must own every tile and the whole row range
 * (world 1 and all focal rows, else FS_ENOTSUP); MultiSURF* plans and plans in
 * reference-order accumulation: FS_ENOTSUP; ReliefF / SURF plans: FS_EINVAL;
 * no fs_plan_select since the last pass 1 or re-targeting: FS_EINVAL.
 * Honours fs_plan_set_features.  Pass 2's state is untouched: the next
 * fs_plan_pass2 returns the bits it returned before.  B = 0: FS_OK, nothing
 * written.  CPU backend: row b is bit for bit what fs_multisurf_score returns
 * (times n) with labelling b as y.  GPU backend: float32 MFMA partials of at
 * most 256 pairs folded into float64, fixed summation order (the same call
 * gives the same bits twice).
 *
 * fs_multisurf_score_labels: one call from host arrays -- the plan with
 * labelling 0 as y, its step (with the 16-bit decision check of
 * fs_multisurf_score), the labellings; scores_out[b * n_kept + k] divided by
 * n.  B >= 1.  FS_ENOTSUP when the distance tiles do not fit one device, or
 * in reference-order accumulation.
 *
 * fs_plan_labels_kernel_ms: summed HIP-event time in milliseconds of the last
 * fs_plan_score_labels' kernels (GPU only; -1 when unavailable).  which: 0 =
 * the near-pair record kernels (once per call), 1 = the counts and weights
 * kernels, 2 = the score kernel (both summed over the chunks of labellings). */
FS_API int fs_plan_score_labels(fs_plan* plan, const int32_t* labels, int64_t B, double* scores);
FS_API int fs_multisurf_score_labels(int backend, int device, const float* x, int64_t n, int64_t p,
                                     const int32_t* labels, int64_t B, const float* recip,
                                     const int64_t* feat_idx, int64_t n_kept,
                                     const uint8_t* is_discrete, int n_jobs, float* scores_out);
FS_API double fs_plan_labels_kernel_ms(const fs_plan* plan, int which);
/* ReliefF permutation test: many labellings on one distance pass.
 *
 * ReliefF's neighbour sets read the labels (the k nearest of every class), so
 * fs_plan_score_labels stays FS_EINVAL for ReliefF plans.  Two things do not
 * read them: the distance pass, and the order in which the reference walks a
 * row (one argsort of its float32 keys): for any labelling the k nearest of a
 * class are the first k of that class on that walk.  These calls run pass 1
 * once and then score the labellings on one of two routes
 * (fastselect_amd/csrc/fs_relieff_labels.hip): the general route, the plan's
 * own selection and update per labelling on the resident keys; and, on the
 * GPU, the fast route, which lists every row's first L candidates of that walk
 * once per call (exact keys, ties in the reference's quicksort order), gives
 * each candidate a weight per labelling and scores 32 labellings at a time
 * with the MFMA kernel of fs_plan_score_labels.  A labelling takes the general
 * route when a class present in it has at most k members, when it has more
 * than 8 classes, when min(ceil(3 k / its smallest class share), n - 1) exceeds
 * 256, when a class ran short of k inside some row's prefix (caught and
 * rerun), and when fewer than 8 labellings of the call qualify for the fast
 * route or its once-per-call prefix is estimated to cost more than two thirds
 * of the general route for them.  L is the smallest of 64, 128, 256 that covers the largest need.
 *
 * fs_plan_relieff_score_labels: the ReliefF score sums (not divided by n) of
 * B labellings of the plan's samples.  labels[b * n + i]: host memory, int32
 * class codes in [0, 64).  The priors of labelling b are
 * (float)((double)count_c / (double)n); a code with no member in a labelling
 * takes no part; neighbours are chosen exactly as fs_relieff_score chooses
 * them (float32 keys, ties in the reference's quicksort order), the self-hit
 * of a class with fewer than k other members included.  scores[b * n_kept +
 * k], k in feat_idx order, in the plan's memory space like fs_plan_score's
 * sums.  The call is synchronous and runs pass 1 for the plan's current
 * feature subset itself (it honours fs_plan_set_features and needs no earlier
 * fs_plan_score).  B = 0: FS_OK, nothing written.  FS_EINVAL: a MultiSURF or
 * SURF plan, a code outside [0, 64), a labelling with fewer than 2 classes
 * present (checked for every labelling before any is scored).  FS_ENOTSUP: a
 * plan that does not own the whole focal range [0, n), or one in
 * reference-order accumulation.  The plan's own labels, priors and neighbour
 * state are restored: a later fs_plan_score returns the bits it returned
 * before.  A general-route row b (every row of the CPU backend) is bit for
 * bit what fs_plan_score of a plan of the same backend created with labelling
 * b returns; a fast-route row has the same neighbours, float32 weights and
 * float32 MFMA partials of at most 256 records folded into float64 (within
 * 1e-5 of the two non-cancelling sums a score is made of).  No float atomics:
 * the same call gives the same bits twice.
 *
 * fs_relieff_score_labels: one call from host arrays (every column scored);
 * scores_out[b * p + f] divided by n.  B >= 1.  Fast accumulation only
 * (FS_ENOTSUP in reference order).
 *
 * fs_plan_relieff_labels_info: out[0..4) of the last completed call: the
 * labellings scored on the fast route (0 on the CPU backend), the labellings
 * sent to the general route by the rule, the fast-route labellings rerun after
 * an overflow, the candidate depth L (0: no fast route).  FS_EINVAL before the
 * first call.
 *
 * fs_plan_relieff_labels_kernel_ms: summed HIP-event time in milliseconds of
 * the last call (GPU only; -1 when unavailable).  which: 0 = the candidate
 * prefix (once per call), 1 = walk and weights, 2 = the score kernel (both
 * summed over the chunks of labellings), 3 = the general route's selection and
 * update, summed over its labellings. */
FS_API int fs_plan_relieff_score_labels(fs_plan* plan, const int32_t* labels, int64_t B,
                                        double* scores);
FS_API int fs_relieff_score_labels(int backend, int device, const float* x, int64_t n, int64_t p,
                                   const int32_t* labels, int64_t B, const float* recip,
                                   const uint8_t* is_discrete, int64_t k, int n_jobs,
                                   float* scores_out);
FS_API int fs_plan_relieff_labels_info(const fs_plan* plan, int64_t out[4]);
FS_API double fs_plan_relieff_labels_kernel_ms(const fs_plan* plan, int which);
/* SURF / SURF* permutation test: many labellings on one distance pass
 * (reference scoring: SURF.py:139-218).
 *
 * SURF's near sets N_i = { j != i : (double)(float)D_ij < avg_i } never read
 * the labels: distances, their exact float32 resolution and the means run
 * once for any number of labellings.  A near side weighs -1 for a hit and +1
 * for a miss, so with s_b(i, j) = +1 where labelling b labels i and j
 * differently, -1 where equally, and c_ij = near_i(j) + near_j(i),
 *
 *   S_surf[f, b] = sum over i < j of s_b(i, j) c_ij d_f(i, j)
 *   S_star[f, b] = 2 S_surf[f, b] - 2 (T_f - 2 Hs[f, b])
 *   T_f = sum over i < j of d_f(i, j),  Hs[f, b] = the same over the pairs of one class under b
 *
 * (fastselect_amd/csrc/fs_surf_labels.hip).  Hs comes from one label-free
 * sort of the column per call and one walk over it per labelling.
 *
 * fs_plan_surf_score_labels (SURF.py:139-218): the score sums (not divided by
 * n) of the plan's current feature set with labelling b as y; SURF or SURF*
 * as the plan's use_star says.  labels[b * n + i]: host memory, int32,
 * compared by equality only.  scores[b * n_kept + k] in the plan's memory
 * space like fs_plan_score's sums (device memory for a GPU plan, host memory
 * for a CPU plan).  The call is synchronous, runs the distance stage itself
 * and honours fs_plan_set_features; a later fs_plan_score returns the bits it
 * returned before.  B = 0: FS_OK, nothing written.  FS_EINVAL: not a SURF
 * plan, or a NULL buffer.  FS_ENOTSUP: reference-order accumulation; a plan
 * that does not own every focal row [0, n) or has world > 1; on the GPU for
 * SURF*: n > 24576 or a label code outside [0, 8).  FS_EOOM: the weight buffer
 * does not fit.  CPU backend: row b is bit for bit what fs_plan_score of a
 * plan created with labelling b returns (any number of classes, any n).  GPU
 * backend: float32 MFMA partials of at most 256 pairs folded into float64,
 * the column terms in float64 in the order of the sort; no float atomics (the
 * same call gives the same bits twice).
 *
 * fs_surf_score_labels (SURF.py:139-218): one call from host arrays (float64
 * X, every column scored, labelling 0 as the plan's y); scores_out[b * p + f]
 * divided by n.  B >= 1.  FS_ENOTSUP in reference order and, on the GPU, when
 * the distance rows do not fit one plan (fs_surf_score would score in row
 * panels).
 *
 * fs_plan_surf_labels_info (SURF.py:139-218): out[0..4) of the last completed
 * call: the weighted pairs listed (pairs with a near side), the near sides
 * sum_i |N_i|, the chunks of labellings walked (CPU: the labellings), 1 if
 * the star walk ran.  FS_EINVAL before the first call.
 *
 * fs_plan_surf_labels_kernel_ms (SURF.py:139-218): summed HIP-event time in
 * milliseconds of the last call (GPU only; -1 when unavailable).  which: 0 =
 * distances + resolve + records (once per call), 1 = the weights kernels, 2 =
 * the score kernel (both summed over the chunks), 3 = the column sort and the
 * star walk (-1 when the star walk did not run). */
FS_API int fs_plan_surf_score_labels(fs_plan* plan, const int32_t* labels, int64_t B,
                                     double* scores);
FS_API int fs_surf_score_labels(int backend, int device, const double* x, int64_t n, int64_t p,
                                const int32_t* labels, int64_t B, const float* recip,
                                const uint8_t* is_discrete, int use_star, int n_jobs,
                                float* scores_out);
FS_API int fs_plan_surf_labels_info(const fs_plan* plan, int64_t out[4]);
FS_API double fs_plan_surf_labels_kernel_ms(const fs_plan* plan, int which);
/* RReliefF: Relief for continuous targets (definitions: csrc/fs_rrelieff.h).
 * The neighbours of a focal sample are its k nearest other samples -- the
 * lists of a ReliefF plan with ONE class (fs_plan_create_relieff with
 * n_classes = 1, y_enc all 0, class_probs = {1}) -- and do not read the
 * target, so the distance pass and the selection run once per call for any
 * number of targets.
 *
 * fs_plan_score_targets: for the B targets targets[b * n + i] (host memory,
 * float64, finite) the raw sums over the (focal row, neighbour) pairs of the
 * plan's focal rows and current feature subset: s_a[n_kept] = sum of diff,
 * s_ca[b * n_kept + f] = sum of dy_b * diff, s_c[b] = sum of dy_b, with
 * dy_b(i, j) = |t_i - t_j| / (max t - min t) of target b (0 for a constant
 * target).  Outputs in the memory space fs_plan_score writes to.  The sums add
 * up over disjoint focal-row ranges; the number of pairs is rows * k.  Row b
 * of any call has the bits of the B = 1 call of target b, s_a the same bits
 * for any B, and a repeated call gives the same bits (no float atomics).
 * FS_EINVAL, with nothing written: a NULL pointer, B < 1, a non-finite target,
 * a plan with more than one class, a SURF or MultiSURF plan, a plan in
 * reference-order accumulation, k < 1 or k > n - 1.  An empty row range gives
 * zeros.
 *
 * fs_rrelieff_scores: the epilogue on the host, for one target:
 * scores[f] = s_ca[f] / s_c - (s_a[f] - s_ca[f]) / (n_pairs - s_c) in float64,
 * rounded to float32; all 0 when s_c == 0 or s_c == n_pairs.
 *
 * fs_rrelieff_score: one call from host arrays (every column scored, fast
 * accumulation); scores_out[b * p + f].
 *
 * fs_plan_targets_kernel_ms: HIP-event time in milliseconds of the last
 * completed fs_plan_score_targets (GPU only; -1 when unavailable).  which:
 * 0 = the neighbour selection, 1 = the update kernel, summed over the chunks
 * of targets. */
FS_API int fs_plan_score_targets(fs_plan* plan, const double* targets, int64_t B, double* s_a,
                                 double* s_ca, double* s_c);
FS_API int fs_rrelieff_scores(const double* s_a, const double* s_ca_row, double s_c,
                              double n_pairs, int64_t n_kept, float* scores);
FS_API int fs_rrelieff_score(int backend, int device, const float* x, int64_t n, int64_t p,
                             const double* targets, int64_t B, const float* recip,
                             const uint8_t* is_discrete, int64_t k, int n_jobs,
                             float* scores_out);
FS_API double fs_plan_targets_kernel_ms(const fs_plan* plan, int which);
/* After the three stages of a MultiSURF step, with rowstats[3n], counts[2n]
 * and scores[n_kept] all-reduced (identical on every rank): the 16-bit
 * decision check of fs_multisurf_score (see fs_multisurf_last_guard) for
 * plans whose pass 1 runs on 16-bit operands.  risk_out = the estimated score
 * error of threshold-moved decisions over max |score| (-1: nothing to check:
 * 32-bit operands, MultiSURF*, the CPU backend).  Above the bound the plan
 * switches to 32-bit operands for good and *switched_out = 1: every rank
 * computed the same risk and switched alike, and the caller runs the step
 * again (the reference's single threshold rule, MultiSURF.py:193-217, and
 * TuRF's refits, TuRF.py:87,111, through the same plan). */
FS_API int fs_plan_decision_guard(fs_plan* plan, const double* rowstats, const double* counts,
                                  const double* scores, double* risk_out, int* switched_out);
/* Reference-order accumulation (fs_set_accumulation(FS_ACCUM_REFERENCE))
 * over world > 1 ranks, GPU backend.  The reference's float32 sums run over
 * every focal sample in order (MultiSURF.py:231-253, then
 * np.sum(temp, axis=0)), so pass 2 is not a sum of rank partials; after
 * pass1 / all-reduce / select / all-reduce, instead of fs_plan_pass2:
 *   1. fs_plan_ref_masks: this rank's pair-tile decisions as bit masks in
 *      masks[words] (device memory, words >= fs_plan_ref_mask_words; zeroed
 *      first, so every word outside this rank's tiles is 0);
 *   2. a SUM all-reduce of the masks as int64 (each word is nonzero on at
 *      most one rank, so the sum is the whole triangle's masks);
 *   3. fs_plan_ref_pass2 on every rank at once: the per-sample hit / miss
 *      chains of the focal rows [row_begin, row_end) of the rank's contiguous
 *      block (counts = the all-reduced counts[2n]) into the plan's float32
 *      temp rows;
 *   4. fs_plan_ref_sums on the ranks in order: rank r continues the float32
 *      column sums init[n_kept] it received from rank r - 1 (NULL on the
 *      first rank) over its temp rows and hands sums[n_kept] to rank r + 1;
 *      the last rank's sums, divided by n, are the reference's scores bit
 *      for bit (fastselect_amd/parallel.py ShardedMultiSURF). */
FS_API int fs_plan_ref_mask_words(fs_plan* plan, int64_t* words);
FS_API int fs_plan_ref_masks(fs_plan* plan, uint64_t* masks, int64_t words);
FS_API int fs_plan_ref_pass2(fs_plan* plan, const uint64_t* masks, const double* counts,
                             int64_t row_begin, int64_t row_end);
FS_API int fs_plan_ref_sums(fs_plan* plan, const double* init, double* sums);
/* The same rank chain for row-sharded ReliefF and SURF (fs_plan_create_relieff
 * / fs_plan_create_surf over the rank's focal rows, reference order, GPU
 * backend): fs_plan_ref_temp runs fs_plan_score up to the plan's float32 temp
 * rows (ReliefF.py:208-218, SURF.py:191-193) on every rank at once, then
 * fs_plan_ref_sums continues the previous rank's column sums over them
 * (ReliefF.py:219-220, SURF.py:195: one sequential float32 sum). */
FS_API int fs_plan_ref_temp(fs_plan* plan);
/* Restrict the next pass2 of a MultiSURF plan to the focal samples
 * [row_begin, row_end) (as fs_multisurf_score_rows; a new plan scores
 * [0, n)).  pass1 / select are unchanged: thresholds and counts are global. */
FS_API int fs_plan_set_rows(fs_plan* plan, int64_t row_begin, int64_t row_end);
/* Re-target a MultiSURF plan to the pair tiles of shard (rank, world) --
 * tile t belongs to rank t % world -- keeping X and its quantised operands
 * resident (the GPU plan frees the previous shard's distance tiles).  With
 * it one device scores a job whose distance tiles exceed its memory in
 * shards; the stages then run in three rounds, each over all shards (row
 * moments -> all-reduce; select -> counts -> all-reduce; select, pass2 ->
 * scores), every round recomputing the shard's distances
 * (fastselect_amd/parallel.py ShardedMultiSURF).  An N-GPU job with V
 * shards per GPU uses rank + N * v of N * V.  No reference counterpart (the
 * reference streams each focal sample's distance row, MultiSURF.py:174-214). */
FS_API int fs_plan_set_shard(fs_plan* plan, int rank, int world);
/* The star form of a plan.  A GPU MultiSURF* plan scores its far pairs in one
 * of two ways: dense (pass 2 weighs every pair of the tiles it owns) or split
 * (pass 2 weighs the near pairs, and the far part of EVERY pair comes from
 * per-column terms, of which a rank adds its share of the columns).  The two
 * are the same sum only when all plans that share a MultiSURF* job -- the
 * ranks and shards whose partial vectors are added -- are in one form: a
 * mixed job counts some far pairs twice and misses some columns' far terms,
 * silently.  A plan picks its form at creation from its device's free memory
 * of that moment, so the plans of a job may differ.  Ask each plan with
 * fs_plan_star_split (1 = split, 0 = dense, and 0 for every plan that never
 * splits: no star, reference-order accumulation, ReliefF, the CPU backend),
 * take the minimum over the job, and give it to every plan with
 * fs_plan_set_star_split before the first fs_plan_pass1 (the GPU plan lays
 * out its buffers again; X stays resident; a later pass1 / select / pass2
 * sequence starts over).  FS_EINVAL when the split is asked of a plan that
 * cannot take it (more than 24576 samples or 8 classes, no star, reference
 * order, the CPU backend), or either change of a SURF* plan: row plans score
 * their own focal rows completely in either form and need no agreement.  The
 * one-shot calls agree by themselves (fs_multisurf_score_devices decides once
 * for all its devices); fs_multisurf_last_star_split tells the form of this
 * thread's last GPU fs_multisurf_score[_rows|_devices] call (-1: none yet). */
FS_API int fs_plan_star_split(const fs_plan* plan, int* split_out);
FS_API int fs_plan_set_star_split(fs_plan* plan, int split);
FS_API int fs_multisurf_last_star_split(int* split_out);
/* Shards per device that keep a MultiSURF job of n samples, p features and
 * `world` ranks within the device's free memory (1 when it fits, or without
 * a GPU; the shards test hook overrides).  The one-shot fs_multisurf_score[_rows]
 * shards by itself. */
FS_API int fs_multisurf_shards(int device, int64_t n, int64_t p, int world, int* shards);
/*
 * ReliefF / SURF plans (resident scoring): X uploaded once (GPU) or copied
 * (CPU), arguments as fs_relieff_score / fs_surf_score, focal samples
 * [row_begin, row_end) as fs_*_score_rows.  fs_plan_score writes the float64
 * score sums of those samples for the plan's current feature subset to
 * sums[n_kept] (device memory for the GPU backend, host memory for the CPU
 * backend); fs_plan_set_features re-targets the plan to another column subset
 * without re-uploading X, which is how TuRF re-scores its shrinking feature
 * sets (TuRF.py:93-115).  pass1 / select / pass2 are MultiSURF-only, and
 * fs_plan_score is ReliefF / SURF-only (FS_EINVAL otherwise).
 */
FS_API int fs_plan_create_relieff(fs_plan** plan_out, int backend, int device, const float* x,
                                  int64_t n, int64_t p, const int32_t* y_enc, const float* recip,
                                  const uint8_t* is_discrete, int64_t k, const float* class_probs,
                                  int64_t n_classes, int64_t row_begin, int64_t row_end,
                                  int n_jobs, uint64_t stream);
FS_API int fs_plan_create_surf(fs_plan** plan_out, int backend, int device, const double* x,
                               int64_t n, int64_t p, const int32_t* y, const float* recip,
                               int use_star, const uint8_t* is_discrete, int64_t row_begin,
                               int64_t row_end, int n_jobs, uint64_t stream);
FS_API int fs_plan_score(fs_plan* plan, double* sums);
/* STIR for ReliefF (definitions: fastselect_amd/csrc/fs_stir.h, "STIR for
 * ReliefF"): fs_plan_score on a ReliefF plan, and in the same call the four
 * STIR sums over the very neighbour lists that score weighs.  H is the set of
 * ordered pairs (i, j) with j one of focal sample i's nearest hits, M the
 * same over its nearest misses of every other class, pooled and unweighted
 * (the class priors of the score do not enter; the published STIR for two
 * classes, this project's generalisation for more).  The reference's
 * self-hit (a focal sample counted as its own zero-diff hit when its class
 * has fewer than k other members) is not a pair.
 *   sums[n_kept]         what fs_plan_score writes, the same bits;
 *   stir_sums[4 n_kept]  stir_sums[q * n_kept + k], q = 0..3 for S1H, S2H,
 *                        S1M, S2M, k in feat_idx order (as fs_plan_stir);
 *   pair_counts[2]       |H| and |M| as doubles (exact integers).
 * All three lie in the memory space fs_plan_score uses for sums (device
 * memory for the GPU backend, host memory for the CPU backend) and cover the
 * plan's focal rows [row_begin, row_end) and current feature subset; the
 * sums and counts of disjoint row ranges add up to the whole (a pair belongs
 * to its focal sample).  An empty row range gives zeros.  fs_stir_statistics
 * turns the summed sums and counts into t-statistics.  Both accumulation
 * modes (the neighbour sets are the same); a later fs_plan_score is
 * unchanged.  SURF plans: FS_ENOTSUP; MultiSURF plans: FS_EINVAL (their STIR
 * is fs_plan_stir). */
FS_API int fs_plan_score_stir(fs_plan* plan, double* sums, double* stir_sums,
                              double* pair_counts);
/* Number of pair tiles this plan owns, the pair-feature evaluations one full
 * pass1+pass2 performs on this rank (throughput accounting) and the number of
 * ambiguous pairs the last stage 2 recomputed exactly.  NULL outputs are
 * skipped. */
FS_API int fs_plan_info(const fs_plan* plan, int64_t* owned_tiles, double* pair_feature_evals,
                        int64_t* refined_pairs);
/* Refinement-band calibration of the plan's current feature layout (GPU
 * MultiSURF / ReliefF plans; no reference counterpart -- it guards the
 * integer pass 1 that replaces the reference's float distance loop,
 * MultiSURF.py:176-188).  fs_plan_calibration writes out[6] (its size since
 * the first release): [0] 1 if pass 1 runs on 16-bit operands, [1] / [2] rms
 * / max |quantised - reference| distance error over 4096 sampled pairs
 * (integer units), [3] the independent-rounding model's standard deviation
 * sqrt(pc/6 + 1), [4] band / model band, [5] 1 if the coherence guard turned
 * 16-bit operands off, 2 if the per-row guard did (a row whose mean pass-1
 * error, measured by the mean correction, exceeds 12 standard deviations of
 * independent rounding); SURF plans (32-bit operands against its float64
 * terms, fs_surfint.hip): [5] 0 on integer distances, 3 on float64 ones (the
 * band above one float32 ulp of the shorter sampled distances, a small
 * problem, or the surf_f64 test hook).  fs_plan_calibration_ex writes min(n_out, 8)
 * values -- the six above, then [6] that row guard's largest row bias over
 * its limit (0 when it did not run) and [7] SC, the integer units per
 * scaled-diff unit of pass 1 (the row statistics of fs_plan_pass1 are in
 * these units: mu_i = (rowstats[3i] - rowstats[3i+2]) / (n - 1) / SC) -- and
 * returns how many it wrote (or a negative FS_E* code).  CPU plans:
 * {0, 0, 0, model sigma, 1, 0, 0, SC}. */
FS_API int fs_plan_calibration(const fs_plan* plan, double* out);
FS_API int fs_plan_calibration_ex(const fs_plan* plan, double* out, int n_out);
/* Owned pairs that carried a non-zero pass-2 weight in the last pass 2 (the
 * pairs the sparse GPU pass 2 evaluates; -1 when the plan does not count
 * them: CPU backend, dense pass 2, or before the first pass 2). */
FS_API int fs_plan_weighted_pairs(const fs_plan* plan, int64_t* pairs);
/* Average duration in milliseconds of the last pass1 / pass2 distance and
 * score kernels, measured with HIP events on the plan's stream (GPU only;
 * -1 when unavailable).  which: 0 = distance kernel, 1 = score kernel (for
 * ReliefF plans: neighbour selection, exact refinement and update), 2 =
 * ReliefF's first k_rf_select launch. */
FS_API double fs_plan_kernel_ms(const fs_plan* plan, int which);
FS_API int fs_plan_destroy(fs_plan* plan);

/* ---- MDR: exhaustive k-way SNP interaction search ----------------------- */

/*
 * Balanced accuracy of every k-combination of the p genotype columns, for all
 * cross-validation folds in one pass.  Replaces mdr_kernel (MDR.py:20-79) and
 * _batch_balanced_accuracy_cpu (MDR.py:82-129), which the reference's fit
 * calls once per fold on a host-built list of combinations (MDR.py:246-283).
 *   x          [n][p] row-major genotypes in {0,1,2} (the uint8 X of MDR.py:220)
 *   is_case    [n] nonzero marks a case (y == 1, MDR.py:47, 102)
 *   fold       [n] in [0, n_folds): the fold whose TEST set holds sample i;
 *              fold f trains on every sample with fold[i] != f.  fold == NULL
 *              and n_folds == 0: one scan that trains on all samples (outputs
 *              have length 1)
 *   n_jobs     CPU threads (-1 = all); ignored by the GPU backend
 *   best_ba    [max(n_folds,1)] the largest float32 BA of each fold
 *   best_rank  [max(n_folds,1)] the smallest combination rank
 *              (itertools.combinations order) that attains it, i.e.
 *              np.argmax of the fold's BAs (MDR.py:282)
 *   ba_out     NULL, or [max(n_folds,1)][C(p,k)] float32, fold-major (sized by
 *              the caller; for tests and small jobs)
 * Cell counts are popcounts of ANDed genotype bit-planes; a cell is high risk
 * iff control == 0 or case * total_control > control * total_case, which
 * equals the reference's float64 comparison for n < 2^25; BA = (tp /
 * total_case + tn / total_control) / 2.0 in IEEE float64, rounded to float32.
 * Both backends give the same bits.  FS_EINVAL: k outside 1..6, k > p, n < 1
 * or n >= 2^25, a genotype above 2, a fold id out of range, C(p,k) > 2^62,
 * NULL pointers.
 */
FS_API int fs_mdr_scan(int backend, int device, const uint8_t* x, int64_t n, int64_t p,
                       const uint8_t* is_case, int k, const int32_t* fold, int n_folds,
                       int n_jobs, float* best_ba, int64_t* best_rank, float* ba_out);
/*
 * fs_mdr_scan for n_labelings phenotype vectors of one genotype matrix in one
 * pass: the permutation test of an MDR search, or several binary traits.
 *   labels     [n_labelings][n] row-major, nonzero marks a case; the rows are
 *              arbitrary (they need not be permutations of each other)
 *   fold       as in fs_mdr_scan, shared by all labellings
 *   best_ba    [n_labelings][F], F = max(n_folds, 1)
 *   best_rank  [n_labelings][F]
 *   ba_out     NULL, or [n_labelings][F][C(p,k)] float32
 * Row b of every output holds exactly what fs_mdr_scan(x, labels[b], k, fold,
 * n_folds) returns, bit for bit, on both backends: the genotype planes are
 * ANDed once per combination and each labelling adds one AND and one popcount
 * per word.  FS_EINVAL: as fs_mdr_scan, and n_labelings outside 1..65535.
 */
FS_API int fs_mdr_scan_labels(int backend, int device, const uint8_t* x, int64_t n, int64_t p,
                              const uint8_t* labels, int n_labelings, int k,
                              const int32_t* fold, int n_folds, int n_jobs, float* best_ba,
                              int64_t* best_rank, float* ba_out);
/* Milliseconds the calling thread's last GPU fs_mdr_scan_labels spent on
 * upload, pack, scan (with the device reduction) and download (HIP events; -1
 * where unavailable), for the benchmark tool. */
FS_API int fs_mdr_labels_last_timing(double* ms4);
/*
 * The n_top best combinations of every fold instead of the one best: the
 * ranked list ("model landscape") of an MDR search, without the F x C(p,k)
 * array of ba_out.  Arguments and checks as fs_mdr_scan, and
 *   n_top      1..4096 (kMdrMaxTop, the size the backends' buffers are laid
 *              out for)
 *   top_ba     [F][n_top] float32, F = max(n_folds, 1)
 *   top_rank   [F][n_top]
 * Row f holds the first min(n_top, C(p,k)) combinations of fold f ordered by
 * (float32 BA descending, rank ascending), i.e. np.argsort(-ba_out[f],
 * kind="stable")[:n_top] and the BAs there; entries past C(p,k) are rank -1,
 * BA 0.  Entry 0 of a row is what fs_mdr_scan returns for that fold.  Both
 * backends give the same bits, whatever the thread count or launch schedule.
 * The GPU backend scans twice (a histogram of the BAs' leading bits, then the
 * combinations at or above the bin that holds the n_top-th); its device
 * memory does not grow with C(p,k).  FS_EINVAL: as fs_mdr_scan, n_top out of
 * range, NULL outputs.
 */
FS_API int fs_mdr_scan_top(int backend, int device, const uint8_t* x, int64_t n, int64_t p,
                           const uint8_t* is_case, int k, const int32_t* fold, int n_folds,
                           int n_top, int n_jobs, float* top_ba, int64_t* top_rank);
/* As fs_mdr_labels_last_timing for the last GPU fs_mdr_scan_top: upload, pack,
 * scan (both scans, the threshold search and the selection), download. */
FS_API int fs_mdr_top_last_timing(double* ms4);
/* C(p,k), the length of np.array(list(combinations(range(p), k))) that the
 * reference builds on the host (MDR.py:247-251); FS_EINVAL if above 2^62. */
FS_API int fs_mdr_combinations(int64_t p, int k, int64_t* count);
/* rank -> the k ascending column indices of that combination, i.e.
 * all_combos[rank] of the reference (MDR.py:283), without the list. */
FS_API int fs_mdr_unrank(int64_t p, int k, int64_t rank, int32_t* features);

/* ---- mRMR: pairwise discrete mutual information -------------------------- */

/*
 * Relevance I(X_f; y) of every column and the p x p matrix of pairwise mutual
 * information I(X_i; X_j) of integer-coded data.  Replaces _mi_pair_cpu and
 * _batch_mi_cpu (mutual_information.py:25-63), _mi_pair_gpu_kernel
 * (mutual_information.py:70-115) and the backend dispatch of
 * calculate_mi_matrices (mutual_information.py:158-196), whose GPU path
 * leaves the matrix to the CPU.
 *   codes       [n][p] row-major state codes, 0..n_states-1
 *   ycodes      [n] codes of the target, same range
 *   unit        0 = bits, 1 = nats
 *   n_jobs      CPU threads (-1 = all); ignored by the GPU backend
 *   relevance   [p]
 *   redundancy  [p][p] symmetric, zero diagonal; NULL: relevance only
 *   counts_out  NULL, or [p][p][n_states][n_states] int32: for i < j the
 *               contingency table of the pair (row = state of column i), else
 *               zeros (sized by the caller; for tests and small jobs)
 * A table cell is a popcount of two ANDed state bit-planes (exact integers,
 * equal in both backends); the float64 expressions of _mi_pair_cpu follow in
 * their written order (mutual_information.py:31-46), a pair once for i < j with
 * the rows taken from column i, then mirrored.  The backends differ only
 * through the host's and the device's log().  FS_EINVAL: n < 1 or n >= 2^31,
 * p < 1, n_states outside 1..256, a code >= n_states, unit outside 0..1, more
 * than 32 states on the GPU backend (the reference's _MAX_STATES_GPU), NULL
 * codes / ycodes / relevance.  FS_EOOM when the matrices do not fit.
 */
FS_API int fs_mi_matrices(int backend, int device, const uint8_t* codes, const uint8_t* ycodes,
                          int64_t n, int64_t p, int n_states, int unit, int n_jobs,
                          double* relevance, double* redundancy, int32_t* counts_out);
/* Milliseconds the calling thread's last GPU fs_mi_matrices spent on upload,
 * pack, scan and download (HIP events; -1 where unavailable), for the
 * benchmark tool. */
FS_API int fs_mi_last_timing(double* ms4);

/* ---- CFS: correlation-based feature selection ----------------------------- */

/*
 * Symmetrical uncertainty SU(x, y) = 2 I(x; y) / (H(x) + H(y)) of integer-coded
 * columns, float64 in the written order of _entropy, _mutual_information and
 * _symmetrical_uncertainty (CFS.py:26-77, compiled numba's typing), stored as
 * float32; the column with the lower index supplies a pair's table rows
 * (CFS.py:96-102), the target counts as column p.  The handle keeps the packed
 * state bit-planes and computes a row SU(f, .) when the search selects f: the
 * p x p matrix of _precompute_correlations_{cpu, gpu_kernel} (CFS.py:80-104,
 * 219-243) never exists.  The backends differ only through the host's and the
 * device's log2().
 */
typedef struct fs_cfs fs_cfs;
/*
 * Uploads and packs the codes once and computes r_cf (replaces the r_cf half
 * of _precompute_correlations_cpu, CFS.py:88-92).
 *   codes    [n][p] row-major state codes, 0..n_states-1
 *   ycodes   [n] codes of the target, same range
 *   n_jobs   CPU threads (-1 = all); ignored by the GPU backend
 * FS_EINVAL: NULL out / codes / ycodes, n < 1 or n >= 2^31, p < 1, n_states
 * outside 1..256, a code >= n_states, more than 32 states on the GPU backend
 * (CFS.py:349).  FS_EOOM when the planes do not fit (decided before any array
 * is read).
 */
FS_API int fs_cfs_create(fs_cfs** out, int backend, int device, const uint8_t* codes,
                         const uint8_t* ycodes, int64_t n, int64_t p, int n_states, int n_jobs);
/* r_cf[p]: SU(X_f, y), the feature supplying the rows (CFS.py:88-92). */
FS_API int fs_cfs_relevance(fs_cfs* h, float* r_cf);
/*
 * _best_first_search (CFS.py:115-162) on lazy rows: starts at argmax(r_cf)
 * (empty when that is < min_r_cf), scans the unselected features with
 * r_cf >= min_r_cf, sums in float64 in the reference's order, takes the
 * lowest-index candidate of the highest merit while the merit grows.
 *   selected    [p] capacity, in selection order
 *   n_selected  the number selected
 *   merits      [p] capacity: merits[s] = the merit after s + 1 features
 */
FS_API int fs_cfs_search(fs_cfs* h, double min_r_cf, int64_t* selected, int64_t* n_selected,
                         double* merits);
/*
 * row[p] = SU(feature, .), the diagonal 0: one row of the reference's
 * r_ff_matrix (CFS.py:94-102), from the handle's row cache if the last search
 * selected the feature, else computed on the spot (same bits either way).
 */
FS_API int fs_cfs_row(fs_cfs* h, int64_t feature, float* row);
/*
 * _best_first_search (CFS.py:115-162) on a caller's r_cf[p] and symmetric
 * r_ff[p][p] through the same step code as fs_cfs_search (r_ff[i, s] is read
 * as row s, column i).
 */
FS_API int fs_cfs_search_matrix(int backend, int device, const float* r_cf, const float* r_ff,
                                int64_t p, double min_r_cf, int64_t* selected,
                                int64_t* n_selected, double* merits);
/* Milliseconds the calling thread's last GPU handle spent on upload, pack,
 * relevance, rows and steps (HIP events; the last two grow with every
 * fs_cfs_search / fs_cfs_row; -1 where unavailable), for the benchmark tool. */
FS_API int fs_cfs_last_timing(double* ms5);
/* Frees the handle (NULL: nothing). */
FS_API int fs_cfs_destroy(fs_cfs* h);

/* ---- mRMR: selection without the redundancy matrix ------------------------ */

/*
 * The greedy selection of mRMR.fit (mRMR.py:96-117) on rows of mutual
 * information computed when their feature is selected: the relevance
 * I(X_f; y), then per step the scores (MID: rel - rsum / i, MIQ: rel /
 * (rsum / i + 1e-9), mRMR.py:104-107), the candidates within
 * np.isclose(scores, max, atol=1e-12) (mRMR.py:109) resolved by the lowest
 * mean redundancy and then the lowest index (mRMR.py:110-114), and
 * rsum += I(.; X_best) (mRMR.py:117).  k p pairs instead of the p^2 / 2 of
 * calculate_mi_matrices (mRMR.py:94-96); nothing of size p x p is allocated.
 * Every value is the entry fs_mi_matrices computes on the same backend, bit
 * for bit.  The GPU backend queues all k steps on one stream and synchronises
 * once.
 *   method      0 = MID, 1 = MIQ
 *   relevance   [p]
 *   selected    [k] in selection order
 *   rows        NULL, or [k][p] float64 with rows[s][c] = I(X_c; X_selected[s]),
 *               0.0 at c == selected[s]
 *   n_jobs      CPU threads (-1 = all); ignored by the GPU backend
 * codes, ycodes, n, p, n_states, unit: as fs_mi_matrices.  FS_EINVAL: as
 * fs_mi_matrices, and k outside 1..p, method outside 0..1, NULL selected.
 * FS_EOOM when the planes and rows do not fit (decided before any array is
 * read).
 */
FS_API int fs_mrmr_select(int backend, int device, const uint8_t* codes, const uint8_t* ycodes,
                          int64_t n, int64_t p, int n_states, int unit, int method, int64_t k,
                          int n_jobs, double* relevance, int64_t* selected, double* rows);
/*
 * The same step code (mRMR.py:96-117) on a caller's relevance[p] and symmetric
 * redundancy[p][p] (the picked feature's row is read): for tests that pin the
 * tie rules, and for callers who hold a matrix already.
 */
FS_API int fs_mrmr_search_matrix(int backend, int device, const double* relevance,
                                 const double* redundancy, int64_t p, int method, int64_t k,
                                 int64_t* selected);
/* Milliseconds the calling thread's last GPU fs_mrmr_select spent on upload,
 * pack, relevance (with the first pick), rows and steps (HIP events; -1 where
 * unavailable: above 64 steps the loop is timed as a whole, in `rows`), for
 * the benchmark tool. */
FS_API int fs_mrmr_last_timing(double* ms5);

/* ---- JMI and CMIM: selection on rows of joint relevance ------------------- */

/*
 * Greedy selection by the joint relevance J(f, s) = I(X_f, X_s; y) of a
 * candidate with every selected feature, which sees a feature that matters
 * only together with another one.  For columns lo < hi the table
 * T[(a * kcol[hi] + b)][c] counts the samples with x_lo = a, x_hi = b, y = c;
 * J is the mutual information of its rows (the joint state) and columns (y) by
 * the float64 expressions of fs_mi_matrices in their order, so J(lo, hi)
 * equals, bit for bit on the same backend, the relevance fs_mi_matrices gives
 * the column x_lo * K + x_hi (K >= kcol[hi]).  J(f, f) = 0.0.
 * Step 0 picks argmax relevance; after picking s the row J(., s) enters
 *   JMI  (method 0, Yang & Moody):  acc[f] += J(f, s), from +0.0;
 *   CMIM (method 1, Fleuret):       acc[f] = min(acc[f], J(f, s) - relevance[s]),
 *                                   from +inf (I(X_f; y | X_s));
 * step i >= 1 picks the unselected feature with the largest acc.  Among exact
 * equals the lowest index wins; there is no closeness rule.  k p joint tables
 * in all; nothing of size p x p is allocated.  The GPU backend queues all k
 * steps on one stream and synchronises once.
 *   relevance   [p]: I(X_f; y), the bits of fs_mi_matrices / fs_mrmr_select
 *   selected    [k] in selection order
 *   rows        NULL, or [k][p] float64 with rows[s][c] = J(c, selected[s]),
 *               0.0 at c == selected[s]
 *   n_jobs      CPU threads (-1 = all); ignored by the GPU backend
 * codes, ycodes, n, p, n_states, unit: as fs_mi_matrices.  FS_EINVAL: as
 * fs_mi_matrices, and k outside 1..p, method outside 0..1, NULL relevance /
 * selected; on the CPU backend a joint table of more than 2^20 cells
 * (max kcol^2 * kcol[y]); on the GPU backend more than 32 states or more than
 * 4 classes of y.  FS_EOOM when the planes and rows do not fit (decided before
 * any array is read).
 */
FS_API int fs_jmi_select(int backend, int device, const uint8_t* codes, const uint8_t* ycodes,
                         int64_t n, int64_t p, int n_states, int unit, int method, int64_t k,
                         int n_jobs, double* relevance, int64_t* selected, double* rows);
/*
 * The joint relevance of caller-chosen anchors through the same row code:
 * rows[t][c] = J(c, anchors[t]), 0.0 at c == anchors[t].
 *   anchors  [m] columns in 0..p-1, m >= 1
 *   rows     [m][p] float64
 * FS_EINVAL as fs_jmi_select, and an anchor outside 0..p-1, m < 1, NULL
 * anchors / rows.
 */
FS_API int fs_jmi_rows(int backend, int device, const uint8_t* codes, const uint8_t* ycodes,
                       int64_t n, int64_t p, int n_states, int unit, const int64_t* anchors,
                       int64_t m, int n_jobs, double* rows);
/*
 * The same step code on a caller's relevance[p] and symmetric joint[p][p] (the
 * picked feature's row is read): for tests that pin the tie and minimum rules,
 * and for callers who hold a matrix already.
 */
FS_API int fs_jmi_search_matrix(int backend, int device, const double* relevance,
                                const double* joint, int64_t p, int method, int64_t k,
                                int64_t* selected);
/* Milliseconds the calling thread's last GPU fs_jmi_select spent on upload,
 * pack, relevance (with the first pick), rows and steps (HIP events; -1 where
 * unavailable: above 64 steps the loop is timed as a whole, in `rows`), for
 * the benchmark tool. */
FS_API int fs_jmi_last_timing(double* ms5);

/* ---- Pair screen: the n_top best of all pairs by joint relevance ---------- */

/*
 * An exhaustive scan of the joint relevance J(i, j) = I(X_i, X_j; y) of
 * fs_jmi_select over all C(p,2) pairs i < j, returned as a ranked list, not a
 * matrix: it finds a pair that acts purely together (y = x_a XOR x_b), which
 * no marginal or greedy selector reaches.  J(i, j) has, on the same backend,
 * the bits fs_jmi_rows gives for (c = j, anchor = i).  The score of a pair is
 *   score_kind 0 ("joint"):  J(i, j);
 *   score_kind 1 ("gain"):   (J(i, j) - relevance[i]) - relevance[j] in float64
 *                            in that order (the interaction information:
 *                            positive for synergy, negative for redundancy).
 * The list is ordered by (score descending, rank ascending), the rank of a
 * pair being its place in itertools.combinations(range(p), 2),
 * i * (2p - i - 1) / 2 + (j - i - 1); there is no closeness rule, and -0.0
 * counts (and is returned) as +0.0.
 *   relevance     [p]: I(X_f; y), the bits of fs_mi_matrices / fs_jmi_select
 *   top_score     [n_top], top_i, top_j [n_top]: the first min(n_top, C(p,2))
 *                 pairs in that order; the entries past C(p,2) are score 0.0,
 *                 i = j = -1 (as fs_mdr_scan_top)
 *   feature_best  NULL, or [p]: the largest score of any pair that contains f
 *   n_top         1..65536
 *   n_jobs        CPU threads (-1 = all); ignored by the GPU backend
 * The result is identical for every thread count, launch split and buffer
 * size.  codes, ycodes, n, p, n_states, unit: as fs_jmi_select.  FS_EINVAL:
 * as fs_jmi_select, and p < 2, n_top outside 1..65536, score_kind outside
 * 0..1, NULL relevance / top_score / top_i / top_j; on the CPU backend a joint
 * table of more than 2^20 cells; on the GPU backend more than 32 states or
 * more than 4 classes of y (a one-class y gives all-zero scores without a
 * scan).  Device memory is the bit-planes plus O(p + n_top): nothing of size
 * p x p.  FS_EOOM when the planes do not fit (decided before any array is
 * read).
 */
FS_API int fs_pair_screen(int backend, int device, const uint8_t* codes, const uint8_t* ycodes,
                          int64_t n, int64_t p, int n_states, int unit, int score_kind,
                          int64_t n_top, int n_jobs, double* relevance, double* top_score,
                          int64_t* top_i, int64_t* top_j, double* feature_best);
/* Milliseconds the calling thread's last GPU fs_pair_screen spent on upload,
 * pack, relevance, the scan with the selection (its launches and the host
 * merges between them) and download (HIP events; -1 where unavailable), for
 * the benchmark tool. */
FS_API int fs_pair_screen_last_timing(double* ms5);

/*
 * The pair screen under many labellings of y in one pass: the null of a
 * permutation test, or several traits at once.  A pair's joint cells do not
 * depend on y, so the columns are packed and combined once for all rows.
 *   labels      [n_labelings][n] row-major codes in 0..n_states-1; the rows are
 *               arbitrary (they need not be permutations of each other)
 *   best_score, best_i, best_j  [n_labelings]
 *   relevance   NULL, or [n_labelings][p]
 * Row b of best_* is top_score[0], top_i[0], top_j[0] of
 * fs_pair_screen(codes, labels[b], ..., n_top = 1) on the same backend, bit for
 * bit: the best pair by (score descending, rank ascending), -0.0 returned as
 * +0.0; row b of relevance is that call's relevance.  Neither depends on
 * n_jobs, the launch split or how the labellings are chunked.  A one-class row
 * gives (0.0, 0, 1) and zero relevance, as fs_pair_screen does.
 * Classes: the class count of the batch is the largest code over all rows plus
 * one.  A class that a row does not take adds exact zeros to that row's sums
 * (its cells' pxy are 0.0, its marginal is 0.0 and is not counted as used, its
 * terms are 0.0), so the common count changes no bits against the row's own.
 * FS_EINVAL: as fs_pair_screen (without n_top), and n_labelings outside
 * 1..65535, NULL labels / best_score / best_i / best_j, a label code >=
 * n_states; on the GPU backend more than 32 states or more than 4 classes over
 * all rows.  FS_EOOM is decided from the sizes before any array is read.
 * On the GPU up to 4 states take a kernel with one lane per labelling; 5..32
 * states run fs_pair_screen's kernels once per labelling on columns packed
 * once (correct, and no faster than that many calls by much).
 */
FS_API int fs_pair_screen_labels(int backend, int device, const uint8_t* codes,
                                 const uint8_t* labels, int n_labelings, int64_t n, int64_t p,
                                 int n_states, int unit, int score_kind, int n_jobs,
                                 double* best_score, int64_t* best_i, int64_t* best_j,
                                 double* relevance);
/* Milliseconds the calling thread's last GPU fs_pair_screen_labels spent on
 * upload, pack, relevance, the scan with its reduction and download (HIP
 * events; -1 where unavailable; above 4 states the per-labelling relevance
 * launches are timed with the scan), for the benchmark tool. */
FS_API int fs_pair_labels_last_timing(double* ms5);

#ifdef __cplusplus
}
#endif

#endif /* FASTSELECT_AMD_H */
