// fs_gpu_internal.h -- what the GPU backend's translation units share: the
// Plan (one scoring job's device state), the device helpers the kernels use,
// the launch helpers and the entry points each unit offers the others; the
// owners of device memory are in fs_devmem.h.  One unit per stage of the
// pipeline:
//
//   fs_gpu_mem.hip   devices, the device block cache, pinned host staging
//   fs_pass1.hip     k_quantize, k_dist, row moments, mean correction glue,
//                    calibration / row guard, SURF's averages and scoring
//   fs_select.hip    MultiSURF thresholds, refinement of ambiguous pairs,
//                    exact thresholds of flagged rows, near / far counts
//   fs_pass2.hip     pair weights, dense and sparse pass 2, segment reduce,
//                    reference-order masks / chains glue
//   fs_relieff.hip   ReliefF selection and update
//   fs_plan.hip      plan create / layout / shard / score entry points
//   fs_devices.hip   single-process multi-GPU (the estimators' devices=)
//   fs_stir.hip      STIR: hit / miss sums of diff and diff^2 over the near pairs
//   fs_stir_relieff.hip  the same sums over ReliefF's neighbour lists
//   fs_rrelieff.hip  RReliefF: the sums of a one-class ReliefF plan per target
//   fs_labels.hip    MultiSURF permutation test: many labellings on one plan's decisions
//   fs_relieff_labels.hip  ReliefF permutation test: many labellings on one pass 1
//   fs_surf_labels.hip     SURF / SURF* permutation test: many labellings on one distance stage
//
// Kernel map and rooflines: DESIGN.md §3.  No float atomics touch scores:
// every reduction has a fixed order, so two runs of the same input are
// bit-identical.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/fastselect_amd.h"
#include "fs_devmem.h"
#include "fs_internal.h"

namespace fs {
namespace gpu {

#define FS_HIP(expr)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) {                                                               \
      set_error(std::string("HIP error '") + hipGetErrorString(e_) + "' in " #expr);      \
      return FS_EHIP;                                                                     \
    }                                                                                     \
  } while (0)

// Launch shapes shared between units
constexpr int kRowcorrMaxSlices = 16;
constexpr int kExRows = 8, kExJ = 4, kExChunk = kExJ;
constexpr int kSWaves = 16;
constexpr int kTileWeights = kTile * kTile;  // floats of a tile in the sparse weight blocks (k_weights_sparse3)
constexpr int64_t kXsSlack = 512;
constexpr int kXcds = 8;

// ---------------------------------------------------------------------------
// Device helpers
// ---------------------------------------------------------------------------

__device__ __forceinline__ uint32_t sad_u32(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t d;
  asm("v_sad_u32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}

// c + |a.lo - b.lo| + |a.hi - b.hi| over unsigned 16-bit halves (two
// features per word; checked on gfx950 by tools/ubench/sad16_check.hip)
__device__ __forceinline__ uint32_t sad_u16(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t d;
  asm("v_sad_u16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}

// c + sc * [a != b] for small category codes, without lane masks (a
// compare would burn an SGPR pair per pair-accumulator).
__device__ __forceinline__ uint32_t mismatch_u32(uint32_t a, uint32_t b, uint32_t sc, uint32_t c) {
  uint32_t t, d;
  asm("v_xor_b32 %1, %2, %3\n\tv_min_u32 %1, %1, 1\n\tv_mad_u32_u24 %0, %1, %4, %5"
      : "=v"(d), "=&v"(t)
      : "v"(a), "v"(b), "v"(sc), "v"(c));
  return d;
}

// Fixed-shape block reduction of doubles (256 threads), deterministic.
__device__ __forceinline__ double block_sum_256(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// Distance storage.  Full layout (ReliefF / SURF, whose neighbour selection
// reads whole rows): D[i][j] over n_pad x n_pad, both halves.  Tiled layout
// (MultiSURF, whose kernels only ever read inside an owned tile): one
// 128 x 128 block per owned tile t, T_t[b][a] = D(i0 + a, j0 + b) -- half the
// memory of the full matrix for the whole triangle, and a rank of an N-GPU
// job holds only its 1/N of the tiles.  d_at(..., a, b) addresses element
// (i0 + a, j0 + b) of owned tile t either way; consecutive a are consecutive
// doubles in both layouts (the full layout reads it as D[j][i]).
__device__ __forceinline__ int64_t d_at(int tiled, int64_t n_pad, int64_t t, int64_t i0,
                                        int64_t j0, int a, int b) {
  return tiled ? ((t * kTile + b) * kTile + a) : ((j0 + b) * n_pad + i0 + a);
}

// Row window of the full layout (ReliefF / SURF row plans): only the rows
// [win.x, win.y) -- the plan's focal 128-sample blocks -- are stored, and the
// plan's D points where row 0 would be, so row r of the full matrix is still
// D + r * n_pad.  A whole fit stores every row; a row-sharded plan (one rank
// of N, a row panel) 1/N of them.  Writes skip rows outside the window; a
// read of (i0 + a, j0 + b) takes row j0 + b when it is stored and row i0 + a
// otherwise (D is symmetric, and every tile of a row plan has one of its two
// blocks inside the window).
__device__ __forceinline__ bool d_row_in(int2 win, int64_t r) { return r >= win.x && r < win.y; }
__device__ __forceinline__ int64_t d_rd(int tiled, int2 win, int64_t n_pad, int64_t t, int64_t i0,
                                        int64_t j0, int a, int b) {
  if (tiled) return (t * kTile + b) * kTile + a;
  const int64_t j = j0 + b;
  return d_row_in(win, j) ? j * n_pad + i0 + a : (i0 + a) * n_pad + j;
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
// Device memory of a Plan has one of two owners (fs_devmem.h).  Blocks that
// live and die together sit in one of four arenas, named at each allocation:
// mem_plan (sized by n: as long as the plan), mem_layout (sized by the feature
// layout: until the next plan_layout), mem_shard (sized by the owned tiles:
// until the next plan_set_shard) and mem_call (one plan_score, plan_stir or plan_score_labels call).  A buffer
// that grows on demand is a DevBuf member: reserve() synchronises the streams
// it is given, frees the old block and allocates the new size.  Kernels take
// the raw pointer (.p) and capacity (.cap).  plan_destroy synchronises the
// plan's streams; destroying the Plan then frees all of it.
struct Plan {
  explicit Plan(int dev) : device(dev) {}
  Prepared P;
  const int device;
  int rank = 0, world = 1;
  int x_is_f64 = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // MultiSURF's mean correction (k_colrank, k_rowcorr) runs on `side`,
  // forked after k_quantize and joined before k_rowstats_reduce, beside k_dist
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // MultiSURF*: the star split's per-sample sums on a stream of their own
  // (beside k_dist and the correction), joined by run_weights
  hipStream_t side2 = nullptr;
  hipEvent_t ev_star = nullptr;
  int64_t nb = 0, n_tiles = 0, seg_len = 1, nseg = 1;
  int64_t nsegpart = 1;         // rows of spart (nseg, or 2 * nseg sparse: one per half)
  int ksplit = 1;               // pass-1 K-split parts of the tail tiles (k_dist)
  int64_t kfull = 0;            // tiles k_dist computes whole (the rest are split)
  int use_q16 = 0;              // pass 1 on packed 16-bit continuous operands
  double calib[7] = {0, 0, 0, 0, 1, 0, 0};  // plan_calibration (calibrate_band, row_guard)
  double cal32[2] = {0, 0};     // sampled rms / max error of 32-bit operands (row_guard)
  int64_t c_lo = 0, c_hi = 0;   // this rank's continuous columns of the mean correction
  int64_t r_lo = 0, r_hi = 0;   // focal rows scored by this plan (row sharding)
  double2* rspart = nullptr;    // per owned tile row-moment partials [tiles][256]
  double* Dpart = nullptr;      // (ksplit - 1) partial distance planes
  int key_shift = 8;             // colsort_key shift of the current scale
  DevBuf<char> colsort_scratch{device};  // large-n route of colsort_terms (its stream: run_colsort)
  // device buffers
  void* x = nullptr;            // X on the device: the plan's own, or a staged copy
  const void* x_staged = nullptr;  // the staged copy x reads (staged_acquire), released by plan_destroy
  int64_t* src_col = nullptr;
  int64_t* out_pos = nullptr;
  double *off = nullptr, *qs = nullptr, *scl = nullptr;
  float* scl32 = nullptr;       // scl as float (k_exact_pairs_rows)
  bool rows_direct = false;     // kept features = X's columns, all continuous, f32, 16-B pitch
  int64_t* dtab_off = nullptr;
  double* dtab = nullptr;
  int32_t* lab = nullptr;
  uint8_t* lab8 = nullptr;  // ReliefF: class codes as bytes (zero padding)
  uint32_t* xqT = nullptr;
  float* xs = nullptr;
  float* epsT = nullptr;
  double* corr = nullptr;
  double* corr_part = nullptr;  // [rowcorr_slices][n_pad] k_rowcorr slice partials
  double* xT64 = nullptr;      // SURF: float64 feature-major operands (the float64 route)
  bool surf_int = false;        // SURF: integer distances resolved to float32 (fs_surfint.hip)
  double* D = nullptr;
  int tiled = 0;                // D in the tiled layout (MultiSURF; d_at)
  int64_t dplane = 0;           // doubles of one distance plane (D, each Dpart)
  int2 tw = make_int2(0, 0);    // k_exact_pairs' store_pair: (nb, world) when tiled
  int2 win = make_int2(0, 0);   // full layout: rows [win.x, win.y) stored (d_row_in)
  void* D_alloc = nullptr;      // allocation behind D (D itself points at row 0)
  float* Dk = nullptr;          // ReliefF: the float32 keys instead of D (same layout)
  int2* tiles = nullptr;
  double* thr = nullptr;
  float* Wt = nullptr;          // dense pair weights (sparse == 0)
  float* wrow = nullptr;        // sparse pair weights, row-major per wave (sparse == 1)
  unsigned long long* nnz = nullptr;  // non-zero weights of the last pass 2
  bool nnz_valid = false;
  int sparse = 0;               // pass 2 over non-zero weights only
  // MultiSURF* / SURF* split (fs_starterm.hip): pass 2 weighs the near pairs
  // only and the far pairs' all-pairs part comes per column from its sorted
  // values: xsT (float32 pass-2 values, feature-major), the per-sample
  // coefficients `alpha` and the per-column terms `tcol` k_reduce adds
  bool star_split = false;
  float* xsT = nullptr;
  double* alpha = nullptr;
  double* tcol = nullptr;
  DevBuf<double> spart{device};   // pass-2 segment partials (shard_segments)
  // sparse pass-2 schedule (build_sparse_schedule): tile order, segment
  // offsets and the unit tables of the F = 8 / F = 4 launches
  std::vector<int2> h_tiles;      // the owned tiles (host copy of `tiles`)
  DevBuf<int32_t> sched{device};  // the tile order, then the segment offsets
  int32_t* seg_off = nullptr;     // inside sched
  DevBuf<int2> units8{device};    // the F = 8 units, then the F = 4 ones, then the 8-wave kernel's
  int2* units4 = nullptr;         // inside units8
  int2* unitsw = nullptr;         // inside units8
  int64_t nunits8 = 0, nunits4 = 0, nfb8 = 0, nfb4 = 0, f_tail = 0;
  // k_score_sparse3_w8 (choose_w8): its 256-feature blocks cover features
  // [0, f_w8), the F = 8 / F = 4 launches the rest
  int64_t nunitsw = 0, nfbw = 0, f_w8 = 0;
  // exact thresholds of uncertain rows (exact_thresholds)
  unsigned int* unc = nullptr;  // [n_pad] row flags
  int32_t* urows = nullptr;     // [n_pad + 1] flagged rows in index order, then their count
  DevBuf<double2> uparts{device};  // [thr_rows][nchunk] exact row-moment partials
  int thr_rows = kExactThrRows; // rows fixed at most: exact_thr_rows(n) (thr_exact_all test hook: all)
  bool thr_all = false;
  int32_t n_exact_thr = 0;      // rows whose threshold the last select recomputed (-1: too many)
  // ambiguous-pair refinement
  DevBuf<int2> list{device};
  DevBuf<double> pair_part{device};  // k_exact_pairs_rows' per-pair sums between feature chunks
  unsigned long long* list_count = nullptr;
  int64_t n_refined = 0;
  int64_t n_tie_rows = 0;      // ReliefF rows re-ordered by k_rf_ties
  DevBuf<char> sort_scratch{device};  // pair-list sort (fs_sort.hip)
  // ev[0..1] distance kernel, ev[2..3] score kernel(s) / ReliefF selection +
  // update, ev[4..5] ReliefF's first k_rf_select launch (plan_kernel_ms)
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // plan_stir (fs_stir.hip): per chunk of tiles the weights kernel's and the
  // score kernel's start / stop events (plan_stir_kernel_ms), taken on demand
  std::vector<hipEvent_t> ev_stir;
  int stir_chunks = 0;          // chunks the last plan_stir walked
  // plan_score_stir (fs_stir_relieff.hip): k_rf_stir's start / stop events,
  // taken on the first call; rf_stir_timed: the last plan_score_stir ran it
  hipEvent_t ev_rf_stir[2] = {nullptr, nullptr};
  bool rf_stir_timed = false;
  // plan_score_labels (fs_labels.hip): the record kernels' start / stop
  // events, then per chunk of labellings the counts kernels' and the score
  // kernel's (plan_labels_kernel_ms), taken on demand
  std::vector<hipEvent_t> ev_labels;
  int labels_chunks = -1;       // chunks the last plan_score_labels walked (-1: none)
  // plan_relieff_score_labels (fs_relieff_labels.hip): the last call's route
  // counts and depth (plan_relieff_labels_info; [0] < 0: no call yet), its
  // summed kernel times (plan_relieff_labels_kernel_ms) and the two events
  // that time one labelling's general route and the six of the fast route's
  // stages (prefix, walk, score), taken on the first call
  int64_t rf_labels_info[4] = {-1, 0, 0, 0};
  double rf_labels_ms[4] = {0, 0, 0, 0};
  hipEvent_t ev_rf_labels[2] = {nullptr, nullptr};
  hipEvent_t ev_rf_fast[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // plan_surf_score_labels (fs_surf_labels.hip): the last call's counts
  // (plan_surf_labels_info; [0] < 0: no call yet), its summed stage times
  // (plan_surf_labels_kernel_ms) and its events, taken on demand: [0..1] the
  // distance and record stage, [2..3] the column sort, then per chunk of
  // labellings the weights', the score kernel's and the star walk's
  int64_t surf_labels_info[4] = {-1, 0, 0, 0};
  double surf_labels_ms[4] = {0, 0, 0, 0};
  std::vector<hipEvent_t> ev_surf_labels;
  // plan_score_targets (fs_rrelieff.hip): the selection's start / stop events
  // and per chunk of targets k_rrf_update's (plan_targets_kernel_ms), taken
  // on demand; rrf_chunks: chunks the last completed call walked (-1: none)
  hipEvent_t ev_rrf_sel[2] = {nullptr, nullptr};
  std::vector<hipEvent_t> ev_rrf;
  int rrf_chunks = -1;
  DevArena mem_plan{device};    // buffers sized by n (live as long as the plan)
  DevArena mem_layout{device};  // buffers sized by the feature layout (PW)
  DevArena mem_shard{device};   // buffers sized by the owned tiles (plan_set_shard)
  DevArena mem_call{device};    // buffers of one plan_score / plan_stir call
  bool row_mode = false;
  // the row guard's quantised operands and mean correction are the first
  // step's (one plan over every continuous column): pass 1 takes them
  bool corr_ready = false;
  bool guard_pending = false;       // the row guard waits for the first pass 1 (P.defer_guard)
  std::vector<char> colmin, colmax; // per input column, x's dtype (device-measured)
  // reference-order accumulation (P.ref_accum, fs_refacc.hip): the kept
  // columns of X (float32 [n_pad][Kp]), their recip / discreteness, the
  // discrete flag of each 256-feature block (layout buffers); MultiSURF's
  // decision masks [n_pad][n_pad / 64][4] (plan buffer) and the per-batch
  // flagged-row counts of exact_thresholds
  float* xk = nullptr;
  double* xk64 = nullptr;       // SURF: the kept columns of its float64 X [n_pad][Kp]
  int64_t Kp = 0;
  int64_t* kcol = nullptr;
  float* krecip = nullptr;
  uint8_t* kdisc = nullptr;
  uint8_t* kblk = nullptr;
  uint64_t* masks = nullptr;
  int32_t* bcnt = nullptr;
  DevBuf<float> temp{device};   // the reference's temp rows [rows][Kp]
  int64_t ref_rows = -1;        // rows of temp the last plan_ref_pass2 / _temp wrote (-1: none)
  bool ref_defer = false;       // ReliefF reference order: stop at the temp rows (plan_ref_temp)
  DevBuf<float> rkeys{device};  // ReliefF neighbour keys
  bool ref_seeded = false;      // ReliefF: the column sums continue from the sums buffer
  double* risk_dev = nullptr;   // plan_decision_guard's result (mem_plan, allocated on first use)
};

#define FS_TRY(expr)              \
  do {                            \
    int rc_ = (expr);             \
    if (rc_ != FS_OK) return rc_; \
  } while (0)

template <typename T>
int h2d(Plan* g, T* dst, const T* src, size_t count) {
  if (count == 0) return FS_OK;
  FS_HIP(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, g->stream));
  return FS_OK;
}

inline int launch_check(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error(std::string("kernel launch failed (") + what + "): " + hipGetErrorString(e));
    return FS_EHIP;
  }
  return FS_OK;
}

// ---------------------------------------------------------------------------
// Entry points between units
// ---------------------------------------------------------------------------
// fs_gpu_mem.hip: pooled streams (non-blocking) and events (timing or not)
hipStream_t stream_get(int device);
void stream_put(int device, hipStream_t s);
hipEvent_t event_get(int device, bool timing);
void event_put(int device, hipEvent_t e, bool timing);
// A pooled stream and timing events for one call or one handle.  Declare it
// after the arenas and buffers whose blocks the stream uses: it is destroyed
// first, so the stream is synchronised before any block is freed on every
// return path.
struct StreamLease {
  int device;
  hipStream_t s = nullptr;
  std::vector<hipEvent_t> ev;
  explicit StreamLease(int dev) : device(dev) {}
  StreamLease(const StreamLease&) = delete;
  StreamLease& operator=(const StreamLease&) = delete;
  int open(size_t events) {  // stream_get / event_get have set the error
    if (!(s = stream_get(device))) return FS_EHIP;
    for (size_t k = 0; k < events; k++) {
      ev.push_back(event_get(device, true));
      if (!ev.back()) return FS_EHIP;
    }
    return FS_OK;
  }
  ~StreamLease() {
    if (s) {
      (void)hipStreamSynchronize(s);
      stream_put(device, s);
    }
    for (hipEvent_t e : ev) event_put(device, e, true);
    (void)hipGetLastError();
  }
};
inline int no_device() {
  set_error("backend='gpu' requested but no HIP device is visible");
  return FS_ENODEV;
}
// fs_pass1.hip
int choose_ksplit(int64_t tiles, int device, int nchunks, int64_t feats, bool beside);
int calibrate_band(Plan* g);
int row_guard(Plan* g);
// after a 32-bit switch: the operand scale and sort key on the device
int apply_operand_width(Plan* g);
int run_quantize_dist(Plan* g);
int plan_score_surf(Plan* g, double* sums_dev);
// SURF's distance stage alone: run_quantize_dist, then the means into thr and
// (integer route) every stored distance as its float32 value
int surf_distances(Plan* g);
// fs_surfint.hip: after k_dist on a SURF plan's integer operands, the focal
// rows' means into thr and every stored distance as its float32 value
int surf_resolve(Plan* g);
// fs_starterm.hip: the star split's sizes (n <= 24576, up to 8 classes);
// SURF*'s per-column all-pairs terms of this plan's focal rows into g->tcol
// (star_terms, beside pass 1); MultiSURF*'s in two steps: star_sums (beside
// pass 1: every sample's sum over the other classes, into xsT in place; the
// continuous columns' come with the mean correction's sort, colsort_star_terms,
// unless `continuous`), then
// star_reduce once the neighbour counts are known (alpha-weighted column sums
// of this rank's column share into g->tcol).  All launched on st.
bool star_split_fits(int64_t n, int32_t n_classes);
int star_terms(Plan* g, hipStream_t st);
int star_sums(Plan* g, hipStream_t st, bool continuous);
int star_reduce(Plan* g, const double* counts, hipStream_t st);
// fs_starterm.hip, for the SURF* permutation test (fs_surf_labels.hip).
// star_lab_sort: every scored column of xsT [PW][n_pad] sorted once, without
// the labels: sval[c][k] the k-th smallest value (a discrete column: its
// float's bits, equal inside a run), sidx[c][k] its sample, tcol[c] = T_c =
// the sum of d_c over all pairs, in float64 in the order of the sort.
// star_lab_split: the items per segment and segments per column of the walk
// (star_lab_seg hook honoured).  star_lab_walk: for the nb labellings of labT
// ([n][32], codes in [0, 8)) the same-class sums Hs of every column into
// hs[(c * nseg + seg) * 32 + b]; cnt: 4 * PW * nseg * 32 uint64 of scratch
// (unused when nseg == 1), ncls: 64 uint64.  star_lab_apply: scores[b][o] =
// 2 scores[b][o] - 2 (T_c - 2 Hs[c][b]) with the segments added in order.
int star_lab_sort(Plan* g, const float* xsT, float* sval, uint16_t* sidx, double* tcol,
                  hipStream_t st);
void star_lab_split(const Plan* g, int64_t* seg_items, int64_t* nseg);
int star_lab_walk(Plan* g, const float* sval, const uint16_t* sidx, const int32_t* labT, int nb,
                  int64_t seg_items, int64_t nseg, uint64_t* ncls, uint64_t* cnt, double* hs,
                  hipStream_t st);
int star_lab_apply(Plan* g, const double* tcol, const double* hs, int64_t nseg, int nb,
                   double* scores, hipStream_t st);
// fs_pass2.hip
int shard_segments(Plan* g);
int choose_w8(int64_t units, double tiles_per_seg);  // fs_plan.hip
int run_weights(Plan* g, const double* counts, int algo, double inv_sc);
int run_pass2(Plan* g, double* scores_dev);
int ref_masks(Plan* g);
int ref_temp(Plan* g, int64_t rows, float** out);
int ref_chains(Plan* g, const double* counts, double* scores);
// SURF reference order (plan_score_surf): the focal rows' masks, chains and
// float32 column sums (seeded by sums when g->ref_seeded; stopping at the
// temp rows when g->ref_defer), after the distances and means.
int surf_ref(Plan* g, double* sums);
// dst[k] += src[k] over count doubles (k_accumulate)
int accumulate(double* dst, const double* src, int64_t count, hipStream_t st);
// sums[out_pos[c]] = the fixed-order sum of part[0..nrows)[c] (k_reduce),
// plus add[c] when add is given
int reduce_segments(const double* part, int64_t nrows, int64_t PW, const int64_t* out_pos,
                    double* sums, hipStream_t st, const double* add = nullptr);
// fs_relieff.hip.  kRfRows: focal rows per workgroup of k_rf_update and
// k_rf_stir (their partials have one row per block of kRfRows).  stir_dev /
// counts_dev: the optional STIR output (plan_score_stir), summed over the
// neighbour lists right after the selection.
constexpr int64_t kRfRows = 64;
int plan_score_relieff(Plan* g, double* sums_dev, double* stir_dev = nullptr,
                       double* counts_dev = nullptr);
// Fast accumulation after a selection: k_rf_update over nbr / nfound and the
// fold into sums_dev (plan_score_relieff's tail); relieff_select_update: the
// selection first, on resident distances, with the plan's current lab / lab8
// and g->P's class count (one general-route labelling of
// plan_relieff_score_labels).
int relieff_update_fold(Plan* g, const double* dprior, const int32_t* nbr, const int32_t* nfound,
                        double* part, double* sums_dev);
int relieff_select_update(Plan* g, const int64_t* dcc, const double* dprior, int32_t* nbr,
                          int32_t* nfound, double* part, double* sums_dev);
// The selection alone, on resident distances (run_quantize_dist): the lists
// nbr[n][C][k] / nfound[n][C] of the plan's focal rows, dcc the class counts
// on the device (fs_rrelieff.hip scores targets on a one-class plan's lists).
int relieff_select(Plan* g, const int64_t* dcc, int32_t* nbr, int32_t* nfound);
// Exact float32 keys of whole rows (drows on the device) into keys[nr][n],
// +inf at the focal sample; and numba's order for the runs of equal keys in
// the candidate prefixes cand[i][0..lok[i]) (L per row, sorted keys ckeys) of
// the rows tie_rows (fs_relieff_labels.hip).
int relieff_exact_rows(Plan* g, const int32_t* drows, int64_t nr, float* keys);
int relieff_prefix_ties(Plan* g, const std::vector<int32_t>& tie_rows, int64_t L, int32_t* cand,
                        const int32_t* lok, const float* ckeys);
// fs_labels.hip, for record lists of other makers (fs_relieff_labels.hip):
// labT[i * 32 + b] from nb raw labellings on the device (k_lab_transpose);
// the split of k_lab_score over n_tiles groups of records (labels_seg_len
// hook honoured); k_lab_score + k_lab_reduce of nb labellings into
// scores[nb][n_kept] (part: nb * nseg * PW doubles; `scored`: an event
// recorded between the two).  plan_score_labels launches through them too.
// lab_records: the record stage of one call into g->mem_call (rec: nrec
// records in whole groups per tile, goff; Nn[i] = |N_i|; wcnt: the weighted
// pairs per wave quarter of a tile), with MultiSURF's decisions or (surf) SURF's:
// (double)(float)D against thr.  One host synchronisation.
int lab_transpose(Plan* g, const int32_t* lab_raw, int nb, int32_t* labT);
int lab_records(Plan* g, bool surf, uint32_t** wcnt, int64_t** goff, uint32_t** Nn, int2** rec,
                int64_t* nrec);
void lab_score_split(const Plan* g, int64_t n_tiles, int64_t* seg_len, int64_t* nseg);
int lab_score_reduce(Plan* g, const int2* rec, const int64_t* goff, const float* W,
                     int64_t n_tiles, int64_t seg_len, int64_t nseg, int nb, double* part,
                     double* scores, hipEvent_t scored = nullptr);
// fs_stir_relieff.hip: the four STIR sums and the pair counts of the focal
// rows' neighbour lists nbr / nfound (relieff_select's, in the call arena)
int relieff_stir_sums(Plan* g, const int32_t* nbr, const int32_t* nfound, double* stir_dev,
                      double* counts_dev);
int relieff_run_one(const Prepared& P, const void* x, int device, int64_t r_lo, int64_t r_hi,
                    double* sums_out, const double* seed = nullptr);
// fs_plan.hip
// whether one ReliefF / SURF plan holds the distance rows of every sample (a
// one-shot call then scores without row panels)
bool rows_fit_one_plan(const Prepared& P, int device);
int plan_layout(Plan* g);
int copy_sums(Plan* g, const double* sums_dev, double* sums_out);
int surf_run_one(const Prepared& P, const void* x, int device, int64_t r_lo, int64_t r_hi,
                 double* sums_out, const double* seed = nullptr);
// the decision guard's last risk / re-run of this thread (plan_decision_guard)
extern thread_local double g_last_risk;
extern thread_local int g_last_rerun;
// the star form of this thread's last one-shot MultiSURF call (multisurf_last_star_split)
extern thread_local int g_last_star;

}  // namespace gpu
}  // namespace fs
