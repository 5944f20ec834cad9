// fs_api.cpp -- the C ABI (include/fastselect_amd.h): argument validation,
// backend dispatch, error reporting.  See the header for the reference
// interface each entry point replaces.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fastselect_amd.h"
#include "fs_cfs.h"
#include "fs_internal.h"
#include "fs_jmi.h"
#include "fs_mdr.h"
#include "fs_mi.h"
#include "fs_mrmr.h"
#include "fs_pairscan.h"
#include "fs_rrelieff.h"
#include "fs_stir.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>

namespace fs {
static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }

static thread_local int g_accum = FS_ACCUM_FAST;
int accumulation_mode() { return g_accum; }

TestHooks& test_hooks() {
  static TestHooks h;
  return h;
}

bool trace_on() {
  static const bool on = std::getenv("FS_TRACE") != nullptr;
  return on;
}

void trace_mark(const char* phase) {
  if (!trace_on()) return;
  using clk = std::chrono::steady_clock;
  static thread_local clk::time_point last = clk::now();
  const clk::time_point now = clk::now();
  std::fprintf(stderr, "[fs_trace] %-22s %9.3f ms\n", phase,
               std::chrono::duration<double, std::milli>(now - last).count());
  last = now;
}
}  // namespace fs

using namespace fs;

static int map_prep_rc(int rc) { return rc == 0 ? FS_OK : FS_EINVAL; }

// The calling thread's accumulation mode into a prepared problem
// (fs_set_accumulation).  Reference order: MultiSURF's and ReliefF's
// per-sample sums and column sums (MultiSURF.py:198-253, ReliefF.py:181-220),
// SURF's in its n_jobs = 1 order (SURF.py:139-218: with more threads the
// reference adds its per-thread rows in schedule order); MultiSURF then
// takes 32-bit pass-1 operands.
static int apply_accumulation(Prepared& P) {
  P.ref_accum = g_accum == FS_ACCUM_REFERENCE ? 1 : 0;
  if (P.ref_accum && P.algo == ALGO_MULTISURF && !test_hooks().ref_q16) P.no_q16 = 1;
  return FS_OK;
}

static int no_reference_devices() {
  if (g_accum != FS_ACCUM_REFERENCE) return FS_OK;
  set_error("reference-order accumulation runs on one device (its column sums are one "
            "sequential float32 sum per feature)");
  return FS_ENOTSUP;
}

static int check_backend(int backend, int device) {
  if (backend != FS_BACKEND_CPU && backend != FS_BACKEND_GPU) {
    set_error("backend must be FS_BACKEND_CPU or FS_BACKEND_GPU");
    return FS_EINVAL;
  }
  if (backend == FS_BACKEND_GPU) {
    const int nd = gpu::device_count();
    if (nd <= 0) {
      set_error("backend='gpu' was selected, but no HIP device (MI355X) is visible");
      return FS_ENODEV;
    }
    if (device < 0 || device >= nd) {
      set_error("device ordinal out of range");
      return FS_EINVAL;
    }
  }
  return FS_OK;
}

// devices[0..n) for the multi-device entry points: at least one, each a
// visible HIP ordinal (repeats allowed: several plans share a device).
static int check_devices(const int* devices, int n) {
  if (!devices || n < 1) {
    set_error("devices: need at least one device ordinal");
    return FS_EINVAL;
  }
  const int nd = gpu::device_count();
  if (nd <= 0) {
    set_error("backend='gpu' was selected, but no HIP device (MI355X) is visible");
    return FS_ENODEV;
  }
  for (int i = 0; i < n; i++)
    if (devices[i] < 0 || devices[i] >= nd) {
      set_error("devices: ordinal " + std::to_string(devices[i]) + " out of range (" +
                std::to_string(nd) + " visible)");
      return FS_EINVAL;
    }
  return FS_OK;
}

extern "C" {

const char* fs_version(void) { return "fastselect_amd 0.1.0 (gfx950)"; }

const char* fs_last_error(void) { return g_last_error.c_str(); }

int fs_device_count(void) { return gpu::device_count(); }

int fs_set_accumulation(int mode, int* previous) {
  if (mode != FS_ACCUM_FAST && mode != FS_ACCUM_REFERENCE) {
    set_error("accumulation mode must be FS_ACCUM_FAST or FS_ACCUM_REFERENCE");
    return FS_EINVAL;
  }
  if (previous) *previous = g_accum;
  g_accum = mode;
  return FS_OK;
}

int fs_get_accumulation(void) { return g_accum; }

int fs_test_hook(const char* name, int64_t value) {
  if (!name) {
    set_error("fs_test_hook: name is NULL");
    return FS_EINVAL;
  }
  TestHooks& h = test_hooks();
  const std::string k(name);
  if (k == "reset") h = TestHooks();
  else if (k == "ksplit") h.ksplit = value;
  else if (k == "q16") h.q16 = value;
  else if (k == "sparse") h.sparse = value;
  else if (k == "shards") h.shards = value;
  else if (k == "q16_guard_off") h.q16_guard_off = value;
  else if (k == "thr_exact_all") h.thr_exact_all = value;
  else if (k == "exact_gather") h.exact_gather = value;
  else if (k == "row_panel") h.row_panel = value;
  else if (k == "rf_xlds") h.rf_xlds = value;
  else if (k == "rf_fcap") h.rf_fcap = value;
  else if (k == "ties_1w") h.ties_1w = value;
  else if (k == "ties_coop") h.ties_coop = value;
  else if (k == "rf_ref_replay") h.rf_ref_replay = value;
  else if (k == "ref_q16") h.ref_q16 = value;
  else if (k == "surf_f64") h.surf_f64 = value;
  else if (k == "star_split") h.star_split = value;
  else if (k == "star_dense_ranks") h.star_dense_ranks = value;
  else if (k == "colsort_star") h.colsort_star = value;
  else if (k == "colsort_bins12") h.colsort_bins12 = value;
  else if (k == "colsort_global") h.colsort_global = value;
  else if (k == "mi_tiles") h.mi_tiles = value;
  else if (k == "list_cap") h.list_cap = value;
  else if (k == "cfs_rows_cap") h.cfs_rows_cap = value;
  else if (k == "seg_len") h.seg_len = value;
  else if (k == "pass2_generic") h.pass2_generic = value;
  else if (k == "pass2_w8") h.pass2_w8 = value;
  else if (k == "mdr_top_cap") h.mdr_top_cap = value;
  else if (k == "mdr_ranks") h.mdr_ranks = value;
  else if (k == "mdr_blocks") h.mdr_blocks = value;
  else if (k == "mdr_labels") h.mdr_labels = value;
  else if (k == "pair_tiles") h.pair_tiles = value;
  else if (k == "pair_cap") h.pair_cap = value;
  else if (k == "pair_labels") h.pair_labels = value;
  else if (k == "pair_lab_ranks") h.pair_lab_ranks = value;
  else if (k == "stir_chunk") h.stir_chunk = value;
  else if (k == "stir_seg_len") h.stir_seg_len = value;
  else if (k == "labels_chunk") h.labels_chunk = value;
  else if (k == "labels_seg_len") h.labels_seg_len = value;
  else if (k == "star_lab_seg") h.star_lab_seg = value;
  else if (k == "rf_labels_route") h.rf_labels_route = value;
  else if (k == "rf_labels_depth") h.rf_labels_depth = value;
  else if (k == "rf_labels_depth_cap") h.rf_labels_depth_cap = value;
  else {
    set_error("fs_test_hook: unknown hook '" + k + "'");
    return FS_EINVAL;
  }
  return FS_OK;
}

int fs_multisurf_last_guard(double* risk_out, int* rerun_out) {
  return gpu::multisurf_last_guard(risk_out, rerun_out);
}

int fs_multisurf_last_star_split(int* split_out) {
  if (!split_out) {
    set_error("split_out is NULL");
    return FS_EINVAL;
  }
  *split_out = gpu::multisurf_last_star_split();
  return FS_OK;
}

int fs_device_cache_release(void) {
  gpu::dev_cache_release();
  return FS_OK;
}

int fs_host_alloc(uint64_t bytes, void** out) {
  if (!out) {
    set_error("fs_host_alloc: out is NULL");
    return FS_EINVAL;
  }
  *out = nullptr;
  if (gpu::device_count() <= 0) {
    set_error("backend='gpu' requested but no HIP device is visible");
    return FS_ENODEV;
  }
  return gpu::host_alloc(out, (size_t)bytes);
}

int fs_host_free(void* p) {
  gpu::host_free(p);
  return FS_OK;
}

int fs_stage_x(int device, const void* x, int x_is_f64, int64_t n, int64_t p, uint64_t* staged) {
  if (!x || !staged || n < 1 || p < 1) {
    set_error("fs_stage_x: need x, staged, n >= 1 and p >= 1");
    return FS_EINVAL;
  }
  if (gpu::device_count() <= 0) {
    set_error("backend='gpu' requested but no HIP device is visible");
    return FS_ENODEV;
  }
  return gpu::stage_x(device, x, x_is_f64, n, p, staged);
}

int fs_stage_x_device(int device, const void* x, const void* x_device, int x_is_f64, int64_t n,
                      int64_t p, uint64_t* staged) {
  if (!x || !x_device || !staged || n < 1 || p < 1) {
    set_error("fs_stage_x_device: need x, x_device, staged, n >= 1 and p >= 1");
    return FS_EINVAL;
  }
  if (gpu::device_count() <= 0) {
    set_error("backend='gpu' requested but no HIP device is visible");
    return FS_ENODEV;
  }
  return gpu::stage_x_device(device, x, x_device, x_is_f64, n, p, staged);
}

int fs_stage_x_cast(int device, const void* x, int x_is_f64, int64_t n, int64_t p, int n_jobs,
                    float* out, int* finite, uint64_t* staged) {
  if (!x || !out || !finite || !staged || n < 1 || p < 1) {
    set_error("fs_stage_x_cast: need x, out, finite, staged, n >= 1 and p >= 1");
    return FS_EINVAL;
  }
  if (gpu::device_count() <= 0) {
    set_error("backend='gpu' requested but no HIP device is visible");
    return FS_ENODEV;
  }
  return gpu::stage_x_cast(device, x, x_is_f64, n, p, n_jobs, out, finite, staged);
}

int fs_unstage_x(uint64_t staged) { return gpu::unstage_x(staged); }

int fs_all_finite(const void* x, int x_is_f64, int64_t n, int64_t p, int n_jobs, int* finite) {
  if (!x || !finite || n < 0 || p < 0) {
    set_error("fs_all_finite: need x, finite, n >= 0 and p >= 0");
    return FS_EINVAL;
  }
  *finite = cpu::all_finite(x, x_is_f64, n * p, n_jobs);
  return FS_OK;
}

int fs_column_stats(int backend, int device, const void* x, int x_is_f64, int64_t n, int64_t p,
                    int64_t count_cap, void* colmin_out, void* colmax_out,
                    int64_t* ndistinct_out) {
  int rc = check_backend(backend, device);
  if (rc != FS_OK) return rc;
  if (!x || !colmin_out || !colmax_out || !ndistinct_out || n < 1 || p < 1 || count_cap < 0) {
    set_error("fs_column_stats: need x, outputs, n >= 1, p >= 1 and count_cap >= 0");
    return FS_EINVAL;
  }
  const int f64 = x_is_f64 ? 1 : 0;
  trace_mark("column_stats: enter");
  if (backend == FS_BACKEND_GPU)
    rc = gpu::column_stats(x, f64, n, p, count_cap, device, colmin_out, colmax_out, ndistinct_out);
  else
    rc = cpu::column_stats(x, f64, n, p, count_cap, -1, colmin_out, colmax_out, ndistinct_out);
  trace_mark("column_stats");
  return rc;
}

int fs_multisurf_score(int backend, int device, const float* x, int64_t n, int64_t p,
                       const double* y, const float* recip, const int64_t* feat_idx,
                       int64_t n_kept, int use_star, const uint8_t* is_discrete, int n_jobs,
                       float* scores_out) {
  if (!scores_out) {
    set_error("scores_out is NULL");
    return FS_EINVAL;
  }
  int rc = check_backend(backend, device);
  if (rc != FS_OK) return rc;
  Prepared P;
  trace_mark("multisurf: enter");
  rc = prepare(P, ALGO_MULTISURF, x, 0, n, p, feat_idx, n_kept, recip, is_discrete, n_jobs,
               backend == FS_BACKEND_GPU);
  trace_mark("prepare (host)");
  if (rc) return map_prep_rc(rc);
  if (encode_labels_f64(P, y)) return FS_EINVAL;
  P.use_star = use_star ? 1 : 0;
  if ((rc = apply_accumulation(P)) != FS_OK) return rc;
  if (backend == FS_BACKEND_GPU) return gpu::multisurf_run(P, x, device, scores_out);
  cpu::CpuState st;
  std::vector<double> rs(3 * n), cnt(2 * n), S(P.n_kept);
  cpu::multisurf_pass1(P, x, 0, 1, n_jobs, st, rs.data());
  cpu::multisurf_select(P, x, 0, 1, rs.data(), n_jobs, st, cnt.data());
  cpu::multisurf_pass2(P, x, st, cnt.data(), 0, 1, n_jobs, 0, n, S.data());
  for (int64_t k = 0; k < P.n_kept; k++) scores_out[k] = (float)(S[k] / (double)n);
  return FS_OK;
}

int fs_multisurf_score_rows(int backend, int device, const float* x, int64_t n, int64_t p,
                            const double* y, const float* recip, const int64_t* feat_idx,
                            int64_t n_kept, int use_star, const uint8_t* is_discrete, int n_jobs,
                            int64_t row_begin, int64_t row_end, double* sums_out) {
  if (!sums_out) {
    set_error("sums_out is NULL");
    return FS_EINVAL;
  }
  if (!(0 <= row_begin && row_begin <= row_end && row_end <= n)) {
    set_error("row range must satisfy 0 <= row_begin <= row_end <= n");
    return FS_EINVAL;
  }
  int rc = check_backend(backend, device);
  if (rc != FS_OK) return rc;
  Prepared P;
  rc = prepare(P, ALGO_MULTISURF, x, 0, n, p, feat_idx, n_kept, recip, is_discrete, n_jobs,
               backend == FS_BACKEND_GPU);
  if (rc) return map_prep_rc(rc);
  if (encode_labels_f64(P, y)) return FS_EINVAL;
  P.use_star = use_star ? 1 : 0;
  if ((rc = apply_accumulation(P)) != FS_OK) return rc;
  if (backend == FS_BACKEND_GPU) return gpu::multisurf_rows(P, x, device, row_begin, row_end, sums_out);
  cpu::CpuState st;
  std::vector<double> rs(3 * n), cnt(2 * n);
  cpu::multisurf_pass1(P, x, 0, 1, n_jobs, st, rs.data());
  cpu::multisurf_select(P, x, 0, 1, rs.data(), n_jobs, st, cnt.data());
  return cpu::multisurf_pass2(P, x, st, cnt.data(), 0, 1, n_jobs, row_begin, row_end, sums_out);
}

int fs_multisurf_score_labels(int backend, int device, const float* x, int64_t n, int64_t p,
                              const int32_t* labels, int64_t B, const float* recip,
                              const int64_t* feat_idx, int64_t n_kept, const uint8_t* is_discrete,
                              int n_jobs, float* scores_out) {
  if (!scores_out || !labels || B < 1) {
    set_error("fs_multisurf_score_labels: need labels, scores_out and B >= 1");
    return FS_EINVAL;
  }
  int rc = check_backend(backend, device);
  if (rc != FS_OK) return rc;
  Prepared P;
  rc = prepare(P, ALGO_MULTISURF, x, 0, n, p, feat_idx, n_kept, recip, is_discrete, n_jobs,
               backend == FS_BACKEND_GPU);
  if (rc) return map_prep_rc(rc);
  if (encode_labels_i32(P, labels)) return FS_EINVAL;  // labelling 0 is the plan's y
  if ((rc = apply_accumulation(P)) != FS_OK) return rc;
  if (P.ref_accum) {
    set_error("fs_multisurf_score_labels: not built for reference-order accumulation");
    return FS_ENOTSUP;
  }
  if (backend == FS_BACKEND_GPU)
    return gpu::multisurf_labels_run(P, x, device, labels, B, scores_out);
  cpu::CpuState st;
  std::vector<double> rs(3 * n), cnt(2 * n), S((size_t)B * P.n_kept);
  cpu::multisurf_pass1(P, x, 0, 1, n_jobs, st, rs.data());
  cpu::multisurf_select(P, x, 0, 1, rs.data(), n_jobs, st, cnt.data());
  if ((rc = cpu::multisurf_score_labels(P, x, st, labels, B, n_jobs, S.data())) != FS_OK) return rc;
  for (int64_t k = 0; k < B * P.n_kept; k++) scores_out[k] = (float)(S[k] / (double)n);
  return FS_OK;
}

// Shared by the one-shot and the row-range entry points: validate, prepare,
// score the focal samples [r_lo, r_hi) -> float64 sums (not divided by n).
static int relieff_sums(int backend, int device, const float* x, int64_t n, int64_t p,
                        const int32_t* y_enc, const float* recip, const uint8_t* is_discrete,
                        int64_t k, const float* class_probs, int64_t n_classes, int n_jobs,
                        int64_t r_lo, int64_t r_hi, double* sums, const int* devices = nullptr,
                        int n_devices = 0) {
  if (!y_enc || !class_probs || n_classes < 1 || k < 0) {
    set_error("invalid ReliefF arguments (y_enc, class_probs, n_classes, k)");
    return FS_EINVAL;
  }
  if (!(0 <= r_lo && r_lo <= r_hi && r_hi <= n)) {
    set_error("row range must satisfy 0 <= row_begin <= row_end <= n");
    return FS_EINVAL;
  }
  int rc = check_backend(backend, device);
  if (rc != FS_OK) return rc;
  Prepared P;
  trace_mark("relieff: enter");
  rc = prepare(P, ALGO_RELIEFF, x, 0, n, p, nullptr, p, recip, is_discrete, n_jobs,
               backend == FS_BACKEND_GPU);
  trace_mark("prepare (host)");
  if (rc) return map_prep_rc(rc);
  P.labels.assign(y_enc, y_enc + n);
  for (int64_t i = 0; i < n; i++)
    if (P.labels[i] < 0 || P.labels[i] >= n_classes) {
      set_error("y_enc entry outside [0, n_classes)");
      return FS_EINVAL;
    }
  P.n_classes = (int32_t)n_classes;
  P.class_prior.assign(n_classes, 0.0);
  for (int64_t c = 0; c < n_classes; c++) P.class_prior[c] = (double)class_probs[c];
  P.k_neighbors = k;
  if ((rc = apply_accumulation(P)) != FS_OK) return rc;
  if (devices) {
    if ((rc = no_reference_devices()) != FS_OK) return rc;
    if (n_classes > 64) {
      set_error("GPU ReliefF supports at most 64 classes");
      return FS_ENOTSUP;
    }
    return gpu::rows_run_devices(P, x, devices, n_devices, r_lo, r_hi, sums);
  }
  if (backend == FS_BACKEND_GPU) return gpu::relieff_run(P, x, device, r_lo, r_hi, sums);
  return cpu::relieff_run(P, x, n_jobs, r_lo, r_hi, sums);
}

static int surf_sums(int backend, int device, const double* x, int64_t n, int64_t p,
                     const int32_t* y, const float* recip, int use_star,
                     const uint8_t* is_discrete, int n_jobs, int64_t r_lo, int64_t r_hi,
                     double* sums, const int* devices = nullptr, int n_devices = 0) {
  if (!(0 <= r_lo && r_lo <= r_hi && r_hi <= n)) {
    set_error("row range must satisfy 0 <= row_begin <= row_end <= n");
    return FS_EINVAL;
  }
  int rc = check_backend(backend, device);
  if (rc != FS_OK) return rc;
  Prepared P;
  trace_mark("surf: enter");
  rc = prepare(P, ALGO_SURF, x, 1, n, p, nullptr, p, recip, is_discrete, n_jobs,
               backend == FS_BACKEND_GPU);
  trace_mark("prepare (host)");
  if (rc) return map_prep_rc(rc);
  if (encode_labels_i32(P, y)) return FS_EINVAL;
  P.use_star = use_star ? 1 : 0;
  if ((rc = apply_accumulation(P)) != FS_OK) return rc;
  if (devices) {
    if ((rc = no_reference_devices()) != FS_OK) return rc;
    return gpu::rows_run_devices(P, x, devices, n_devices, r_lo, r_hi, sums);
  }
  if (backend == FS_BACKEND_GPU) return gpu::surf_run(P, x, device, r_lo, r_hi, sums);
  return cpu::surf_run(P, x, n_jobs, r_lo, r_hi, sums);
}

int fs_relieff_score(int backend, int device, const float* x, int64_t n, int64_t p,
                     const int32_t* y_enc, const float* recip, const uint8_t* is_discrete,
                     int64_t k, const float* class_probs, int64_t n_classes, int n_jobs,
                     float* scores_out) {
  if (!scores_out) {
    set_error("scores_out is NULL");
    return FS_EINVAL;
  }
  std::vector<double> S(p > 0 ? p : 1);
  const int rc = relieff_sums(backend, device, x, n, p, y_enc, recip, is_discrete, k,
                              class_probs, n_classes, n_jobs, 0, n, S.data());
  if (rc != FS_OK) return rc;
  for (int64_t f = 0; f < p; f++) scores_out[f] = (float)(S[f] / (double)n);
  return FS_OK;
}

int fs_relieff_score_rows(int backend, int device, const float* x, int64_t n, int64_t p,
                          const int32_t* y_enc, const float* recip, const uint8_t* is_discrete,
                          int64_t k, const float* class_probs, int64_t n_classes, int n_jobs,
                          int64_t row_begin, int64_t row_end, double* sums_out) {
  if (!sums_out) {
    set_error("sums_out is NULL");
    return FS_EINVAL;
  }
  return relieff_sums(backend, device, x, n, p, y_enc, recip, is_discrete, k, class_probs,
                      n_classes, n_jobs, row_begin, row_end, sums_out);
}

int fs_surf_score(int backend, int device, const double* x, int64_t n, int64_t p,
                  const int32_t* y, const float* recip, int use_star,
                  const uint8_t* is_discrete, int n_jobs, float* scores_out) {
  if (!scores_out) {
    set_error("scores_out is NULL");
    return FS_EINVAL;
  }
  std::vector<double> S(p > 0 ? p : 1);
  const int rc = surf_sums(backend, device, x, n, p, y, recip, use_star, is_discrete, n_jobs, 0,
                           n, S.data());
  if (rc != FS_OK) return rc;
  for (int64_t f = 0; f < p; f++) scores_out[f] = (float)(S[f] / (double)n);
  return FS_OK;
}

int fs_surf_score_rows(int backend, int device, const double* x, int64_t n, int64_t p,
                       const int32_t* y, const float* recip, int use_star,
                       const uint8_t* is_discrete, int n_jobs, int64_t row_begin,
                       int64_t row_end, double* sums_out) {
  if (!sums_out) {
    set_error("sums_out is NULL");
    return FS_EINVAL;
  }
  return surf_sums(backend, device, x, n, p, y, recip, use_star, is_discrete, n_jobs, row_begin,
                   row_end, sums_out);
}

int fs_multisurf_score_devices(const int* devices, int n_devices, const float* x, int64_t n,
                               int64_t p, const double* y, const float* recip,
                               const int64_t* feat_idx, int64_t n_kept, int use_star,
                               const uint8_t* is_discrete, int n_jobs, int64_t row_begin,
                               int64_t row_end, double* sums_out) {
  if (!sums_out) {
    set_error("sums_out is NULL");
    return FS_EINVAL;
  }
  if (!(0 <= row_begin && row_begin <= row_end && row_end <= n)) {
    set_error("row range must satisfy 0 <= row_begin <= row_end <= n");
    return FS_EINVAL;
  }
  int rc = check_devices(devices, n_devices);
  if (rc != FS_OK) return rc;
  Prepared P;
  rc = prepare(P, ALGO_MULTISURF, x, 0, n, p, feat_idx, n_kept, recip, is_discrete, n_jobs, true);
  if (rc) return map_prep_rc(rc);
  if (encode_labels_f64(P, y)) return FS_EINVAL;
  P.use_star = use_star ? 1 : 0;
  if ((rc = no_reference_devices()) != FS_OK) return rc;
  return gpu::multisurf_run_devices(P, x, devices, n_devices, row_begin, row_end, sums_out);
}

int fs_relieff_score_devices(const int* devices, int n_devices, const float* x, int64_t n,
                             int64_t p, const int32_t* y_enc, const float* recip,
                             const uint8_t* is_discrete, int64_t k, const float* class_probs,
                             int64_t n_classes, int n_jobs, int64_t row_begin, int64_t row_end,
                             double* sums_out) {
  if (!sums_out) {
    set_error("sums_out is NULL");
    return FS_EINVAL;
  }
  const int rc = check_devices(devices, n_devices);
  if (rc != FS_OK) return rc;
  return relieff_sums(FS_BACKEND_GPU, devices[0], x, n, p, y_enc, recip, is_discrete, k,
                      class_probs, n_classes, n_jobs, row_begin, row_end, sums_out, devices,
                      n_devices);
}

int fs_surf_score_devices(const int* devices, int n_devices, const double* x, int64_t n,
                          int64_t p, const int32_t* y, const float* recip, int use_star,
                          const uint8_t* is_discrete, int n_jobs, int64_t row_begin,
                          int64_t row_end, double* sums_out) {
  if (!sums_out) {
    set_error("sums_out is NULL");
    return FS_EINVAL;
  }
  const int rc = check_devices(devices, n_devices);
  if (rc != FS_OK) return rc;
  return surf_sums(FS_BACKEND_GPU, devices[0], x, n, p, y, recip, use_star, is_discrete, n_jobs,
                   row_begin, row_end, sums_out, devices, n_devices);
}

int fs_pair_screen(int backend, int device, const uint8_t* codes, const uint8_t* ycodes, int64_t n,
                   int64_t p, int n_states, int unit, int score_kind, int64_t n_top, int n_jobs,
                   double* relevance, double* top_score, int64_t* top_i, int64_t* top_j,
                   double* feature_best) {
  if (backend != FS_BACKEND_CPU && backend != FS_BACKEND_GPU) {
    set_error("backend must be FS_BACKEND_CPU or FS_BACKEND_GPU");
    return FS_EINVAL;
  }
  // the argument checks come before the device check, as in fs_jmi_select
  int rc = pair_check(backend, codes, ycodes, n, p, n_states, unit, score_kind, n_top, relevance,
                      top_score, top_i, top_j);
  if (rc != FS_OK) return rc;
  // so do the GPU backend's size and class limits
  if (backend == FS_BACKEND_GPU && (rc = gpu::pair_limits(ycodes, n, p, n_states)) != FS_OK)
    return rc;
  if ((rc = check_backend(backend, device)) != FS_OK) return rc;
  if (backend == FS_BACKEND_GPU)
    return gpu::pair_screen(device, codes, ycodes, n, p, n_states, unit, score_kind, (int)n_top,
                            relevance, top_score, top_i, top_j, feature_best);
  return cpu::pair_screen(codes, ycodes, n, p, n_states, unit, score_kind, (int)n_top, n_jobs,
                          relevance, top_score, top_i, top_j, feature_best);
}

int fs_pair_screen_last_timing(double* ms5) {
  if (!ms5) {
    set_error("fs_pair_screen_last_timing: NULL output");
    return FS_EINVAL;
  }
  gpu::pair_last_timing(ms5);
  return FS_OK;
}

int fs_pair_screen_labels(int backend, int device, const uint8_t* codes, const uint8_t* labels,
                          int n_labelings, int64_t n, int64_t p, int n_states, int unit,
                          int score_kind, int n_jobs, double* best_score, int64_t* best_i,
                          int64_t* best_j, double* relevance) {
  if (backend != FS_BACKEND_CPU && backend != FS_BACKEND_GPU) {
    set_error("backend must be FS_BACKEND_CPU or FS_BACKEND_GPU");
    return FS_EINVAL;
  }
  // the argument checks come before the device check, as in fs_pair_screen
  int rc = pair_labels_check(backend, codes, labels, n_labelings, n, p, n_states, unit,
                             score_kind, best_score, best_i, best_j);
  if (rc != FS_OK) return rc;
  // so do the GPU backend's size and class limits
  int classes = 0;
  if (backend == FS_BACKEND_GPU &&
      (rc = gpu::pair_labels_limits(labels, n_labelings, n, p, n_states, &classes)) != FS_OK)
    return rc;
  if ((rc = check_backend(backend, device)) != FS_OK) return rc;
  if (backend == FS_BACKEND_GPU)
    return gpu::pair_screen_labels(device, codes, labels, n_labelings, classes, n, p, n_states,
                                   unit, score_kind, best_score, best_i, best_j, relevance);
  return cpu::pair_screen_labels(codes, labels, n_labelings, n, p, n_states, unit, score_kind,
                                 n_jobs, best_score, best_i, best_j, relevance);
}

int fs_pair_labels_last_timing(double* ms5) {
  if (!ms5) {
    set_error("fs_pair_labels_last_timing: NULL output");
    return FS_EINVAL;
  }
  gpu::pair_labels_last_timing(ms5);
  return FS_OK;
}

}  // extern "C"

// The _ex one-shot calls: the accumulation mode is an argument, in force for
// that call only (the calling thread's fs_set_accumulation mode is restored
// on return, whatever it was).
namespace {
struct ScopedAccumulation {
  int prev;
  explicit ScopedAccumulation(int mode) : prev(g_accum) { g_accum = mode; }
  ~ScopedAccumulation() { g_accum = prev; }
};
int check_mode(int mode) {
  if (mode == FS_ACCUM_FAST || mode == FS_ACCUM_REFERENCE) return FS_OK;
  set_error("accumulation must be FS_ACCUM_FAST or FS_ACCUM_REFERENCE");
  return FS_EINVAL;
}
}  // namespace

extern "C" {

int fs_multisurf_score_ex(int backend, int device, const float* x, int64_t n, int64_t p,
                          const double* y, const float* recip, const int64_t* feat_idx,
                          int64_t n_kept, int use_star, const uint8_t* is_discrete, int n_jobs,
                          int accumulation, float* scores_out) {
  if (const int rc = check_mode(accumulation)) return rc;
  ScopedAccumulation mode(accumulation);
  return fs_multisurf_score(backend, device, x, n, p, y, recip, feat_idx, n_kept, use_star,
                            is_discrete, n_jobs, scores_out);
}

int fs_relieff_score_ex(int backend, int device, const float* x, int64_t n, int64_t p,
                        const int32_t* y_enc, const float* recip, const uint8_t* is_discrete,
                        int64_t k, const float* class_probs, int64_t n_classes, int n_jobs,
                        int accumulation, float* scores_out) {
  if (const int rc = check_mode(accumulation)) return rc;
  ScopedAccumulation mode(accumulation);
  return fs_relieff_score(backend, device, x, n, p, y_enc, recip, is_discrete, k, class_probs,
                          n_classes, n_jobs, scores_out);
}

int fs_surf_score_ex(int backend, int device, const double* x, int64_t n, int64_t p,
                     const int32_t* y, const float* recip, int use_star,
                     const uint8_t* is_discrete, int n_jobs, int accumulation,
                     float* scores_out) {
  if (const int rc = check_mode(accumulation)) return rc;
  ScopedAccumulation mode(accumulation);
  return fs_surf_score(backend, device, x, n, p, y, recip, use_star, is_discrete, n_jobs,
                       scores_out);
}

}  // extern "C"

// ---- sharded MultiSURF plan ------------------------------------------------

struct fs_plan {
  int backend = FS_BACKEND_CPU;
  int rank = 0, world = 1, n_jobs = -1;
  int x_is_f64 = 0;
  int64_t r_lo = 0, r_hi = 0;   // focal rows (MultiSURF: fs_plan_set_rows, else [0, n))
  // a fs_plan_select has run on the current shard, feature set and distances
  // (fs_plan_stir reads its decisions); pass1 and every re-targeting clear it
  bool selected = false;
  // labellings of the last completed fs_plan_relieff_score_labels on the CPU
  // backend (-1: none; the GPU plan keeps its own record)
  int64_t rf_labels_done = -1;
  // fs_plan_surf_labels_info of the last completed fs_plan_surf_score_labels
  // on the CPU backend ([0] < 0: none)
  int64_t surf_labels_info[4] = {-1, 0, 0, 0};
  Prepared P;
  Prepared P0;                  // as created (all columns): discrete tables for re-targeting
  gpu::Plan* g = nullptr;
  // CPU state
  std::vector<char> x;          // the CPU plan's copy of X (x_is_f64 ? double : float)
  cpu::CpuState st;
  const void* xp() const { return (const void*)x.data(); }
};

static bool is_multisurf_plan(const fs_plan* pl) {
  if (pl->P.algo == ALGO_MULTISURF) return true;
  set_error("pass1 / select / pass2 are the MultiSURF plan stages (use fs_plan_score)");
  return false;
}

extern "C" {

int fs_plan_create(fs_plan** plan_out, int backend, int device, const float* x, int64_t n,
                   int64_t p, const double* y, const float* recip, const int64_t* feat_idx,
                   int64_t n_kept, int use_star, const uint8_t* is_discrete, int rank, int world,
                   int n_jobs, uint64_t stream) {
  if (!plan_out) {
    set_error("plan_out is NULL");
    return FS_EINVAL;
  }
  *plan_out = nullptr;
  if (world < 1 || rank < 0 || rank >= world) {
    set_error("invalid rank/world");
    return FS_EINVAL;
  }
  int rc = check_backend(backend, device);
  if (rc != FS_OK) return rc;
  fs_plan* pl = new fs_plan();
  pl->backend = backend;
  pl->rank = rank;
  pl->world = world;
  pl->n_jobs = n_jobs;
  rc = prepare(pl->P, ALGO_MULTISURF, x, 0, n, p, feat_idx, n_kept, recip, is_discrete, n_jobs,
               backend == FS_BACKEND_GPU);
  if (rc || encode_labels_f64(pl->P, y)) {
    delete pl;
    return FS_EINVAL;
  }
  pl->P.use_star = use_star ? 1 : 0;
  if ((rc = apply_accumulation(pl->P)) != FS_OK) {
    delete pl;
    return rc;
  }
  if (pl->P.ref_accum && world > 1 && backend != FS_BACKEND_GPU) {
    delete pl;
    set_error("reference-order accumulation with world > 1 (fs_plan_ref_masks / "
              "fs_plan_ref_pass2) runs on the GPU backend only");
    return FS_ENOTSUP;
  }
  pl->r_lo = 0;
  pl->r_hi = n;
  if (backend == FS_BACKEND_GPU) {
    rc = gpu::plan_create(&pl->g, pl->P, x, 0, device, rank, world, stream);
    if (rc != FS_OK) {
      delete pl;
      return rc;
    }
  } else {
    const char* xb = (const char*)x;
    pl->x.assign(xb, xb + (size_t)n * p * sizeof(float));
  }
  *plan_out = pl;
  return FS_OK;
}

// ReliefF / SURF plans: prepared problem in pl->P, X uploaded (GPU) or copied
// (CPU), focal rows [r_lo, r_hi).
static int finish_rows_plan(fs_plan* pl, int device, const void* x, int64_t r_lo, int64_t r_hi,
                            uint64_t stream) {
  const Prepared& P = pl->P;
  if (pl->backend == FS_BACKEND_GPU && pl->x_is_f64) pl->P0 = P;  // value tables
  pl->r_lo = r_lo;
  pl->r_hi = r_hi;
  if (pl->backend == FS_BACKEND_GPU)
    return gpu::plan_create(&pl->g, P, x, pl->x_is_f64, device, 0, 1, stream, r_lo, r_hi);
  const char* xb = (const char*)x;
  pl->x.assign(xb, xb + (size_t)P.n * P.p_in * (pl->x_is_f64 ? 8 : 4));
  return FS_OK;
}

int fs_plan_create_relieff(fs_plan** plan_out, int backend, int device, const float* x,
                           int64_t n, int64_t p, const int32_t* y_enc, const float* recip,
                           const uint8_t* is_discrete, int64_t k, const float* class_probs,
                           int64_t n_classes, int64_t row_begin, int64_t row_end, int n_jobs,
                           uint64_t stream) {
  if (!plan_out || !y_enc || !class_probs || n_classes < 1 || k < 0) {
    set_error("invalid ReliefF plan arguments");
    return FS_EINVAL;
  }
  *plan_out = nullptr;
  if (!(0 <= row_begin && row_begin <= row_end && row_end <= n)) {
    set_error("row range must satisfy 0 <= row_begin <= row_end <= n");
    return FS_EINVAL;
  }
  int rc = check_backend(backend, device);
  if (rc != FS_OK) return rc;
  if (backend == FS_BACKEND_GPU && n_classes > 64) {
    set_error("GPU ReliefF supports at most 64 classes");
    return FS_ENOTSUP;
  }
  fs_plan* pl = new fs_plan();
  pl->backend = backend;
  pl->n_jobs = n_jobs;
  rc = prepare(pl->P, ALGO_RELIEFF, x, 0, n, p, nullptr, p, recip, is_discrete, n_jobs,
               backend == FS_BACKEND_GPU);
  if (rc) {
    delete pl;
    return map_prep_rc(rc);
  }
  pl->P.labels.assign(y_enc, y_enc + n);
  for (int64_t i = 0; i < n; i++)
    if (pl->P.labels[i] < 0 || pl->P.labels[i] >= n_classes) {
      delete pl;
      set_error("y_enc entry outside [0, n_classes)");
      return FS_EINVAL;
    }
  pl->P.n_classes = (int32_t)n_classes;
  pl->P.class_prior.assign(n_classes, 0.0);
  for (int64_t c = 0; c < n_classes; c++) pl->P.class_prior[c] = (double)class_probs[c];
  pl->P.k_neighbors = k;
  if ((rc = apply_accumulation(pl->P)) != FS_OK ||
      (rc = finish_rows_plan(pl, device, x, row_begin, row_end, stream)) != FS_OK) {
    delete pl;
    return rc;
  }
  *plan_out = pl;
  return FS_OK;
}

int fs_plan_create_surf(fs_plan** plan_out, int backend, int device, const double* x, int64_t n,
                        int64_t p, const int32_t* y, const float* recip, int use_star,
                        const uint8_t* is_discrete, int64_t row_begin, int64_t row_end,
                        int n_jobs, uint64_t stream) {
  if (!plan_out) {
    set_error("plan_out is NULL");
    return FS_EINVAL;
  }
  *plan_out = nullptr;
  if (!(0 <= row_begin && row_begin <= row_end && row_end <= n)) {
    set_error("row range must satisfy 0 <= row_begin <= row_end <= n");
    return FS_EINVAL;
  }
  int rc = check_backend(backend, device);
  if (rc != FS_OK) return rc;
  fs_plan* pl = new fs_plan();
  pl->backend = backend;
  pl->n_jobs = n_jobs;
  pl->x_is_f64 = 1;
  rc = prepare(pl->P, ALGO_SURF, x, 1, n, p, nullptr, p, recip, is_discrete, n_jobs,
               backend == FS_BACKEND_GPU);
  if (rc || encode_labels_i32(pl->P, y)) {
    delete pl;
    return FS_EINVAL;
  }
  pl->P.use_star = use_star ? 1 : 0;
  if ((rc = apply_accumulation(pl->P)) != FS_OK ||
      (rc = finish_rows_plan(pl, device, x, row_begin, row_end, stream)) != FS_OK) {
    delete pl;
    return rc;
  }
  *plan_out = pl;
  return FS_OK;
}

int fs_plan_score(fs_plan* pl, double* sums) {
  if (!pl || !sums) {
    set_error("NULL plan or buffer");
    return FS_EINVAL;
  }
  if (pl->P.algo == ALGO_MULTISURF) {
    set_error("fs_plan_score is for ReliefF / SURF plans (MultiSURF: pass1 / select / pass2)");
    return FS_EINVAL;
  }
  if (pl->g) return gpu::plan_score(pl->g, sums);
  if (pl->P.algo == ALGO_RELIEFF)
    return cpu::relieff_run(pl->P, pl->xp(), pl->n_jobs, pl->r_lo, pl->r_hi, sums);
  return cpu::surf_run(pl->P, pl->xp(), pl->n_jobs, pl->r_lo, pl->r_hi, sums);
}

int fs_plan_score_stir(fs_plan* pl, double* sums, double* stir_sums, double* pair_counts) {
  if (!pl || !sums || !stir_sums || !pair_counts) {
    set_error("fs_plan_score_stir: NULL plan or buffer");
    return FS_EINVAL;
  }
  if (pl->P.algo == ALGO_MULTISURF) {
    set_error("fs_plan_score_stir is for ReliefF plans (MultiSURF: pass1 / select, then "
              "fs_plan_stir)");
    return FS_EINVAL;
  }
  if (pl->P.algo != ALGO_RELIEFF) {
    set_error("fs_plan_score_stir: STIR is not built for SURF plans (ReliefF: this call, "
              "MultiSURF: fs_plan_stir)");
    return FS_ENOTSUP;
  }
  if (pl->g) return gpu::plan_score_stir(pl->g, sums, stir_sums, pair_counts);
  const int rc = cpu::relieff_run(pl->P, pl->xp(), pl->n_jobs, pl->r_lo, pl->r_hi, sums);
  if (rc != FS_OK) return rc;
  return cpu::relieff_stir(pl->P, (const float*)pl->xp(), pl->n_jobs, pl->r_lo, pl->r_hi,
                           stir_sums, pair_counts);
}

int fs_plan_set_features(fs_plan* pl, const int64_t* feat_idx, int64_t n_kept) {
  if (!pl) {
    set_error("plan is NULL");
    return FS_EINVAL;
  }
  const Prepared& O = pl->P;
  const bool gpu = pl->backend == FS_BACKEND_GPU;
  // the GPU plan keeps X and its column ranges on the device; the CPU plan
  // keeps its own copy of X
  const void* x = gpu ? nullptr : pl->xp();
  Prepared P;
  int rc = prepare(P, O.algo, x, pl->x_is_f64, O.n, O.p_in, feat_idx, n_kept, O.recip_in.data(),
                   O.disc_in.data(), pl->n_jobs, gpu, gpu ? &pl->P0 : nullptr);
  if (rc) return map_prep_rc(rc);
  P.labels = O.labels;
  P.n_classes = O.n_classes;
  P.class_prior = O.class_prior;
  P.use_star = O.use_star;
  P.k_neighbors = O.k_neighbors;
  P.ref_accum = O.ref_accum;  // the plan's mode, fixed at creation
  P.no_q16 = O.ref_accum && O.algo == ALGO_MULTISURF && !test_hooks().ref_q16 ? 1 : 0;
  pl->selected = false;
  if (gpu) {
    rc = gpu::plan_set_features(pl->g, P);
    if (rc != FS_OK) return rc;
  }
  pl->P = P;
  return FS_OK;
}

int fs_plan_pass1(fs_plan* pl, double* rowstats) {
  if (!pl || !rowstats) {
    set_error("NULL plan or buffer");
    return FS_EINVAL;
  }
  if (!is_multisurf_plan(pl)) return FS_EINVAL;
  pl->selected = false;  // the distances are written again, unrefined
  if (pl->g) return gpu::plan_pass1(pl->g, rowstats);
  return cpu::multisurf_pass1(pl->P, pl->xp(), pl->rank, pl->world, pl->n_jobs, pl->st,
                              rowstats);
}

int fs_plan_select(fs_plan* pl, const double* rowstats, double* counts) {
  if (!pl || !rowstats || !counts) {
    set_error("NULL plan or buffer");
    return FS_EINVAL;
  }
  if (!is_multisurf_plan(pl)) return FS_EINVAL;
  const int rc = pl->g ? gpu::plan_select(pl->g, rowstats, counts)
                       : cpu::multisurf_select(pl->P, pl->xp(), pl->rank, pl->world, rowstats,
                                               pl->n_jobs, pl->st, counts);
  pl->selected = rc == FS_OK;
  return rc;
}

int fs_plan_stir(fs_plan* pl, double* sums) {
  if (!pl || !sums) {
    set_error("NULL plan or buffer");
    return FS_EINVAL;
  }
  if (pl->P.algo != ALGO_MULTISURF) {
    set_error("fs_plan_stir: STIR is defined on MultiSURF plans (not ReliefF / SURF)");
    return FS_EINVAL;
  }
  if (pl->P.use_star) {
    set_error("fs_plan_stir: MultiSURF* has no STIR definition (its far misses are not pairs of "
              "the test)");
    return FS_ENOTSUP;
  }
  if (!pl->selected) {
    set_error("fs_plan_stir: no fs_plan_select on the plan's current shard and feature set "
              "(run pass1 and select after the last re-targeting)");
    return FS_EINVAL;
  }
  if (pl->g) return gpu::plan_stir(pl->g, sums);
  return cpu::multisurf_stir(pl->P, (const float*)pl->xp(), pl->st, pl->rank, pl->world,
                             pl->n_jobs, pl->r_lo, pl->r_hi, sums);
}

int fs_stir_statistics(const double* sums, int64_t n_kept, double n_hit_pairs,
                       double n_miss_pairs, double* hit_mean, double* miss_mean, double* t,
                       double* df) {
  return fs_stir_statistics_ex(sums, n_kept, n_hit_pairs, n_miss_pairs, hit_mean, miss_mean, t,
                               df, nullptr);
}

int fs_stir_statistics_ex(const double* sums, int64_t n_kept, double n_hit_pairs,
                          double n_miss_pairs, double* hit_mean, double* miss_mean, double* t,
                          double* df, double* pooled_sd) {
  if (n_kept < 0 || (n_kept > 0 && !sums)) {
    set_error("fs_stir_statistics: NULL sums or n_kept < 0");
    return FS_EINVAL;
  }
  if (!stir::statistics(sums, n_kept, n_hit_pairs, n_miss_pairs, hit_mean, miss_mean, t, df,
                        pooled_sd)) {
    set_error("fs_stir_statistics: fewer than 2 near-hit pairs or fewer than 2 near-miss pairs");
    return FS_EINVAL;
  }
  return FS_OK;
}

double fs_plan_stir_kernel_ms(const fs_plan* pl, int which) {
  if (!pl || !pl->g) return -1.0;
  return gpu::plan_stir_kernel_ms(pl->g, which);
}

int fs_plan_score_labels(fs_plan* pl, const int32_t* labels, int64_t B, double* scores) {
  if (!pl || B < 0 || (B > 0 && (!labels || !scores))) {
    set_error("fs_plan_score_labels: NULL plan or buffer, or B < 0");
    return FS_EINVAL;
  }
  if (pl->P.algo != ALGO_MULTISURF) {
    set_error("fs_plan_score_labels: a MultiSURF plan (ReliefF: fs_plan_relieff_score_labels; "
              "SURF: fs_plan_surf_score_labels)");
    return FS_EINVAL;
  }
  if (pl->P.use_star) {
    set_error("fs_plan_score_labels: MultiSURF* is not built (the star split's per-column "
              "terms read the labels)");
    return FS_ENOTSUP;
  }
  if (pl->P.ref_accum) {
    set_error("fs_plan_score_labels: not built for reference-order accumulation");
    return FS_ENOTSUP;
  }
  if (pl->world != 1 || pl->r_lo != 0 || pl->r_hi != pl->P.n) {
    set_error("fs_plan_score_labels: the plan must own every tile and focal row (world 1, no "
              "fs_plan_set_shard / fs_plan_set_rows): a labelling's counts would need an "
              "all-reduce of their own");
    return FS_ENOTSUP;
  }
  if (!pl->selected) {
    set_error("fs_plan_score_labels: no fs_plan_select on the plan's current shard and feature "
              "set (run pass1 and select after the last re-targeting)");
    return FS_EINVAL;
  }
  if (B == 0) return FS_OK;
  if (pl->g) return gpu::plan_score_labels(pl->g, labels, B, scores);
  return cpu::multisurf_score_labels(pl->P, pl->xp(), pl->st, labels, B, pl->n_jobs, scores);
}

double fs_plan_labels_kernel_ms(const fs_plan* pl, int which) {
  if (!pl || !pl->g) return -1.0;
  return gpu::plan_labels_kernel_ms(pl->g, which);
}

int fs_plan_relieff_score_labels(fs_plan* pl, const int32_t* labels, int64_t B, double* scores) {
  if (!pl || B < 0 || (B > 0 && (!labels || !scores))) {
    set_error("fs_plan_relieff_score_labels: NULL plan or buffer, or B < 0");
    return FS_EINVAL;
  }
  if (pl->P.algo != ALGO_RELIEFF) {
    set_error("fs_plan_relieff_score_labels: a ReliefF plan (MultiSURF: fs_plan_score_labels; "
              "SURF: fs_plan_surf_score_labels)");
    return FS_EINVAL;
  }
  if (pl->P.ref_accum) {
    set_error("fs_plan_relieff_score_labels: not built for reference-order accumulation");
    return FS_ENOTSUP;
  }
  if (pl->r_lo != 0 || pl->r_hi != pl->P.n) {
    set_error("fs_plan_relieff_score_labels: the plan must own every focal row [0, n)");
    return FS_ENOTSUP;
  }
  if (B == 0) return FS_OK;
  pl->rf_labels_done = -1;
  const int rc = pl->g ? gpu::plan_relieff_score_labels(pl->g, labels, B, scores)
                       : cpu::relieff_score_labels(pl->P, pl->xp(), labels, B, pl->n_jobs, scores);
  if (rc == FS_OK) pl->rf_labels_done = B;
  return rc;
}

int fs_relieff_score_labels(int backend, int device, const float* x, int64_t n, int64_t p,
                            const int32_t* labels, int64_t B, const float* recip,
                            const uint8_t* is_discrete, int64_t k, int n_jobs,
                            float* scores_out) {
  if (!scores_out || !labels || B < 1 || k < 0) {
    set_error("fs_relieff_score_labels: need labels, scores_out, B >= 1 and k >= 0");
    return FS_EINVAL;
  }
  int rc = check_backend(backend, device);
  if (rc != FS_OK) return rc;
  Prepared P;
  rc = prepare(P, ALGO_RELIEFF, x, 0, n, p, nullptr, p, recip, is_discrete, n_jobs,
               backend == FS_BACKEND_GPU);
  if (rc) return map_prep_rc(rc);
  P.k_neighbors = k;
  if (const int bad = relieff_set_labelling(P, labels)) {  // labelling 0 is the plan's y
    set_error(bad == 1 ? "fs_relieff_score_labels: labelling 0 holds a class code outside [0, 64)"
                       : "fs_relieff_score_labels: labelling 0 has fewer than 2 classes");
    return FS_EINVAL;
  }
  if ((rc = apply_accumulation(P)) != FS_OK) return rc;
  if (P.ref_accum) {
    set_error("fs_relieff_score_labels: not built for reference-order accumulation");
    return FS_ENOTSUP;
  }
  if (backend == FS_BACKEND_GPU)
    return gpu::relieff_labels_run(P, x, device, labels, B, scores_out);
  std::vector<double> S((size_t)B * P.n_kept);
  if ((rc = cpu::relieff_score_labels(P, x, labels, B, n_jobs, S.data())) != FS_OK) return rc;
  for (int64_t q = 0; q < B * P.n_kept; q++) scores_out[q] = (float)(S[q] / (double)n);
  return FS_OK;
}

int fs_plan_relieff_labels_info(const fs_plan* pl, int64_t out[4]) {
  if (!pl || !out) {
    set_error("fs_plan_relieff_labels_info: NULL plan or buffer");
    return FS_EINVAL;
  }
  if (pl->g) return gpu::plan_relieff_labels_info(pl->g, out);
  if (pl->rf_labels_done < 0) {
    set_error("fs_plan_relieff_labels_info: no completed fs_plan_relieff_score_labels call");
    return FS_EINVAL;
  }
  out[0] = 0, out[1] = pl->rf_labels_done, out[2] = 0, out[3] = 0;
  return FS_OK;
}

double fs_plan_relieff_labels_kernel_ms(const fs_plan* pl, int which) {
  if (!pl || !pl->g) return -1.0;
  return gpu::plan_relieff_labels_kernel_ms(pl->g, which);
}

int fs_plan_surf_score_labels(fs_plan* pl, const int32_t* labels, int64_t B, double* scores) {
  if (!pl || B < 0 || (B > 0 && (!labels || !scores))) {
    set_error("fs_plan_surf_score_labels: NULL plan or buffer, or B < 0");
    return FS_EINVAL;
  }
  if (pl->P.algo != ALGO_SURF) {
    set_error("fs_plan_surf_score_labels: a SURF plan (MultiSURF: fs_plan_score_labels; ReliefF: "
              "fs_plan_relieff_score_labels)");
    return FS_EINVAL;
  }
  if (pl->P.ref_accum) {
    set_error("fs_plan_surf_score_labels: not built for reference-order accumulation");
    return FS_ENOTSUP;
  }
  if (pl->world != 1 || pl->r_lo != 0 || pl->r_hi != pl->P.n) {
    set_error("fs_plan_surf_score_labels: the plan must own every focal row [0, n) (world 1)");
    return FS_ENOTSUP;
  }
  if (B == 0) return FS_OK;
  pl->surf_labels_info[0] = -1;
  if (pl->g) return gpu::plan_surf_score_labels(pl->g, labels, B, scores);
  int64_t info[4];
  const int rc = cpu::surf_score_labels(pl->P, pl->xp(), labels, B, pl->n_jobs, scores, info);
  if (rc == FS_OK) std::copy(info, info + 4, pl->surf_labels_info);
  return rc;
}

int fs_surf_score_labels(int backend, int device, const double* x, int64_t n, int64_t p,
                         const int32_t* labels, int64_t B, const float* recip,
                         const uint8_t* is_discrete, int use_star, int n_jobs,
                         float* scores_out) {
  if (!scores_out || !labels || B < 1) {
    set_error("fs_surf_score_labels: need labels, scores_out and B >= 1");
    return FS_EINVAL;
  }
  int rc = check_backend(backend, device);
  if (rc != FS_OK) return rc;
  Prepared P;
  rc = prepare(P, ALGO_SURF, x, 1, n, p, nullptr, p, recip, is_discrete, n_jobs,
               backend == FS_BACKEND_GPU);
  if (rc) return map_prep_rc(rc);
  if (encode_labels_i32(P, labels)) return FS_EINVAL;  // labelling 0 is the plan's y
  P.use_star = use_star ? 1 : 0;
  if ((rc = apply_accumulation(P)) != FS_OK) return rc;
  if (P.ref_accum) {
    set_error("fs_surf_score_labels: not built for reference-order accumulation");
    return FS_ENOTSUP;
  }
  if (backend == FS_BACKEND_GPU) return gpu::surf_labels_run(P, x, device, labels, B, scores_out);
  std::vector<double> S((size_t)B * P.n_kept);
  if ((rc = cpu::surf_score_labels(P, x, labels, B, n_jobs, S.data())) != FS_OK) return rc;
  for (int64_t q = 0; q < B * P.n_kept; q++) scores_out[q] = (float)(S[q] / (double)n);
  return FS_OK;
}

int fs_plan_surf_labels_info(const fs_plan* pl, int64_t out[4]) {
  if (!pl || !out) {
    set_error("fs_plan_surf_labels_info: NULL plan or buffer");
    return FS_EINVAL;
  }
  if (pl->g) return gpu::plan_surf_labels_info(pl->g, out);
  if (pl->surf_labels_info[0] < 0) {
    set_error("fs_plan_surf_labels_info: no completed fs_plan_surf_score_labels call");
    return FS_EINVAL;
  }
  std::copy(pl->surf_labels_info, pl->surf_labels_info + 4, out);
  return FS_OK;
}

double fs_plan_surf_labels_kernel_ms(const fs_plan* pl, int which) {
  if (!pl || !pl->g) return -1.0;
  return gpu::plan_surf_labels_kernel_ms(pl->g, which);
}

// ---- RReliefF (fs_rrelieff.h) ------------------------------------------------

int fs_plan_score_targets(fs_plan* pl, const double* targets, int64_t B, double* s_a,
                          double* s_ca, double* s_c) {
  if (!pl || !targets || !s_a || !s_ca || !s_c) {
    set_error("fs_plan_score_targets: NULL plan or buffer");
    return FS_EINVAL;
  }
  if (B < 1) {
    set_error("fs_plan_score_targets: B < 1");
    return FS_EINVAL;
  }
  if (pl->P.algo != ALGO_RELIEFF) {
    set_error("fs_plan_score_targets: a ReliefF plan with one class (not a SURF or MultiSURF "
              "plan)");
    return FS_EINVAL;
  }
  if (pl->P.n_classes != 1) {
    set_error("fs_plan_score_targets: the plan has more than one class (RReliefF's neighbours "
              "are the k nearest of all: create the plan with n_classes = 1)");
    return FS_EINVAL;
  }
  if (pl->P.ref_accum) {
    set_error("fs_plan_score_targets: not built for reference-order accumulation");
    return FS_EINVAL;
  }
  if (pl->P.k_neighbors < 1 || pl->P.k_neighbors > pl->P.n - 1) {
    set_error("fs_plan_score_targets: k must satisfy 1 <= k <= n - 1");
    return FS_EINVAL;
  }
  std::vector<double> u;
  if (const int64_t bad = rrelieff::scale_targets(targets, B, pl->P.n, u); bad >= 0) {
    set_error("fs_plan_score_targets: target " + std::to_string(bad) +
              " holds a non-finite value");
    return FS_EINVAL;
  }
  if (pl->g) return gpu::plan_score_targets(pl->g, u.data(), B, s_a, s_ca, s_c);
  return cpu::rrelieff_sums(pl->P, (const float*)pl->xp(), pl->n_jobs, pl->r_lo, pl->r_hi,
                            u.data(), B, s_a, s_ca, s_c);
}

int fs_rrelieff_scores(const double* s_a, const double* s_ca_row, double s_c, double n_pairs,
                       int64_t n_kept, float* scores) {
  if (n_kept < 0 || (n_kept > 0 && (!s_a || !s_ca_row || !scores))) {
    set_error("fs_rrelieff_scores: NULL buffer or n_kept < 0");
    return FS_EINVAL;
  }
  rrelieff::scores(s_a, s_ca_row, s_c, n_pairs, n_kept, scores);
  return FS_OK;
}

int fs_rrelieff_score(int backend, int device, const float* x, int64_t n, int64_t p,
                      const double* targets, int64_t B, const float* recip,
                      const uint8_t* is_discrete, int64_t k, int n_jobs, float* scores_out) {
  if (!scores_out || !targets || B < 1) {
    set_error("fs_rrelieff_score: need targets, scores_out and B >= 1");
    return FS_EINVAL;
  }
  if (k < 1 || k > n - 1) {
    set_error("fs_rrelieff_score: k must satisfy 1 <= k <= n - 1");
    return FS_EINVAL;
  }
  int rc = check_backend(backend, device);
  if (rc != FS_OK) return rc;
  Prepared P;
  rc = prepare(P, ALGO_RELIEFF, x, 0, n, p, nullptr, p, recip, is_discrete, n_jobs,
               backend == FS_BACKEND_GPU);
  if (rc) return map_prep_rc(rc);
  P.labels.assign((size_t)n, 0);
  P.n_classes = 1;
  P.class_prior.assign(1, 1.0);
  P.k_neighbors = k;
  // fast accumulation whatever the process-wide mode: P.ref_accum stays 0
  std::vector<double> u;
  if (const int64_t bad = rrelieff::scale_targets(targets, B, n, u); bad >= 0) {
    set_error("fs_rrelieff_score: target " + std::to_string(bad) + " holds a non-finite value");
    return FS_EINVAL;
  }
  if (backend == FS_BACKEND_GPU) return gpu::rrelieff_run(P, x, device, u.data(), B, scores_out);
  const int64_t nk = P.n_kept;
  std::vector<double> sa((size_t)nk), sca((size_t)(B * nk)), sc((size_t)B);
  if ((rc = cpu::rrelieff_sums(P, x, n_jobs, 0, n, u.data(), B, sa.data(), sca.data(),
                               sc.data())) != FS_OK)
    return rc;
  for (int64_t b = 0; b < B; b++)
    rrelieff::scores(sa.data(), sca.data() + b * nk, sc[b], (double)n * (double)k, nk,
                     scores_out + b * nk);
  return FS_OK;
}

double fs_plan_targets_kernel_ms(const fs_plan* pl, int which) {
  if (!pl || !pl->g) return -1.0;
  return gpu::plan_targets_kernel_ms(pl->g, which);
}

int fs_plan_pass2(fs_plan* pl, const double* counts, double* scores) {
  if (!pl || !counts || !scores) {
    set_error("NULL plan or buffer");
    return FS_EINVAL;
  }
  if (!is_multisurf_plan(pl)) return FS_EINVAL;
  if (pl->g) return gpu::plan_pass2(pl->g, counts, scores);
  return cpu::multisurf_pass2(pl->P, pl->xp(), pl->st, counts, pl->rank, pl->world, pl->n_jobs,
                              pl->r_lo, pl->r_hi, scores);
}

int fs_plan_ref_mask_words(fs_plan* pl, int64_t* words) {
  if (!pl || !words) {
    set_error("NULL plan or buffer");
    return FS_EINVAL;
  }
  if (!is_multisurf_plan(pl)) return FS_EINVAL;
  if (!pl->g || !pl->P.ref_accum) {
    set_error("fs_plan_ref_mask_words: a GPU plan created in reference-order accumulation");
    return FS_ENOTSUP;
  }
  *words = gpu::ref_mask_words(pl->g);
  return FS_OK;
}

int fs_plan_ref_masks(fs_plan* pl, uint64_t* masks, int64_t words) {
  int64_t need = 0;
  int rc = fs_plan_ref_mask_words(pl, &need);
  if (rc) return rc;
  if (!masks || words < need) {
    set_error("fs_plan_ref_masks: mask buffer NULL or smaller than fs_plan_ref_mask_words");
    return FS_EINVAL;
  }
  return gpu::plan_ref_masks(pl->g, masks);
}

int fs_plan_ref_pass2(fs_plan* pl, const uint64_t* masks, const double* counts, int64_t row_begin,
                      int64_t row_end) {
  int64_t need = 0;
  int rc = fs_plan_ref_mask_words(pl, &need);
  if (rc) return rc;
  if (!masks || !counts) {
    set_error("NULL plan or buffer");
    return FS_EINVAL;
  }
  if (!(0 <= row_begin && row_begin <= row_end && row_end <= pl->P.n)) {
    set_error("fs_plan_ref_pass2: row range outside [0, n)");
    return FS_EINVAL;
  }
  return gpu::plan_ref_pass2(pl->g, masks, counts, row_begin, row_end);
}

// GPU plans in reference order: fs_plan_ref_temp takes the row plans
// (ReliefF, SURF), fs_plan_ref_sums every kind
static int ref_rows_plan(fs_plan* pl, bool rows_only, const char* what) {
  if (!pl) {
    set_error("plan is NULL");
    return FS_EINVAL;
  }
  if (rows_only && pl->P.algo == ALGO_MULTISURF) {
    set_error(std::string(what) + ": a ReliefF or SURF plan");
    return FS_EINVAL;
  }
  if (!pl->g || !pl->P.ref_accum) {
    set_error(std::string(what) + ": a GPU plan created in reference-order accumulation");
    return FS_ENOTSUP;
  }
  return FS_OK;
}

int fs_plan_ref_temp(fs_plan* pl) {
  const int rc = ref_rows_plan(pl, true, "fs_plan_ref_temp");
  return rc ? rc : gpu::plan_ref_temp(pl->g);
}

int fs_plan_ref_sums(fs_plan* pl, const double* init, double* sums) {
  const int rc = ref_rows_plan(pl, false, "fs_plan_ref_sums");
  if (rc) return rc;
  if (!sums) {
    set_error("NULL sums buffer");
    return FS_EINVAL;
  }
  return gpu::plan_ref_sums(pl->g, init, sums);
}

int fs_plan_decision_guard(fs_plan* pl, const double* rowstats, const double* counts,
                           const double* scores, double* risk_out, int* switched_out) {
  if (!pl || !rowstats || !counts || !scores || !risk_out || !switched_out) {
    set_error("NULL plan or buffer");
    return FS_EINVAL;
  }
  if (!is_multisurf_plan(pl)) return FS_EINVAL;
  *risk_out = -1.0;
  *switched_out = 0;
  // the CPU backend always runs pass 1 on 32-bit operands
  if (!pl->g) return FS_OK;
  const int rc = gpu::plan_decision_guard(pl->g, rowstats, counts, scores, risk_out, switched_out);
  if (rc != FS_OK || *switched_out) pl->selected = false;  // a new layout: the step runs again
  return rc;
}

int fs_plan_set_rows(fs_plan* pl, int64_t row_begin, int64_t row_end) {
  if (!pl) {
    set_error("plan is NULL");
    return FS_EINVAL;
  }
  if (!is_multisurf_plan(pl)) return FS_EINVAL;
  if (!(0 <= row_begin && row_begin <= row_end && row_end <= pl->P.n)) {
    set_error("row range must satisfy 0 <= row_begin <= row_end <= n");
    return FS_EINVAL;
  }
  if (pl->g) {
    const int rc = gpu::plan_set_rows(pl->g, row_begin, row_end);
    if (rc != FS_OK) return rc;
  }
  pl->r_lo = row_begin;
  pl->r_hi = row_end;
  return FS_OK;
}

int fs_plan_set_shard(fs_plan* pl, int rank, int world) {
  if (!pl) {
    set_error("plan is NULL");
    return FS_EINVAL;
  }
  if (!is_multisurf_plan(pl)) return FS_EINVAL;
  if (world < 1 || rank < 0 || rank >= world) {
    set_error("shard rank/world must satisfy 0 <= rank < world");
    return FS_EINVAL;
  }
  if (pl->P.ref_accum && world > 1 && !pl->g) {
    set_error("reference-order accumulation with world > 1 (fs_plan_ref_masks / "
              "fs_plan_ref_pass2) runs on the GPU backend only");
    return FS_ENOTSUP;
  }
  pl->selected = false;
  if (pl->g) {
    const int rc = gpu::plan_set_shard(pl->g, rank, world);
    if (rc != FS_OK) return rc;
  }
  pl->rank = rank;
  pl->world = world;
  return FS_OK;
}

int fs_multisurf_shards(int device, int64_t n, int64_t p, int world, int* shards) {
  if (!shards || n < 2 || p < 1 || world < 1) {
    set_error("fs_multisurf_shards: need shards, n >= 2, p >= 1, world >= 1");
    return FS_EINVAL;
  }
  *shards = 1;
  if (test_hooks().shards >= 1) {
    *shards = (int)std::min<int64_t>(test_hooks().shards, 4096);
    return FS_OK;
  }
  if (gpu::device_count() <= 0) return FS_OK;
  Prepared P;
  P.n = n;
  P.n_pad = (n + kTile - 1) / kTile * kTile;
  P.PW = (p + kFeatPad - 1) / kFeatPad * kFeatPad;
  *shards = gpu::multisurf_shards(P, device, world);
  return FS_OK;
}

int fs_plan_info(const fs_plan* pl, int64_t* owned_tiles_out, double* pfe,
                 int64_t* refined_rows) {
  if (!pl) {
    set_error("NULL plan");
    return FS_EINVAL;
  }
  if (pl->g) return gpu::plan_info(pl->g, owned_tiles_out, pfe, refined_rows);
  if (refined_rows) *refined_rows = pl->st.refined;
  std::vector<int32_t> bi, bj;
  owned_tiles(pl->P.n_pad / kTile, pl->rank, pl->world, bi, bj);
  if (owned_tiles_out) *owned_tiles_out = (int64_t)bi.size();
  if (pfe) *pfe = 2.0 * (double)bi.size() * kTile * kTile * (double)(pl->P.pc + pl->P.pd);
  return FS_OK;
}

int fs_plan_calibration_ex(const fs_plan* pl, double* out, int n_out) {
  if (!pl || !out || n_out < 0) {
    set_error("NULL plan or output, or n_out < 0");
    return FS_EINVAL;
  }
  double v[8] = {0.0, 0.0, 0.0, std::sqrt((double)pl->P.pc / 6.0 + 1.0), 1.0, 0.0, 0.0, pl->P.SC};
  if (pl->g) {
    const int rc = gpu::plan_calibration(pl->g, v);
    if (rc != FS_OK) return rc;
  }
  const int m = n_out < 8 ? n_out : 8;
  for (int k = 0; k < m; k++) out[k] = v[k];
  return m;
}

// The six values documented since the first release (writing
// out[6] / out[7] through the old signature overran double[6] callers).
int fs_plan_calibration(const fs_plan* pl, double* out) {
  const int rc = fs_plan_calibration_ex(pl, out, 6);
  return rc < 0 ? rc : FS_OK;
}

int fs_plan_weighted_pairs(const fs_plan* pl, int64_t* pairs) {
  if (!pl || !pairs) {
    set_error("NULL plan or output");
    return FS_EINVAL;
  }
  *pairs = -1;
  if (pl->g) return gpu::plan_weighted_pairs(pl->g, pairs);
  return FS_OK;
}

int fs_plan_star_split(const fs_plan* pl, int* split) {
  if (!pl || !split) {
    set_error("NULL plan or output");
    return FS_EINVAL;
  }
  *split = pl->g ? gpu::plan_star_split(pl->g) : 0;  // the CPU backend weighs every pair
  return FS_OK;
}

int fs_plan_set_star_split(fs_plan* pl, int split) {
  if (!pl) {
    set_error("plan is NULL");
    return FS_EINVAL;
  }
  if (pl->g) {
    const int rc = gpu::plan_set_star_split(pl->g, split);
    // a new layout: fs_plan_stir / fs_plan_score_labels need a select on it
    pl->selected = false;
    return rc;
  }
  if (split) {
    set_error("fs_plan_set_star_split: the CPU backend has no star split");
    return FS_EINVAL;
  }
  return FS_OK;
}

double fs_plan_kernel_ms(const fs_plan* pl, int which) {
  if (!pl || !pl->g) return -1.0;
  return gpu::plan_kernel_ms(pl->g, which);
}

int fs_plan_destroy(fs_plan* pl) {
  if (!pl) return FS_OK;
  if (pl->g) gpu::plan_destroy(pl->g);
  delete pl;
  return FS_OK;
}

int fs_mdr_scan(int backend, int device, const uint8_t* x, int64_t n, int64_t p,
                const uint8_t* is_case, int k, const int32_t* fold, int n_folds, int n_jobs,
                float* best_ba, int64_t* best_rank, float* ba_out) {
  int rc = check_backend(backend, device);
  if (rc != FS_OK) return rc;
  int64_t count = 0;
  if ((rc = mdr_check(x, n, p, is_case, k, fold, n_folds, best_ba, best_rank, &count)) != FS_OK)
    return rc;
  if (backend == FS_BACKEND_GPU)
    return gpu::mdr_scan(device, x, n, p, is_case, k, fold, n_folds, count, best_ba, best_rank,
                         ba_out);
  return cpu::mdr_scan(x, n, p, is_case, k, fold, n_folds, n_jobs, count, best_ba, best_rank,
                       ba_out);
}

int fs_mdr_scan_labels(int backend, int device, const uint8_t* x, int64_t n, int64_t p,
                       const uint8_t* labels, int n_labelings, int k, const int32_t* fold,
                       int n_folds, int n_jobs, float* best_ba, int64_t* best_rank, float* ba_out) {
  int rc = check_backend(backend, device);
  if (rc != FS_OK) return rc;
  int64_t count = 0;
  if ((rc = mdr_check_labels(x, n, p, labels, n_labelings, k, fold, n_folds, best_ba, best_rank,
                             &count)) != FS_OK)
    return rc;
  if (backend == FS_BACKEND_GPU)
    return gpu::mdr_scan_labels(device, x, n, p, labels, n_labelings, k, fold, n_folds, count,
                                best_ba, best_rank, ba_out);
  return cpu::mdr_scan_labels(x, n, p, labels, n_labelings, k, fold, n_folds, n_jobs, count,
                              best_ba, best_rank, ba_out);
}

int fs_mdr_labels_last_timing(double* ms4) {
  if (!ms4) {
    set_error("fs_mdr_labels_last_timing: NULL output");
    return FS_EINVAL;
  }
  gpu::mdr_labels_last_timing(ms4);
  return FS_OK;
}

int fs_mdr_scan_top(int backend, int device, const uint8_t* x, int64_t n, int64_t p,
                    const uint8_t* is_case, int k, const int32_t* fold, int n_folds, int n_top,
                    int n_jobs, float* top_ba, int64_t* top_rank) {
  int rc = check_backend(backend, device);
  if (rc != FS_OK) return rc;
  int64_t count = 0;
  if ((rc = mdr_check(x, n, p, is_case, k, fold, n_folds, top_ba, top_rank, &count)) != FS_OK)
    return rc;
  if (n_top < 1 || n_top > kMdrMaxTop) {
    set_error("fs_mdr_scan_top: n_top must be in 1.." + std::to_string(kMdrMaxTop));
    return FS_EINVAL;
  }
  if (backend == FS_BACKEND_GPU)
    return gpu::mdr_scan_top(device, x, n, p, is_case, k, fold, n_folds, count, n_top, top_ba,
                             top_rank);
  return cpu::mdr_scan_top(x, n, p, is_case, k, fold, n_folds, n_jobs, count, n_top, top_ba,
                           top_rank);
}

int fs_mdr_top_last_timing(double* ms4) {
  if (!ms4) {
    set_error("fs_mdr_top_last_timing: NULL output");
    return FS_EINVAL;
  }
  gpu::mdr_top_last_timing(ms4);
  return FS_OK;
}

int fs_mdr_combinations(int64_t p, int k, int64_t* count) {
  if (!count || k < 1 || k > kMdrMaxK || p < k) {
    set_error("fs_mdr_combinations: need count, k in 1..6 and p >= k");
    return FS_EINVAL;
  }
  if (!mdr_count(p, k, count)) {
    set_error("fs_mdr_combinations: C(p,k) exceeds 2^62");
    return FS_EINVAL;
  }
  return FS_OK;
}

int fs_mdr_unrank(int64_t p, int k, int64_t rank, int32_t* features) {
  int64_t count = 0;
  if (!features || k < 1 || k > kMdrMaxK || p < k || !mdr_count(p, k, &count) || rank < 0 ||
      rank >= count) {
    set_error("fs_mdr_unrank: need features, k in 1..6, p >= k and rank in [0, C(p,k))");
    return FS_EINVAL;
  }
  mdr_unrank(p, k, rank, features);
  return FS_OK;
}

int fs_mi_matrices(int backend, int device, const uint8_t* codes, const uint8_t* ycodes, int64_t n,
                   int64_t p, int n_states, int unit, int n_jobs, double* relevance,
                   double* redundancy, int32_t* counts_out) {
  if (backend != FS_BACKEND_CPU && backend != FS_BACKEND_GPU) {
    set_error("backend must be FS_BACKEND_CPU or FS_BACKEND_GPU");
    return FS_EINVAL;
  }
  // the argument checks come before the device check: both backends reject
  // the same calls the same way, with or without a device
  int rc = mi_check(backend, codes, ycodes, n, p, n_states, unit, relevance);
  if (rc != FS_OK) return rc;
  if ((rc = check_backend(backend, device)) != FS_OK) return rc;
  if (backend == FS_BACKEND_GPU)
    return gpu::mi_matrices(device, codes, ycodes, n, p, n_states, unit, relevance, redundancy,
                            counts_out);
  return cpu::mi_matrices(codes, ycodes, n, p, n_states, unit, n_jobs, relevance, redundancy,
                          counts_out);
}

int fs_mi_last_timing(double* ms4) {
  if (!ms4) {
    set_error("fs_mi_last_timing: NULL output");
    return FS_EINVAL;
  }
  gpu::mi_last_timing(ms4);
  return FS_OK;
}

int fs_cfs_create(fs_cfs** out, int backend, int device, const uint8_t* codes,
                  const uint8_t* ycodes, int64_t n, int64_t p, int n_states, int n_jobs) {
  if (backend != FS_BACKEND_CPU && backend != FS_BACKEND_GPU) {
    set_error("backend must be FS_BACKEND_CPU or FS_BACKEND_GPU");
    return FS_EINVAL;
  }
  // the argument checks come before the device check, as in fs_mi_matrices
  int rc = cfs_check(backend, out, codes, ycodes, n, p, n_states);
  if (rc != FS_OK) return rc;
  *out = nullptr;
  if ((rc = check_backend(backend, device)) != FS_OK) return rc;
  if (backend == FS_BACKEND_GPU) return gpu::cfs_create(out, device, codes, ycodes, n, p, n_states);
  return cpu::cfs_create(out, codes, ycodes, n, p, n_states, n_jobs);
}

int fs_cfs_relevance(fs_cfs* h, float* r_cf) {
  if (!h || !r_cf) {
    set_error("fs_cfs_relevance: NULL argument");
    return FS_EINVAL;
  }
  return h->relevance(r_cf);
}

int fs_cfs_search(fs_cfs* h, double min_r_cf, int64_t* selected, int64_t* n_selected,
                  double* merits) {
  if (!h || !selected || !n_selected || !merits) {
    set_error("fs_cfs_search: NULL argument");
    return FS_EINVAL;
  }
  return h->search(min_r_cf, selected, n_selected, merits);
}

int fs_cfs_row(fs_cfs* h, int64_t feature, float* row) {
  if (!h || !row) {
    set_error("fs_cfs_row: NULL argument");
    return FS_EINVAL;
  }
  if (feature < 0 || feature >= h->p) {
    set_error("fs_cfs_row: feature must be in [0, p)");
    return FS_EINVAL;
  }
  return h->row(feature, row);
}

int fs_cfs_search_matrix(int backend, int device, const float* r_cf, const float* r_ff, int64_t p,
                         double min_r_cf, int64_t* selected, int64_t* n_selected,
                         double* merits) {
  if (backend != FS_BACKEND_CPU && backend != FS_BACKEND_GPU) {
    set_error("backend must be FS_BACKEND_CPU or FS_BACKEND_GPU");
    return FS_EINVAL;
  }
  int rc = cfs_check_matrix(r_cf, r_ff, p, selected, n_selected, merits);
  if (rc != FS_OK) return rc;
  if ((rc = check_backend(backend, device)) != FS_OK) return rc;
  if (backend == FS_BACKEND_GPU)
    return gpu::cfs_search_matrix(device, r_cf, r_ff, p, min_r_cf, selected, n_selected, merits);
  return cpu::cfs_search_matrix(r_cf, r_ff, p, min_r_cf, -1, selected, n_selected, merits);
}

int fs_cfs_last_timing(double* ms5) {
  if (!ms5) {
    set_error("fs_cfs_last_timing: NULL output");
    return FS_EINVAL;
  }
  gpu::cfs_last_timing(ms5);
  return FS_OK;
}

int fs_cfs_destroy(fs_cfs* h) {
  delete h;
  return FS_OK;
}

int fs_mrmr_select(int backend, int device, const uint8_t* codes, const uint8_t* ycodes, int64_t n,
                   int64_t p, int n_states, int unit, int method, int64_t k, int n_jobs,
                   double* relevance, int64_t* selected, double* rows) {
  if (backend != FS_BACKEND_CPU && backend != FS_BACKEND_GPU) {
    set_error("backend must be FS_BACKEND_CPU or FS_BACKEND_GPU");
    return FS_EINVAL;
  }
  // the argument checks come before the device check, as in fs_mi_matrices
  int rc = mrmr_check(backend, codes, ycodes, n, p, n_states, unit, method, k, relevance, selected);
  if (rc != FS_OK) return rc;
  if ((rc = check_backend(backend, device)) != FS_OK) return rc;
  if (backend == FS_BACKEND_GPU)
    return gpu::mrmr_select(device, codes, ycodes, n, p, n_states, unit, method, k, relevance,
                            selected, rows);
  return cpu::mrmr_select(codes, ycodes, n, p, n_states, unit, method, k, n_jobs, relevance,
                          selected, rows);
}

int fs_mrmr_search_matrix(int backend, int device, const double* relevance,
                          const double* redundancy, int64_t p, int method, int64_t k,
                          int64_t* selected) {
  if (backend != FS_BACKEND_CPU && backend != FS_BACKEND_GPU) {
    set_error("backend must be FS_BACKEND_CPU or FS_BACKEND_GPU");
    return FS_EINVAL;
  }
  int rc = mrmr_check_matrix(relevance, redundancy, p, method, k, selected);
  if (rc != FS_OK) return rc;
  if ((rc = check_backend(backend, device)) != FS_OK) return rc;
  if (backend == FS_BACKEND_GPU)
    return gpu::mrmr_search_matrix(device, relevance, redundancy, p, method, k, selected);
  return cpu::mrmr_search_matrix(relevance, redundancy, p, method, k, selected);
}

int fs_mrmr_last_timing(double* ms5) {
  if (!ms5) {
    set_error("fs_mrmr_last_timing: NULL output");
    return FS_EINVAL;
  }
  gpu::mrmr_last_timing(ms5);
  return FS_OK;
}

int fs_jmi_select(int backend, int device, const uint8_t* codes, const uint8_t* ycodes, int64_t n,
                  int64_t p, int n_states, int unit, int method, int64_t k, int n_jobs,
                  double* relevance, int64_t* selected, double* rows) {
  if (backend != FS_BACKEND_CPU && backend != FS_BACKEND_GPU) {
    set_error("backend must be FS_BACKEND_CPU or FS_BACKEND_GPU");
    return FS_EINVAL;
  }
  // the argument checks come before the device check, as in fs_mi_matrices
  int rc = jmi_check_select(backend, codes, ycodes, n, p, n_states, unit, method, k, relevance,
                            selected);
  if (rc != FS_OK) return rc;
  if ((rc = check_backend(backend, device)) != FS_OK) return rc;
  if (backend == FS_BACKEND_GPU)
    return gpu::jmi_select(device, codes, ycodes, n, p, n_states, unit, method, k, relevance,
                           selected, rows);
  return cpu::jmi_select(codes, ycodes, n, p, n_states, unit, method, k, n_jobs, relevance,
                         selected, rows);
}

int fs_jmi_rows(int backend, int device, const uint8_t* codes, const uint8_t* ycodes, int64_t n,
                int64_t p, int n_states, int unit, const int64_t* anchors, int64_t m, int n_jobs,
                double* rows) {
  if (backend != FS_BACKEND_CPU && backend != FS_BACKEND_GPU) {
    set_error("backend must be FS_BACKEND_CPU or FS_BACKEND_GPU");
    return FS_EINVAL;
  }
  int rc = jmi_check_rows(backend, codes, ycodes, n, p, n_states, unit, anchors, m, rows);
  if (rc != FS_OK) return rc;
  if ((rc = check_backend(backend, device)) != FS_OK) return rc;
  if (backend == FS_BACKEND_GPU)
    return gpu::jmi_rows(device, codes, ycodes, n, p, n_states, unit, anchors, m, rows);
  return cpu::jmi_rows(codes, ycodes, n, p, n_states, unit, anchors, m, n_jobs, rows);
}

int fs_jmi_search_matrix(int backend, int device, const double* relevance, const double* joint,
                         int64_t p, int method, int64_t k, int64_t* selected) {
  if (backend != FS_BACKEND_CPU && backend != FS_BACKEND_GPU) {
    set_error("backend must be FS_BACKEND_CPU or FS_BACKEND_GPU");
    return FS_EINVAL;
  }
  int rc = jmi_check_matrix(relevance, joint, p, method, k, selected);
  if (rc != FS_OK) return rc;
  if ((rc = check_backend(backend, device)) != FS_OK) return rc;
  if (backend == FS_BACKEND_GPU)
    return gpu::jmi_search_matrix(device, relevance, joint, p, method, k, selected);
  return cpu::jmi_search_matrix(relevance, joint, p, method, k, selected);
}

int fs_jmi_last_timing(double* ms5) {
  if (!ms5) {
    set_error("fs_jmi_last_timing: NULL output");
    return FS_EINVAL;
  }
  gpu::jmi_last_timing(ms5);
  return FS_OK;
}

}  // extern "C"
