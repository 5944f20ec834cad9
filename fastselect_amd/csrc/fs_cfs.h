// fs_cfs.h -- what the two backends of fs_cfs_* (fs_cfs_cpu.cpp, fs_cfs.hip)
// share: the float64 expressions of symmetrical uncertainty on one pair's
// integer contingency table, the CFS merit, one candidate's merit in the
// reference's summation order, the search driver and the argument checks.
//
// Correlation-based feature selection (the reference's CFS.py): SU(x, y) =
// 2 I(x; y) / (H(x) + H(y)) stored as float32, and a best-first search over
// subsets by merit.  The search reads r_cf[p] and one row of SU per selected
// feature, so rows are computed when the search selects their feature and the
// p x p matrix never exists.
//
// Typing follows compiled numba (CFS.py:26-77): the float32 counts divided by
// the int64 n are float64, and so is everything after until the float32 store.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/fastselect_amd.h"
#include "fs_internal.h"
#include "fs_mi.h"

namespace fs {

constexpr int kCfsMaxStates = kMiMaxStates;        // codes are bytes
constexpr int kCfsMaxStatesGpu = kMiMaxStatesGpu;  // CFS.py:349

// ---- symmetrical uncertainty (CFS.py:26-77) --------------------------------
// The table is tab[a * ld + b], a < k1 states of the column with the lower
// index (it supplies the rows, CFS.py:96-102; the target counts as column p),
// b < k2.  The steps are functions of their own so that the GPU kernel can
// spread a pair's cells over lanes: a cell or state the reference skips
// contributes a term of exactly 0.0, and h - 0.0 == h, mi + 0.0 == mi for
// every value these sums reach (neither becomes -0.0), so running over every
// cell in index order gives the bits of the skipping loops.  States a column
// never takes add exact zeros too, so k = max code + 1 serves as the state
// count.  The build has -ffp-contract=off and no fast-math.
FS_HD inline double cfs_pxy(int32_t count, double dn) { return (double)count / dn; }
// _entropy (CFS.py:26-41): entropy -= prob * log2(prob) over prob > 1e-12,
// prob = (marginal count) / n
FS_HD inline double cfs_h_term(double prob) { return prob > 1e-12 ? prob * log2(prob) : 0.0; }
FS_HD inline double cfs_entropy(const int32_t* cnt, int k, double dn) {
  double h = 0.0;
  for (int s = 0; s < k; s++) h -= cfs_h_term(cfs_pxy(cnt[s], dn));
  return h;
}
// _mutual_information (CFS.py:44-64): px / py are the row / column sums of pxy
// in index order from 0.0; no eps in the denominator (unlike fs_mi.h)
FS_HD inline double cfs_mi_term(double pxy, double px, double py) {
  const double eps = 1e-12;
  return (pxy > eps && px > eps && py > eps) ? pxy * log2(pxy / (px * py)) : 0.0;
}
// _symmetrical_uncertainty (CFS.py:67-77) and the float32 store (CFS.py:88-102)
FS_HD inline float cfs_su(double mi, double hx, double hy) {
  const double hs = hx + hy;
  return hs < 1e-12 ? 0.0f : (float)(2.0 * mi / hs);
}
// py: k2 doubles of workspace
FS_HD inline double cfs_mi_from_table(const int32_t* tab, int ld, int k1, int k2, int64_t n,
                                      double* py) {
  const double dn = (double)n;
  for (int b = 0; b < k2; b++) py[b] = 0.0;
  for (int a = 0; a < k1; a++)
    for (int b = 0; b < k2; b++) py[b] += cfs_pxy(tab[a * ld + b], dn);
  double mi = 0.0;
  for (int a = 0; a < k1; a++) {
    double px = 0.0;
    for (int b = 0; b < k2; b++) px += cfs_pxy(tab[a * ld + b], dn);
    for (int b = 0; b < k2; b++) mi += cfs_mi_term(cfs_pxy(tab[a * ld + b], dn), px, py[b]);
  }
  return mi;
}

// ---- merit and one search step (CFS.py:11-23, 115-162) ---------------------
// _cfs_merit as written, k an integer: every product of k's is exact in
// float64 for any k this library can reach.
FS_HD inline double cfs_merit(double sum_r_cf, int64_t k, double sum_r_ff) {
  if (k == 0) return 0.0;
  const double dk = (double)k;
  const double kk1 = (double)(k * (k - 1));
  const double r_cf_avg = sum_r_cf / dk;
  const double r_ff_avg = k > 1 ? (2.0 * sum_r_ff) / kk1 : 0.0;
  const double denom = sqrt(dk + kk1 * r_ff_avg);
  return denom > 1e-12 ? (dk * r_cf_avg / denom) : 0.0;
}
// Feature i is scanned by a step (CFS.py:128).
FS_HD inline bool cfs_is_candidate(const uint8_t* taken, const float* r_cf, double min_r_cf,
                                   int64_t i) {
  return !taken[i] && !((double)r_cf[i] < min_r_cf);
}
// The merit of selected + [i] (CFS.py:132-150): base_cf / base_ff are the
// sums over the k selected features and their pairs, which every candidate of
// a step starts from; then r_cf[i], then r_ff[i, s] for s in selection order,
// read from the selected features' rows: rows[rowof[s] * stride + i].
FS_HD inline double cfs_candidate_merit(double base_cf, double base_ff, const float* r_cf,
                                        const float* rows, const int64_t* rowof, int64_t stride,
                                        int64_t k, int64_t i) {
  const double sum_r_cf = base_cf + (double)r_cf[i];
  double sum_r_ff = base_ff;
  for (int64_t s = 0; s < k; s++) sum_r_ff += (double)rows[rowof[s] * stride + i];
  return cfs_merit(sum_r_cf, k + 1, sum_r_ff);
}
// The order of two (merit, index) results: the higher merit, the lower index
// among equals.  "No candidate" is (the current merit, -1): it wins every tie,
// which is the reference's strict merit > best_merit, and among candidates the
// lowest index wins as in the reference's ascending scan.
FS_HD inline bool cfs_beats(double ma, int64_t ia, double mb, int64_t ib) {
  return ma > mb || (ma == mb && ia < ib);
}

// ---- the search driver -----------------------------------------------------
// What a backend adds to cfs_search_drive: the scan of one step.
struct CfsStepper {
  virtual ~CfsStepper() {}
  // `first` is selected: mark it and make its row available as row 0
  virtual int begin(int64_t first) = 0;
  // k features are selected.  *best_i = the lowest-index candidate of the
  // highest merit if that merit exceeds `current`, else -1.  When accepted,
  // the backend has marked best_i, made its row available as row k, and
  // entries[s] = r_ff[best_i, selected[s]] for s < k.
  virtual int step(int64_t k, double base_cf, double base_ff, double current, int64_t* best_i,
                   double* best_merit, float* entries) = 0;
};
// _best_first_search (CFS.py:115-162).  selected[p] in selection order,
// merits[s] = the merit after s + 1 features.
int cfs_search_drive(CfsStepper& st, const float* r_cf, int64_t p, double min_r_cf,
                     int64_t* selected, int64_t* n_selected, double* merits);

// Argument checks shared by both backends (the codes themselves are checked
// while they are packed).
int cfs_check(int backend, const void* out, const uint8_t* codes, const uint8_t* ycodes, int64_t n,
              int64_t p, int n_states);
int cfs_check_matrix(const float* r_cf, const float* r_ff, int64_t p, const int64_t* selected,
                     const int64_t* n_selected, const double* merits);

namespace cpu {
int cfs_create(fs_cfs** out, const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p,
               int n_states, int n_jobs);
int cfs_search_matrix(const float* r_cf, const float* r_ff, int64_t p, double min_r_cf,
                      int n_jobs, int64_t* selected, int64_t* n_selected, double* merits);
}
namespace gpu {
int cfs_create(fs_cfs** out, int device, const uint8_t* codes, const uint8_t* ycodes, int64_t n,
               int64_t p, int n_states);
int cfs_search_matrix(int device, const float* r_cf, const float* r_ff, int64_t p,
                      double min_r_cf, int64_t* selected, int64_t* n_selected, double* merits);
// Milliseconds of the calling thread's last GPU handle: upload, pack,
// relevance, rows, steps (HIP events on the handle's stream; the last two
// grow with every fs_cfs_search / fs_cfs_row).
void cfs_last_timing(double* ms5);
}

}  // namespace fs

// The handle behind the C ABI: one per backend.
struct fs_cfs {
  int64_t n = 0, p = 0;
  virtual ~fs_cfs() {}
  virtual int relevance(float* r_cf) = 0;
  virtual int row(int64_t feature, float* out) = 0;
  virtual int search(double min_r_cf, int64_t* selected, int64_t* n_selected, double* merits) = 0;
};
