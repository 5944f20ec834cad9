// fs_mrmr.h -- what the two backends of fs_mrmr_* (fs_mrmr_cpu.cpp,
// fs_mrmr.hip) share: the float64 expressions of the mRMR greedy loop
// (the reference's mRMR.py:96-117), the argument checks and the host side of
// one step.
//
// Selection-only mRMR: after argmax(relevance) every step reads the running
// sum of the selected features' redundancy rows, picks one feature and adds
// that feature's row to the sum.  So a fit needs the relevance and k rows of
// mutual information, k p pairs instead of p^2 / 2, and the p x p matrix never
// exists.  The rows themselves come from fs_mi.h.
//
// Everything here is plain IEEE float64 in the reference's operation order;
// the build has -ffp-contract=off and no fast-math, so the CPU backend, the
// GPU backend and numpy agree bit for bit on a step given the same inputs.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/fastselect_amd.h"
#include "fs_internal.h"
#include "fs_mi.h"

namespace fs {

constexpr int kMrmrMid = 0, kMrmrMiq = 1;

// redundancy_sum[f] / i (mRMR.py:105, 107, 111), i >= 1 converted to double.
// Step 0 has no selected feature: every candidate's mean redundancy is 0.0,
// which leaves the lowest index among equals (np.argmax, mRMR.py:98).
FS_HD inline double mrmr_avg(int64_t i, double rsum) { return i == 0 ? 0.0 : rsum / (double)i; }
// The score of candidate f at step i (mRMR.py:104-107); step 0 is the
// relevance itself (mRMR.py:98).
FS_HD inline double mrmr_score(int method, int64_t i, double rel, double rsum) {
  if (i == 0) return rel;
  const double avg = rsum / (double)i;
  return method == kMrmrMid ? rel - avg : rel / (avg + 1e-9);
}
// f is a top candidate: np.isclose(scores, max, atol=1e-12) with numpy's
// default rtol = 1e-5 (mRMR.py:109), |score - max| <= atol + rtol * |max|.
// Scores are always finite here (a relevance and a mean of finitely many
// mutual informations; the MIQ denominator is >= about 1e-9 - k * 1e-12 > 0),
// so isclose's clauses for infinities and NaN never apply.  Step 0 is
// np.argmax: only the maximum itself.
FS_HD inline bool mrmr_is_top(int64_t i, double score, double mx) {
  if (i == 0) return score == mx;
  return fabs(score - mx) <= 1e-12 + 1e-5 * fabs(mx);
}
// The order of two top candidates (mean redundancy, index): the lower mean,
// the lower index among equal means; index < 0 is "none".  This is
// top[np.argmin(avg)] (mRMR.py:110-112), and with one candidate that candidate
// (mRMR.py:114), so one rule serves both.
FS_HD inline bool mrmr_beats(double aa, int64_t ia, double ab, int64_t ib) {
  if (ia < 0) return false;
  if (ib < 0) return true;
  return aa < ab || (aa == ab && ia < ib);
}

// One step on the host, serial: the feature step i selects among the
// features with taken[f] == 0 (-1: none is left).
inline int64_t mrmr_pick(int method, int64_t i, const double* rel, const double* rsum,
                         const uint8_t* taken, int64_t p) {
  double mx = -HUGE_VAL;
  for (int64_t f = 0; f < p; f++)
    if (!taken[f]) {
      const double s = mrmr_score(method, i, rel[f], rsum[f]);
      if (s > mx) mx = s;
    }
  double ba = 0.0;
  int64_t bi = -1;
  for (int64_t f = 0; f < p; f++)
    if (!taken[f] && mrmr_is_top(i, mrmr_score(method, i, rel[f], rsum[f]), mx)) {
      const double a = mrmr_avg(i, rsum[f]);
      if (mrmr_beats(a, f, ba, bi)) ba = a, bi = f;
    }
  return bi;
}

// Argument checks shared by both backends (the codes themselves are checked
// while they are packed): mi_check's, then k, method and selected.
int mrmr_check(int backend, const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p,
               int n_states, int unit, int method, int64_t k, const double* relevance,
               const int64_t* selected);
int mrmr_check_matrix(const double* relevance, const double* redundancy, int64_t p, int method,
                      int64_t k, const int64_t* selected);

namespace cpu {
int mrmr_select(const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p, int n_states,
                int unit, int method, int64_t k, int n_jobs, double* relevance,
                int64_t* selected, double* rows);
int mrmr_search_matrix(const double* relevance, const double* redundancy, int64_t p, int method,
                       int64_t k, int64_t* selected);
}
namespace gpu {
int mrmr_select(int device, const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p,
                int n_states, int unit, int method, int64_t k, double* relevance,
                int64_t* selected, double* rows);
int mrmr_search_matrix(int device, const double* relevance, const double* redundancy, int64_t p,
                       int method, int64_t k, int64_t* selected);
// Milliseconds of the calling thread's last GPU mrmr_select: upload, pack,
// relevance, rows, steps (HIP events on the call's stream).
void mrmr_last_timing(double* ms5);
}

}  // namespace fs
