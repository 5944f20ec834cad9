// fs_rrelieff.h -- RReliefF: Relief for continuous targets.  This header is
// the specification (there is no reference implementation) and holds the
// host parts both backends share: the scaled targets and the epilogue.
//
// Method: Robnik-Sikonja and Kononenko, "An adaptation of Relief for
// attribute estimation in regression" (ICML 1997); "Theoretical and empirical
// analysis of ReliefF and RReliefF", Machine Learning 53 (2003).
//
// Neighbours.  For a focal sample i of the plan's row range [r_lo, r_hi), N_i
// is the set of its k nearest other samples: exactly the list a ReliefF plan
// with ONE class selects -- the reference's float32 keys (ReliefF.py:145-155),
// numba's quicksort order among equal keys at the k-th place
// (ReliefF.py:157-175), 1 <= k <= n - 1, never the self-hit.  N_i does not
// read the target.  d_f(i, j) is the plan's diff: |x_if - x_jf| / range_f for
// a continuous feature, a mismatch (0 / 1) for a discrete one.
//
// Target.  For a target t (float64, finite):
//   range  = max t - min t
//   u_i    = t_i / range     (one float64 division per sample, on the host;
//                             u = 0 everywhere when range == 0)
//   dy(i, j) = |u_i - u_j|   in float64
//
// Raw sums over the ordered pairs (i, j in N_i) of the focal rows, float64:
//   S_A[f]  = sum d_f            (does not depend on the target)
//   S_CA[f] = sum dy * d_f
//   S_C     = sum dy
//   M       = rows * k           (the number of pairs)
//
//   W[f] = S_CA[f] / S_C - (S_A[f] - S_CA[f]) / (M - S_C)
//
// in float64, rounded to float32 once.  Every neighbour has weight 1 / k,
// which cancels out of both quotients.  W = 0 for every f when S_C == 0 (a
// constant target) or S_C == M.  The paper's rank-weighted neighbours
// (exp(-(rank / sigma)^2)) are not built: in fast accumulation the plan's
// lists are not in rank order.
//
// A pair belongs to its focal sample only, so S_A, S_CA and S_C add up over
// disjoint focal-row ranges (M too); u is scaled by the whole target's range
// whatever the row range.
//
// Order and bits.  A feature's accumulation order is (row, list position)
// whatever the number of targets in the call: row b of a call with B targets
// has the bits of the B = 1 call of target b, and S_A has the same bits for
// any B.  No float atomics: a repeated call gives the same bits.
//
// The GPU stage is fs_rrelieff.hip (k_rrf_update, k_rrf_sc), the CPU stage
// fs_rrelieff_cpu.cpp.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "fs_internal.h"

namespace fs {
namespace rrelieff {

// u[b * n + i] of the B targets t[b * n + i] (above).  Returns the index of
// the first target with a non-finite entry, or -1 (u complete).
inline int64_t scale_targets(const double* t, int64_t B, int64_t n, std::vector<double>& u) {
  u.assign((size_t)(B * n), 0.0);
  for (int64_t b = 0; b < B; b++) {
    const double* tb = t + b * n;
    double lo = HUGE_VAL, hi = -HUGE_VAL;
    for (int64_t i = 0; i < n; i++) {
      if (!std::isfinite(tb[i])) return b;
      lo = tb[i] < lo ? tb[i] : lo;
      hi = tb[i] > hi ? tb[i] : hi;
    }
    const double range = n > 0 ? hi - lo : 0.0;
    if (!(range > 0.0)) continue;
    double* ub = u.data() + b * n;
    for (int64_t i = 0; i < n; i++) ub[i] = tb[i] / range;
  }
  return -1;
}

// The epilogue above: scores[f] of one target from S_A, its row of S_CA and
// its S_C.
inline void scores(const double* s_a, const double* s_ca, double s_c, double n_pairs,
                   int64_t n_kept, float* out) {
  const bool none = s_c == 0.0 || s_c == n_pairs;
  for (int64_t f = 0; f < n_kept; f++)
    out[f] = none ? 0.0f : (float)(s_ca[f] / s_c - (s_a[f] - s_ca[f]) / (n_pairs - s_c));
}

}  // namespace rrelieff

namespace cpu {
// The sums above of the focal rows [r_lo, r_hi) for the B scaled targets
// u[B][n] (fs_rrelieff_cpu.cpp): the lists of relieff_neighbours on the
// one-class P, diffs in the reference's float32 arithmetic widened to
// float64, float64 sums over a partition of the focal rows that depends on
// the row range alone (the same bits for every n_jobs).  x: the plan's
// float32 X.  s_a[n_kept], s_ca[B][n_kept], s_c[B].
int rrelieff_sums(const Prepared& P, const float* x, int n_jobs, int64_t r_lo, int64_t r_hi,
                  const double* u, int64_t B, double* s_a, double* s_ca, double* s_c);
}  // namespace cpu

namespace gpu {
// The same sums of a one-class ReliefF plan's focal rows into device memory
// (fs_rrelieff.hip): pass 1 and the selection once per call, k_rrf_update per
// chunk of up to 8 targets.  u: host memory, [B][n].
// plan_targets_kernel_ms: the last call's selection (0) and update-kernel (1)
// time, the latter summed over the chunks; -1 when unavailable.
int plan_score_targets(Plan* g, const double* u, int64_t B, double* s_a_dev, double* s_ca_dev,
                       double* s_c_dev);
double plan_targets_kernel_ms(const Plan* g, int which);
// One call from host arrays: a one-class plan over every row and column,
// the sums, then the epilogue; scores_out[B][n_kept].
int rrelieff_run(const Prepared& P, const void* x, int device, const double* u, int64_t B,
                 float* scores_out);
}  // namespace gpu

}  // namespace fs
