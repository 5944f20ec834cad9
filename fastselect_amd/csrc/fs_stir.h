// fs_stir.h -- STIR: t-statistics for MultiSURF and ReliefF scores.  This header is the
// specification (there is no reference implementation) and holds the host
// epilogue both backends' callers share.
//
// Method: "STatistical Inference Relief", Le, Urbanowicz, Moore and McKinney,
// Bioinformatics 35(8), 2019, for the MultiSURF neighbourhood.
//
// Definitions.  diff_a(i, j) is the reference's per-feature diff
// (MultiSURF.py:184-187, 222-225): x_i != x_j for a discrete feature,
// |x_i - x_j| * recip_a for a continuous one.  N_i is MultiSURF's near set of
// focal sample i: the samples j != i with dist(i, j) < mu_i - sigma_i / 2 --
// the plan's own decisions, the ones its pass 2 weighs.  H is the multiset of
// ordered pairs (i, j) with j in N_i and y_j == y_i, M the same with
// y_j != y_i; a pair that is near from both sides counts twice.  Per feature:
//
//   S1H = sum over H of diff_a      S2H = sum over H of diff_a^2
//   S1M = sum over M of diff_a      S2M = sum over M of diff_a^2
//   Hbar = S1H / |H|                Mbar = S1M / |M|
//   vH = (S2H - |H| Hbar^2) / (|H| - 1), clamped at 0; vM likewise
//   sp = sqrt(((|M| - 1) vM + (|H| - 1) vH) / (|M| + |H| - 2))
//   t_a = (Mbar - Hbar) / (sp * sqrt(1/|M| + 1/|H|))
//   df = |M| + |H| - 2
//   p_a = P(T_df >= t_a), one-sided (taken by the caller)
//
// all in float64.  |H| is the sum of counts[2i] and |M| of counts[2i + 1]
// over the focal rows in use.  Where sp == 0, t is +inf, -inf or 0 by the
// sign of Mbar - Hbar (p = 0, 1, 1).  |H| < 2 or |M| < 2 has no statistic.
//
// What the statistic is: a pooled two-sample t-test that treats the |H| + |M|
// pairs as independent draws.  They are not -- every sample occurs in many
// pairs -- so the p-values are the published method's approximation and are
// not calibrated on noise features.
//
// fs_plan_stir returns the four sums of one plan's pairs as
// sums[q * n_kept + k], q = 0..3 for S1H, S2H, S1M, S2M, k in feat_idx order:
// partial sums, additive over (rank, world) plans, tile shards and disjoint
// focal-row ranges.  The GPU stage is fs_stir.hip, the CPU one fs_stir_cpu.cpp.
//
// Error of the GPU sums.  The CPU backend sums the float32 diffs themselves.
// The GPU puts every continuous term on a fixed-point grid before it sums
// exactly (fs_stir.hip): a diff on a grid of K1 2^-23, a squared diff on a
// grid of K2 2^-23, K1 and K2 the odd powers of two above the plan's largest
// scaled range Rmax = max over the continuous features of (max - min) * recip
// and above Rmax^2.  The bound is therefore absolute, in units of the plan's
// Rmax, not relative to the term as float32 rounding is: each diff is within
// K1 2^-24 (1.2e-7 at Rmax = 1) and each square within K2 2^-24, rounded to
// nearest.  With the estimators' recip = 1 / range every feature's scaled
// range is 1 and the grid is 2.4e-7 of that range.  A caller's own recip that
// gives the columns different scaled ranges puts every column on the grid of
// the largest one: a column whose scaled range is r carries a relative grid
// of K1 2^-23 / r.  Squares below K2 2^-24 round to 0: a feature whose near
// pairs' diffs all lie below about 3.5e-4 of the range (sqrt(1.2e-7); say one
// far outlier that no near pair includes) gets S2H = S2M = 0, so vH = vM = 0,
// sp = 0 and t = +inf, -inf or 0, where the exact sums give a finite t.
// The sums S1 keep their absolute bound there.
//
// STIR for ReliefF (fs_plan_score_stir).  The published STIR is defined on
// ReliefF's k nearest hits and k nearest misses; the MultiSURF form above is
// the paper's extension.
//
// Neighbour sets.  For a focal sample i of the plan's row range [r_lo, r_hi),
// L_i[c] is the plan's neighbour list of class c: the min(k, members of c
// other than i) nearest samples of class c by the reference's float32 key
// (ReliefF.py:145-155), ties at the k-th key resolved in numba's argsort
// order (ReliefF.py:157-175) -- the very lists the score weighs.  The
// reference counts the focal sample itself as a zero-diff hit in h_found when
// its class has fewer than k other members; that self entry is NOT a pair of
// the test.
//
// H is the set of ordered pairs (i, j) with j in L_i[y_i], M the set of
// ordered pairs (i, j) with j in L_i[c] for any c != y_i.  M is pooled and
// unweighted: the class-prior weights of the score do not enter.  For two
// classes this is the published STIR, |H| = |M| = n k when both classes have
// more than k members; for more classes it is a pooled generalisation, this
// project's choice.  diff_a, S1H, S2H, S1M, S2M and the epilogue are those
// above (stir::statistics, fs_stir_statistics unchanged), with
//
//   |H| = sum over the focal rows of |L_i[y_i]|
//   |M| = sum over the focal rows and the classes c != y_i of |L_i[c]|
//
// A pair belongs to its focal sample only: row ranges, row panels, devices
// and ranks partition the pairs and never cut one, so the four sums and both
// counts add up over disjoint focal-row ranges.  That is why the GPU stage
// (fs_stir_relieff.hip, k_rf_stir) sums in float64 rather than on the
// fixed-point grid: regroupings agree to 1e-12, and the terms are |a - b| of
// the float32 operands xs (each rounded once, ~6e-8 of the feature's range),
// widened to float64 before they are summed or squared.  The CPU stage
// (cpu::relieff_stir) sums the reference's float32 diffs widened to float64.
#pragma once

#include <cmath>
#include <cstdint>

#include "fs_internal.h"

namespace fs {
namespace stir {

// The epilogue above for n_kept features; pooled_sd receives sp (a caller
// tells the sp == 0 cases of t by it).  Any output may be null.  Returns false
// (nothing written) when |H| < 2 or |M| < 2.
inline bool statistics(const double* sums, int64_t n_kept, double nH, double nM, double* hit_mean,
                       double* miss_mean, double* t, double* df, double* pooled_sd = nullptr) {
  if (!(nH >= 2.0) || !(nM >= 2.0)) return false;
  const double dof = nM + nH - 2.0;
  const double scale = std::sqrt(1.0 / nM + 1.0 / nH);
  for (int64_t k = 0; k < n_kept; k++) {
    const double hbar = sums[k] / nH, mbar = sums[2 * n_kept + k] / nM;
    double vh = (sums[n_kept + k] - nH * hbar * hbar) / (nH - 1.0);
    double vm = (sums[3 * n_kept + k] - nM * mbar * mbar) / (nM - 1.0);
    if (!(vh > 0.0)) vh = 0.0;
    if (!(vm > 0.0)) vm = 0.0;
    const double sp = std::sqrt(((nM - 1.0) * vm + (nH - 1.0) * vh) / dof);
    const double d = mbar - hbar;
    if (hit_mean) hit_mean[k] = hbar;
    if (miss_mean) miss_mean[k] = mbar;
    if (pooled_sd) pooled_sd[k] = sp;
    if (t) t[k] = sp == 0.0 ? (d > 0.0 ? HUGE_VAL : (d < 0.0 ? -HUGE_VAL : 0.0)) : d / (sp * scale);
  }
  if (df) *df = dof;
  return true;
}

}  // namespace stir

namespace cpu {
// The four sums of the plan's near pairs (fs_stir_cpu.cpp): the decisions of
// S (the CPU plan's pass 2 reads the same D and thr), the pair sides of the
// focal samples [r_lo, r_hi) in the pairs (rank, world) owns, diffs in the
// reference's float32 arithmetic, float64 sums over a fixed partition of the
// focal rows (the same bits for every n_jobs).  x: the plan's float32 X.
int multisurf_stir(const Prepared& P, const float* x, const CpuState& S, int rank, int world,
                   int n_jobs, int64_t r_lo, int64_t r_hi, double* sums);
// ReliefF's neighbour lists of the focal rows [r_lo, r_hi) (fs_cpu.cpp):
// lists[(i - r_lo) * n_classes + c] = L_i[c], selected as relieff_run selects
// them (relieff_select_row on the same distances and band).
void relieff_neighbours(const Prepared& P, const void* x, int n_jobs, int64_t r_lo, int64_t r_hi,
                        std::vector<std::vector<int32_t>>& lists);
// STIR for ReliefF (above): stir_sums[4 n_kept] and pair_counts[2] = |H|, |M|
// of the focal rows [r_lo, r_hi).  Diffs in the reference's float32
// arithmetic widened to float64, float64 sums over a partition of the focal
// rows that depends on the row range alone (the same bits for every n_jobs).
// x: the plan's float32 X.
int relieff_stir(const Prepared& P, const float* x, int n_jobs, int64_t r_lo, int64_t r_hi,
                 double* stir_sums, double* pair_counts);
}  // namespace cpu

}  // namespace fs
