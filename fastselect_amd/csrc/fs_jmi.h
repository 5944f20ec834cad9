// fs_jmi.h -- what the two backends of fs_jmi_* (fs_jmi_cpu.cpp, fs_jmi.hip)
// share: the definition of a pair's joint relevance, the float64 expressions
// of the JMI and CMIM greedy loops, the argument checks and the host side of
// one step.
//
// Joint relevance.  For two columns lo < hi, T[(a * kcol[hi] + b)][c] counts
// the samples with x_lo = a, x_hi = b, y = c, and
//   J(lo, hi) = mi_from_table(T, ld, kcol[lo] * kcol[hi], kcol[y], n, unit)
// (fs_mi.h, unchanged): the joint column supplies the rows, y the columns, the
// marginals are summed in index order, the terms row-major, mi_constant and
// mi_finish as there.  A state that never occurs adds exact zeros, so a kernel
// may index the rows as a * SP + b; J(lo, hi) is, bit for bit on the same
// backend, the relevance fs_mi_matrices gives the column z = x_lo * K + x_hi
// (K >= kcol[hi]).  J(f, f) = 0.0.  rel[f] = I(X_f; y) is the relevance of
// fs_mi_matrices / fs_mrmr_select.
//
// Greedy loop.  Step 0 picks argmax rel.  After picking s the row
// r_s[f] = J(f, s) enters the candidates' accumulators:
//   JMI  (Yang & Moody):  acc[f] += r_s[f], from +0.0, in selection order;
//   CMIM (Fleuret):       acc[f] = min(acc[f], r_s[f] - rel[s]), from +inf
// (I(X_f; y | X_s) = I(X_f, X_s; y) - I(X_s; y)).  Step i >= 1 picks the
// unselected feature with the largest acc.  Among exact equals the lowest index
// wins, at every step.  There is no isclose rule here: that rule is surface of
// the mRMR reference (fs_mrmr.h mrmr_is_top), and this selector has no
// reference to match.
//
// Everything here is plain IEEE float64; the build has -ffp-contract=off and no
// fast-math, so the CPU backend, the GPU backend and numpy agree bit for bit on
// a step given the same inputs.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/fastselect_amd.h"
#include "fs_internal.h"
#include "fs_mi.h"

namespace fs {

constexpr int kJmiJmi = 0, kJmiCmim = 1;
// A lane of k_jmi_row keeps one 4 x 4 block of counts per class in registers.
constexpr int kJmiMaxClassesGpu = 4;
// The CPU backend holds one joint table per thread: max kcol^2 * kcol[y] cells.
constexpr int64_t kJmiMaxCellsCpu = (int64_t)1 << 20;

// The accumulator before any row.
FS_HD inline double jmi_start(int method) { return method == kJmiJmi ? 0.0 : HUGE_VAL; }
// The accumulator of a candidate after the row of the selected feature s:
// j = J(f, s), rel_s = rel[s].
FS_HD inline double jmi_update(int method, double acc, double j, double rel_s) {
  if (method == kJmiJmi) return acc + j;
  const double d = j - rel_s;
  return d < acc ? d : acc;
}
// The score step i reads: the relevance at step 0, the accumulator after.
FS_HD inline double jmi_score(int64_t i, double rel, double acc) { return i == 0 ? rel : acc; }
// The order of two candidates (score, index): the higher score, the lower
// index among exact equals; index < 0 is "none".
FS_HD inline bool jmi_beats(double sa, int64_t ia, double sb, int64_t ib) {
  if (ia < 0) return false;
  if (ib < 0) return true;
  return sa > sb || (sa == sb && ia < ib);
}

// One step on the host, serial: the feature step i selects among the
// features with taken[f] == 0 (-1: none is left).
inline int64_t jmi_pick(int64_t i, const double* rel, const double* acc, const uint8_t* taken,
                        int64_t p) {
  double bs = 0.0;
  int64_t bi = -1;
  for (int64_t f = 0; f < p; f++)
    if (!taken[f]) {
      const double s = jmi_score(i, rel[f], acc[f]);
      if (jmi_beats(s, f, bs, bi)) bs = s, bi = f;
    }
  return bi;
}

// Argument checks shared by both backends (the codes themselves are checked
// while they are packed).  `who` opens the messages.
int jmi_check(const char* who, int backend, const uint8_t* codes, const uint8_t* ycodes, int64_t n,
              int64_t p, int n_states, int unit);
int jmi_check_select(int backend, const uint8_t* codes, const uint8_t* ycodes, int64_t n,
                     int64_t p, int n_states, int unit, int method, int64_t k,
                     const double* relevance, const int64_t* selected);
int jmi_check_rows(int backend, const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p,
                   int n_states, int unit, const int64_t* anchors, int64_t m, const double* rows);
int jmi_check_matrix(const double* relevance, const double* joint, int64_t p, int method,
                     int64_t k, const int64_t* selected);

namespace cpu {
// The pieces of a row that fs_pairscan_cpu.cpp takes as they are
// (fs_jmi_cpu.cpp): the joint table of the pair i < j with y,
// tab[(a * kcol[j] + b) * kcol[y] + c]; the cells of the largest joint table
// (FS_EINVAL beyond kJmiMaxCellsCpu; `who` opens the message); and
// out[c] = I(X_c; y) for c < p.
void joint_table(const MiColumns& m, int64_t i, int64_t j, int32_t* tab);
int joint_cells(const MiColumns& m, const char* who, int64_t& cells);
void rel_row(const MiColumns& m, int unit, int n_jobs, double* out);
int jmi_select(const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p, int n_states,
               int unit, int method, int64_t k, int n_jobs, double* relevance, int64_t* selected,
               double* rows);
int jmi_rows(const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p, int n_states,
             int unit, const int64_t* anchors, int64_t m, int n_jobs, double* rows);
int jmi_search_matrix(const double* relevance, const double* joint, int64_t p, int method,
                      int64_t k, int64_t* selected);
}
namespace gpu {
int jmi_select(int device, const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p,
               int n_states, int unit, int method, int64_t k, double* relevance,
               int64_t* selected, double* rows);
int jmi_rows(int device, const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p,
             int n_states, int unit, const int64_t* anchors, int64_t m, double* rows);
int jmi_search_matrix(int device, const double* relevance, const double* joint, int64_t p,
                      int method, int64_t k, int64_t* selected);
// Milliseconds of the calling thread's last GPU jmi_select: upload, pack,
// relevance, rows, steps (HIP events on the call's stream).
void jmi_last_timing(double* ms5);
}

}  // namespace fs
