// fs_mi.h -- what the two backends of fs_mi_matrices (fs_mi_cpu.cpp,
// fs_mi.hip) share: the argument checks and the epilogue that turns one
// pair's integer contingency table into its float64 mutual information.
//
// Discrete mutual information (the reference's mutual_information.py) of
// every pair of p columns plus the target: a column is one bit-plane per state
// over the samples, a table cell is popcount(plane_i[a] & plane_j[b]), and
// every quantity is an integer until mi_from_table().  The target y is
// treated as column p, so the relevance I(X_f; y) is the pair (f, p) with the
// rows taken from X_f (mutual_information.py:56).
#pragma once

#include <cstdint>
#include <vector>

#include "fs_internal.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

namespace fs {

constexpr int kMiMaxStates = 256;      // codes are bytes
constexpr int kMiMaxStatesGpu = 32;    // mutual_information.py:66 _MAX_STATES_GPU
constexpr int64_t kMiMaxN = (int64_t)1 << 31;
constexpr double kMiMaxBytes = 1e15;   // a larger device block is FS_EOOM before any allocation

// _mi_pair_cpu's float64 expressions in their written order
// (mutual_information.py:31-46) on an integer table tab[a * ld + b], a < k1
// (states of the first column), b < k2:
//   pxy = count / n; p1[a] = sum_b pxy[a][b]; p2[b] = sum_a pxy[a][b], each
//   sum in index order from 0.0; mi += pxy * log(pxy / (p1[a] * p2[b] + eps))
//   over the cells with pxy > eps, row-major; mi / log(2.0) for bits.
// p2 is k2 doubles of workspace.  States a column never takes add exact
// zeros, so a table wider than the reference's (its k = max code + 1) gives
// the same bits.  The build has -ffp-contract=off and no fast-math: no
// product here fuses with a sum.
//
// The three steps are functions of their own because the GPU kernel runs the
// same expressions with a pair's cells spread over lanes (fs_mi.hip): a cell
// that the reference skips contributes mi_term() == 0.0, and mi + 0.0 == mi
// for every mi this sum can reach (it starts at +0.0 and never becomes -0.0),
// so adding every cell in row-major order gives the bits of the skipping loop.
FS_HD inline double mi_pxy(int32_t count, double dn) { return (double)count / dn; }
FS_HD inline double mi_term(double pxy, double p1, double p2) {
  const double eps = 1e-12;
  return pxy > eps ? pxy * log(pxy / (p1 * p2 + eps)) : 0.0;
}
FS_HD inline double mi_finish(double mi, int unit) { return unit == 0 ? mi / log(2.0) : mi; }
// The one stated deviation: a column that takes a single state (used = its
// states with a non-zero marginal) shares no information with anything, and
// the pair's MI is exactly 0.0.  The expressions above give about
// -k * 1e-12 there (every term is pxy * log(pxy / (pxy + eps))).
FS_HD inline bool mi_constant(int used1, int used2) { return used1 <= 1 || used2 <= 1; }

FS_HD inline double mi_from_table(const int32_t* tab, int ld, int k1, int k2, int64_t n, int unit,
                                  double* p2) {
  const double dn = (double)n;
  for (int b = 0; b < k2; b++) p2[b] = 0.0;
  for (int a = 0; a < k1; a++)
    for (int b = 0; b < k2; b++) p2[b] += mi_pxy(tab[a * ld + b], dn);
  double mi = 0.0;
  int used1 = 0, used2 = 0;
  for (int a = 0; a < k1; a++) {
    double p1 = 0.0;
    for (int b = 0; b < k2; b++) p1 += mi_pxy(tab[a * ld + b], dn);
    for (int b = 0; b < k2; b++) mi += mi_term(mi_pxy(tab[a * ld + b], dn), p1, p2[b]);
    used1 += p1 > 0.0;
  }
  for (int b = 0; b < k2; b++) used2 += p2[b] > 0.0;
  return mi_constant(used1, used2) ? 0.0 : mi_finish(mi, unit);
}

// Argument checks of fs_mi_matrices shared by both backends (the codes
// themselves are checked while they are packed).
int mi_check(int backend, const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p,
             int n_states, int unit, const double* relevance);

namespace cpu {
// The columns of one CPU call, packed once (fs_mi_cpu.cpp): the codes
// column-major with y as column p, each column's state count (max code + 1)
// and, up to kPlaneStates states, one 64-bit plane per state.
struct MiColumns {
  int64_t n = 0, p = 0, W = 0;
  int S = 0;
  bool planes_route = false;
  std::vector<uint8_t> colT;     // [p + 1][n]
  std::vector<uint64_t> planes;  // [p + 1][S][W]
  std::vector<int32_t> kcol;     // [p + 1]
};
// `who` opens the error messages.  FS_EOOM, or FS_EINVAL for a code >= n_states.
int mi_columns(MiColumns& m, const char* who, const uint8_t* codes, const uint8_t* ycodes,
               int64_t n, int64_t p, int n_states, int n_jobs);
// The table of the pair (i, j) into tab[a * S + b], a < kcol[i] (the rows are
// column i's states), b < kcol[j].
void mi_pair_table(const MiColumns& m, int64_t i, int64_t j, int32_t* tab);
int mi_matrices(const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p, int n_states,
                int unit, int n_jobs, double* relevance, double* redundancy, int32_t* counts_out);
}
namespace gpu {
int mi_matrices(int device, const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p,
                int n_states, int unit, double* relevance, double* redundancy,
                int32_t* counts_out);
// Milliseconds of the calling thread's last GPU mi_matrices: upload, pack,
// scan, download (HIP events on the call's stream).
void mi_last_timing(double* ms4);
#if defined(__HIPCC__)
struct DevArena;
// From codes to packed planes, for every unit that scans them (fs_mi.hip,
// fs_cfs.hip, fs_mrmr.hip): codes x [n][p] and y (as column p) ->
// planes[(w * P1p + c) * SP + s] over W = (n + 31) / 32 words, SP = n_states
// rounded up to 4 (NB blocks of 4), P1p = p + 1 columns rounded up to a
// multiple of `pad` (the padding zero); kcol[c] = max code + 1.  In call
// order: shape, alloc, upload, pack (k_mi_pack), fetch_bad, and after a
// synchronisation check.  The caller records its own events in between and
// chooses where it synchronises.  `who` opens the error messages.
struct MiPlanes {
  const char* who = "";
  int64_t n = 0, p = 0, P1 = 0, P1p = 0, W = 0;
  int S = 0, NB = 0, SP = 0;
  uint8_t *dx = nullptr, *dy = nullptr;  // the uploaded codes: dead after pack
  uint32_t* planes = nullptr;
  int32_t* kcol = nullptr;
  int* dbad = nullptr;
  int bad = 0;  // fetch_bad's target: a code is >= n_states
  // The geometry, and FS_EOOM for sizes beyond any device.
  int shape(const char* who_, int64_t n_, int64_t p_, int n_states, int pad);
  // planes, kcol, dbad from `mem`, dx, dy from `up` (may be the same arena).
  int alloc(DevArena& mem, DevArena& up);
  int upload(const uint8_t* codes, const uint8_t* ycodes, hipStream_t s);
  int pack(hipStream_t s);
  int fetch_bad(hipStream_t s);
  int check() const;  // FS_EINVAL for a code >= n_states
};
#endif
}

}  // namespace fs
