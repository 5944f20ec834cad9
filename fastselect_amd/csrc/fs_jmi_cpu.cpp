// fs_jmi_cpu.cpp -- the argument checks of fs_jmi_* (both backends) and the
// CPU backend: the relevance (the pair (f, y), as fs_mrmr_cpu.cpp) and one row
// of joint relevance J(., s) per selected feature from fs_mi_cpu.cpp's packed
// columns, the columns of a row split over host threads, and the greedy loop
// serial (fs_jmi.h jmi_pick, jmi_update).
//
// A pair's joint table T[(a * kcol[hi] + b)][c] comes from the planes (a cell
// is popcount(plane_lo[a] & plane_hi[b] & plane_y[c])) up to the state count at
// which fs_mi_cpu.cpp packs planes, from the byte codes above; mi_from_table
// (fs_mi.h) turns it into the value, so J(lo, hi) equals the CPU relevance of
// the column x_lo * kcol[hi] + x_hi bit for bit.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "fs_jmi.h"

namespace fs {

int jmi_check(const char* who, int backend, const uint8_t* codes, const uint8_t* ycodes, int64_t n,
              int64_t p, int n_states, int unit) {
  const std::string w(who);
  if (!codes || !ycodes) {
    set_error(w + ": codes and ycodes must not be NULL");
    return FS_EINVAL;
  }
  if (n < 1 || n >= kMiMaxN) {
    set_error(w + ": n must be in [1, 2^31)");
    return FS_EINVAL;
  }
  if (p < 1) {
    set_error(w + ": p must be >= 1");
    return FS_EINVAL;
  }
  if (n_states < 1 || n_states > kMiMaxStates) {
    set_error(w + ": n_states must be in 1..256");
    return FS_EINVAL;
  }
  if (unit != 0 && unit != 1) {
    set_error(w + ": unit must be 0 (bit) or 1 (nat)");
    return FS_EINVAL;
  }
  if (backend == FS_BACKEND_GPU && n_states > kMiMaxStatesGpu) {
    set_error(w + ": the GPU backend supports at most 32 states");
    return FS_EINVAL;
  }
  return FS_OK;
}

int jmi_check_select(int backend, const uint8_t* codes, const uint8_t* ycodes, int64_t n,
                     int64_t p, int n_states, int unit, int method, int64_t k,
                     const double* relevance, const int64_t* selected) {
  if (!relevance || !selected) {
    set_error("fs_jmi_select: relevance and selected must not be NULL");
    return FS_EINVAL;
  }
  if (int rc = jmi_check("fs_jmi_select", backend, codes, ycodes, n, p, n_states, unit)) return rc;
  if (method != kJmiJmi && method != kJmiCmim) {
    set_error("fs_jmi_select: method must be 0 (JMI) or 1 (CMIM)");
    return FS_EINVAL;
  }
  if (k < 1 || k > p) {
    set_error("fs_jmi_select: k must be in 1..p");
    return FS_EINVAL;
  }
  return FS_OK;
}

int jmi_check_rows(int backend, const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p,
                   int n_states, int unit, const int64_t* anchors, int64_t m, const double* rows) {
  if (!anchors || !rows) {
    set_error("fs_jmi_rows: anchors and rows must not be NULL");
    return FS_EINVAL;
  }
  if (int rc = jmi_check("fs_jmi_rows", backend, codes, ycodes, n, p, n_states, unit)) return rc;
  if (m < 1) {
    set_error("fs_jmi_rows: m must be >= 1");
    return FS_EINVAL;
  }
  for (int64_t t = 0; t < m; t++)
    if (anchors[t] < 0 || anchors[t] >= p) {
      set_error("fs_jmi_rows: an anchor is outside 0..p-1");
      return FS_EINVAL;
    }
  return FS_OK;
}

int jmi_check_matrix(const double* relevance, const double* joint, int64_t p, int method,
                     int64_t k, const int64_t* selected) {
  if (!relevance || !joint || !selected) {
    set_error("fs_jmi_search_matrix: NULL argument");
    return FS_EINVAL;
  }
  if (p < 1) {
    set_error("fs_jmi_search_matrix: p must be >= 1");
    return FS_EINVAL;
  }
  if (method != kJmiJmi && method != kJmiCmim) {
    set_error("fs_jmi_search_matrix: method must be 0 (JMI) or 1 (CMIM)");
    return FS_EINVAL;
  }
  if (k < 1 || k > p) {
    set_error("fs_jmi_search_matrix: k must be in 1..p");
    return FS_EINVAL;
  }
  return FS_OK;
}

namespace cpu {

namespace {

#if defined(__x86_64__) && defined(__GNUC__)
#define FS_JMI_POPCNT __attribute__((target("popcnt")))
inline bool have_popcnt() { return __builtin_cpu_supports("popcnt"); }
#else
#define FS_JMI_POPCNT
inline bool have_popcnt() { return false; }
#endif

// tab[(a * kj + b) * ky + c] = popcount(plane_i[a] & plane_j[b] & plane_y[c])
template <bool HW>
__attribute__((always_inline)) inline void joint_planes(const uint64_t* pi, const uint64_t* pj,
                                                        const uint64_t* py, int64_t W, int ki,
                                                        int kj, int ky, int32_t* tab) {
  for (int a = 0; a < ki; a++)
    for (int b = 0; b < kj; b++)
      for (int c = 0; c < ky; c++) {
        const uint64_t* x = pi + (size_t)a * W;
        const uint64_t* y = pj + (size_t)b * W;
        const uint64_t* z = py + (size_t)c * W;
        uint64_t s = 0;
        for (int64_t w = 0; w < W; w++) s += (uint64_t)__builtin_popcountll(x[w] & y[w] & z[w]);
        tab[((size_t)a * kj + b) * ky + c] = (int32_t)s;
      }
}
void joint_planes_sw(const uint64_t* pi, const uint64_t* pj, const uint64_t* py, int64_t W, int ki,
                     int kj, int ky, int32_t* tab) {
  joint_planes<false>(pi, pj, py, W, ki, kj, ky, tab);
}
FS_JMI_POPCNT void joint_planes_hw(const uint64_t* pi, const uint64_t* pj, const uint64_t* py,
                                   int64_t W, int ki, int kj, int ky, int32_t* tab) {
  joint_planes<true>(pi, pj, py, W, ki, kj, ky, tab);
}

}  // namespace

// joint_table, joint_cells and rel_row are fs_pairscan_cpu.cpp's too (fs_jmi.h).
// The joint table of the pair i < j with y: tab[(a * kcol[j] + b) * kcol[y] + c].
void joint_table(const MiColumns& m, int64_t i, int64_t j, int32_t* tab) {
  static const auto tabfn = have_popcnt() ? joint_planes_hw : joint_planes_sw;
  const int S = m.S, ki = m.kcol[i], kj = m.kcol[j], ky = m.kcol[m.p];
  if (m.planes_route) {
    tabfn(&m.planes[(size_t)i * S * m.W], &m.planes[(size_t)j * S * m.W],
          &m.planes[(size_t)m.p * S * m.W], m.W, ki, kj, ky, tab);
  } else {
    std::memset(tab, 0, (size_t)ki * kj * ky * 4);
    const uint8_t* ci = &m.colT[(size_t)i * m.n];
    const uint8_t* cj = &m.colT[(size_t)j * m.n];
    const uint8_t* cy = &m.colT[(size_t)m.p * m.n];
    for (int64_t s = 0; s < m.n; s++) tab[((size_t)ci[s] * kj + cj[s]) * ky + cy[s]]++;
  }
}

// The cells of the largest joint table; FS_EINVAL beyond kJmiMaxCellsCpu.
int joint_cells(const MiColumns& m, const char* who, int64_t& cells) {
  int kmax = 1;
  for (int64_t c = 0; c < m.p; c++) kmax = std::max(kmax, (int)m.kcol[c]);
  cells = (int64_t)kmax * kmax * m.kcol[m.p];
  if (cells > kJmiMaxCellsCpu) {
    set_error(std::string(who) +
              ": the CPU backend supports at most 2^20 cells of a joint table "
              "(states^2 * classes)");
    return FS_EINVAL;
  }
  return FS_OK;
}

// out[c] = I(X_c; y) for c < p: mi_row of fs_mrmr_cpu.cpp for the target.
void rel_row(const MiColumns& m, int unit, int n_jobs, double* out) {
  const int64_t p = m.p;
  const int64_t kChunk = 256;
  const int64_t tasks = (p + kChunk - 1) / kChunk;
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(hardware_threads(n_jobs), tasks));
  std::atomic<int64_t> next{0};
  auto work = [&]() {
    std::vector<int32_t> tab((size_t)m.S * m.S);
    std::vector<double> p2((size_t)m.S);
    for (int64_t t = next++; t < tasks; t = next++) {
      const int64_t c1 = std::min(p, (t + 1) * kChunk);
      for (int64_t c = t * kChunk; c < c1; c++) {
        mi_pair_table(m, c, p, tab.data());
        out[c] = mi_from_table(tab.data(), m.S, m.kcol[c], m.kcol[p], m.n, unit, p2.data());
      }
    }
  };
  std::vector<std::thread> th;
  for (int w = 1; w < nt; w++) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
}

namespace {

// out[c] = J(c, anchor) for c < p, 0.0 at c == anchor.  The column with the
// lower index supplies the joint state's high digit.
void jmi_row(const MiColumns& m, int64_t cells, int64_t anchor, int unit, int n_jobs,
             double* out) {
  const int64_t p = m.p;
  const int64_t kChunk = 64;
  const int64_t tasks = (p + kChunk - 1) / kChunk;
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(hardware_threads(n_jobs), tasks));
  const int ky = m.kcol[p];
  std::atomic<int64_t> next{0};
  auto work = [&]() {
    std::vector<int32_t> tab((size_t)cells);
    std::vector<double> p2((size_t)ky);
    for (int64_t t = next++; t < tasks; t = next++) {
      const int64_t c1 = std::min(p, (t + 1) * kChunk);
      for (int64_t c = t * kChunk; c < c1; c++) {
        if (c == anchor) {
          out[c] = 0.0;
          continue;
        }
        const int64_t i = std::min(anchor, c), j = std::max(anchor, c);
        joint_table(m, i, j, tab.data());
        out[c] = mi_from_table(tab.data(), ky, m.kcol[i] * m.kcol[j], ky, m.n, unit, p2.data());
      }
    }
  };
  std::vector<std::thread> th;
  for (int w = 1; w < nt; w++) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
}

// The greedy loop (fs_jmi.h).  row(i, f) returns J(., f) over the p columns
// for the feature f that step i picked, valid until the next call (NULL: no
// later step reads it).
template <class RowFn>
void greedy(const double* rel, int64_t p, int method, int64_t k, int64_t* selected,
            std::vector<double>& acc, std::vector<uint8_t>& taken, RowFn row) {
  for (int64_t i = 0; i < k; i++) {
    const int64_t best = jmi_pick(i, rel, acc.data(), taken.data(), p);
    selected[i] = best;
    taken[best] = 1;
    if (const double* r = row(i, best))
      for (int64_t c = 0; c < p; c++) acc[c] = jmi_update(method, acc[c], r[c], rel[best]);
  }
}

}  // namespace

int jmi_select(const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p, int n_states,
               int unit, int method, int64_t k, int n_jobs, double* relevance, int64_t* selected,
               double* rows) {
  MiColumns m;
  std::vector<double> acc, scratch;
  std::vector<uint8_t> taken;
  try {
    acc.assign((size_t)p, jmi_start(method));
    taken.assign((size_t)p, 0);
    if (!rows) scratch.resize((size_t)p);
  } catch (const std::bad_alloc&) {
    set_error("fs_jmi_select: out of host memory");
    return FS_EOOM;
  }
  if (int rc = mi_columns(m, "fs_jmi_select", codes, ycodes, n, p, n_states, n_jobs)) return rc;
  int64_t cells = 0;
  if (int rc = joint_cells(m, "fs_jmi_select", cells)) return rc;
  rel_row(m, unit, n_jobs, relevance);
  greedy(relevance, p, method, k, selected, acc, taken,
         [&](int64_t i, int64_t f) -> const double* {
           // the last pick's row feeds no step: only a caller's rows need it
           if (i + 1 == k && !rows) return nullptr;
           double* out = rows ? rows + (size_t)i * p : scratch.data();
           jmi_row(m, cells, f, unit, n_jobs, out);
           return out;
         });
  return FS_OK;
}

int jmi_rows(const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p, int n_states,
             int unit, const int64_t* anchors, int64_t mrows, int n_jobs, double* rows) {
  MiColumns m;
  if (int rc = mi_columns(m, "fs_jmi_rows", codes, ycodes, n, p, n_states, n_jobs)) return rc;
  int64_t cells = 0;
  if (int rc = joint_cells(m, "fs_jmi_rows", cells)) return rc;
  for (int64_t t = 0; t < mrows; t++)
    jmi_row(m, cells, anchors[t], unit, n_jobs, rows + (size_t)t * p);
  return FS_OK;
}

int jmi_search_matrix(const double* relevance, const double* joint, int64_t p, int method,
                      int64_t k, int64_t* selected) {
  std::vector<double> acc;
  std::vector<uint8_t> taken;
  try {
    acc.assign((size_t)p, jmi_start(method));
    taken.assign((size_t)p, 0);
  } catch (const std::bad_alloc&) {
    set_error("fs_jmi_search_matrix: out of host memory");
    return FS_EOOM;
  }
  greedy(relevance, p, method, k, selected, acc, taken,
         [&](int64_t, int64_t f) { return joint + (size_t)f * p; });
  return FS_OK;
}

}  // namespace cpu
}  // namespace fs
