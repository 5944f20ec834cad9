// fs_mrmr_cpu.cpp -- the argument checks of fs_mrmr_* (both backends) and the
// CPU backend: the relevance and one row of mutual information per selected
// feature from fs_mi_cpu.cpp's packed columns, the columns of a row split over
// host threads, and the greedy loop serial (fs_mrmr.h mrmr_pick).  It replaces
// the selection of mRMR.fit (mRMR.py:96-117) without the p x p matrix of
// calculate_mi_matrices (mRMR.py:94-96).
//
// A row's entries are the pairs fs_mi_matrices computes, by the same table
// code and mi_from_table with the lower index supplying the rows, so they
// equal the CPU matrix's entries bit for bit.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

#include "fs_mrmr.h"

namespace fs {

int mrmr_check(int backend, const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p,
               int n_states, int unit, int method, int64_t k, const double* relevance,
               const int64_t* selected) {
  if (!codes || !ycodes || !relevance || !selected) {
    set_error("fs_mrmr_select: codes, ycodes, relevance and selected must not be NULL");
    return FS_EINVAL;
  }
  if (n < 1 || n >= kMiMaxN) {
    set_error("fs_mrmr_select: n must be in [1, 2^31)");
    return FS_EINVAL;
  }
  if (p < 1) {
    set_error("fs_mrmr_select: p must be >= 1");
    return FS_EINVAL;
  }
  if (n_states < 1 || n_states > kMiMaxStates) {
    set_error("fs_mrmr_select: n_states must be in 1..256");
    return FS_EINVAL;
  }
  if (unit != 0 && unit != 1) {
    set_error("fs_mrmr_select: unit must be 0 (bit) or 1 (nat)");
    return FS_EINVAL;
  }
  if (method != kMrmrMid && method != kMrmrMiq) {
    set_error("fs_mrmr_select: method must be 0 (MID) or 1 (MIQ)");
    return FS_EINVAL;
  }
  if (k < 1 || k > p) {
    set_error("fs_mrmr_select: k must be in 1..p");
    return FS_EINVAL;
  }
  if (backend == FS_BACKEND_GPU && n_states > kMiMaxStatesGpu) {
    set_error("fs_mrmr_select: the GPU backend supports at most 32 states");
    return FS_EINVAL;
  }
  return FS_OK;
}

int mrmr_check_matrix(const double* relevance, const double* redundancy, int64_t p, int method,
                      int64_t k, const int64_t* selected) {
  if (!relevance || !redundancy || !selected) {
    set_error("fs_mrmr_search_matrix: NULL argument");
    return FS_EINVAL;
  }
  if (p < 1) {
    set_error("fs_mrmr_search_matrix: p must be >= 1");
    return FS_EINVAL;
  }
  if (method != kMrmrMid && method != kMrmrMiq) {
    set_error("fs_mrmr_search_matrix: method must be 0 (MID) or 1 (MIQ)");
    return FS_EINVAL;
  }
  if (k < 1 || k > p) {
    set_error("fs_mrmr_search_matrix: k must be in 1..p");
    return FS_EINVAL;
  }
  return FS_OK;
}

namespace cpu {

namespace {

// out[c] = I(X_c; X_anchor) for c < p, 0.0 at c == anchor; anchor = p: the
// relevance.  The column with the lower index supplies the table's rows.
void mi_row(const MiColumns& m, int64_t anchor, int unit, int n_jobs, double* out) {
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
        if (c == anchor) {
          out[c] = 0.0;
          continue;
        }
        const int64_t i = std::min(anchor, c), j = std::max(anchor, c);
        mi_pair_table(m, i, j, tab.data());
        out[c] = mi_from_table(tab.data(), m.S, m.kcol[i], m.kcol[j], m.n, unit, p2.data());
      }
    }
  };
  std::vector<std::thread> th;
  for (int w = 1; w < nt; w++) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
}

// The greedy loop (mRMR.py:96-117).  row(i, f) returns I(.; X_f) over the p
// columns for the feature f that step i picked, valid until the next call
// (NULL: no later step reads it).
template <class RowFn>
void greedy(const double* rel, int64_t p, int method, int64_t k, int64_t* selected,
            std::vector<double>& rsum, std::vector<uint8_t>& taken, RowFn row) {
  for (int64_t i = 0; i < k; i++) {
    const int64_t best = mrmr_pick(method, i, rel, rsum.data(), taken.data(), p);
    selected[i] = best;
    taken[best] = 1;
    if (const double* r = row(i, best))
      for (int64_t c = 0; c < p; c++) rsum[c] += r[c];
  }
}

}  // namespace

int mrmr_select(const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p, int n_states,
                int unit, int method, int64_t k, int n_jobs, double* relevance,
                int64_t* selected, double* rows) {
  MiColumns m;
  std::vector<double> rsum, scratch;
  std::vector<uint8_t> taken;
  try {
    rsum.assign((size_t)p, 0.0);
    taken.assign((size_t)p, 0);
    if (!rows) scratch.resize((size_t)p);
  } catch (const std::bad_alloc&) {
    set_error("fs_mrmr_select: out of host memory");
    return FS_EOOM;
  }
  if (int rc = mi_columns(m, "fs_mrmr_select", codes, ycodes, n, p, n_states, n_jobs)) return rc;
  mi_row(m, p, unit, n_jobs, relevance);
  greedy(relevance, p, method, k, selected, rsum, taken,
         [&](int64_t i, int64_t f) -> const double* {
           // the last pick's row feeds no step: only a caller's rows need it
           if (i + 1 == k && !rows) return nullptr;
           double* out = rows ? rows + (size_t)i * p : scratch.data();
           mi_row(m, f, unit, n_jobs, out);
           return out;
         });
  return FS_OK;
}

int mrmr_search_matrix(const double* relevance, const double* redundancy, int64_t p, int method,
                       int64_t k, int64_t* selected) {
  std::vector<double> rsum;
  std::vector<uint8_t> taken;
  try {
    rsum.assign((size_t)p, 0.0);
    taken.assign((size_t)p, 0);
  } catch (const std::bad_alloc&) {
    set_error("fs_mrmr_search_matrix: out of host memory");
    return FS_EOOM;
  }
  greedy(relevance, p, method, k, selected, rsum, taken,
         [&](int64_t, int64_t f) { return redundancy + (size_t)f * p; });
  return FS_OK;
}

}  // namespace cpu
}  // namespace fs
