// fs_mi_cpu.cpp -- the argument checks of fs_mi_matrices (both backends) and
// its CPU backend: every pair's contingency table from the column-major
// codes, the pairs split over host threads.  It replaces _mi_pair_cpu and
// _batch_mi_cpu (mutual_information.py:25-63).  The packing (mi_columns) and
// one pair's table (mi_pair_table) also serve fs_mrmr_cpu.cpp.
//
// Two ways to a table, chosen by the state count (measured):
// up to kPlaneStates states a column is one 64-bit plane per state and a cell
// is popcount(AND), S^2 n / 64 word operations per pair; above, the table walk
// of the reference, n increments per pair, is cheaper.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <new>
#include <string>
#include <thread>

#include "../../include/fastselect_amd.h"
#include "fs_mi.h"

namespace fs {

int mi_check(int backend, const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p,
             int n_states, int unit, const double* relevance) {
  if (!codes || !ycodes || !relevance) {
    set_error("fs_mi_matrices: codes, ycodes and relevance must not be NULL");
    return FS_EINVAL;
  }
  if (n < 1 || n >= kMiMaxN) {
    set_error("fs_mi_matrices: n must be in [1, 2^31)");
    return FS_EINVAL;
  }
  if (p < 1) {
    set_error("fs_mi_matrices: p must be >= 1");
    return FS_EINVAL;
  }
  if (n_states < 1 || n_states > kMiMaxStates) {
    set_error("fs_mi_matrices: n_states must be in 1..256");
    return FS_EINVAL;
  }
  if (unit != 0 && unit != 1) {
    set_error("fs_mi_matrices: unit must be 0 (bit) or 1 (nat)");
    return FS_EINVAL;
  }
  if (backend == FS_BACKEND_GPU && n_states > kMiMaxStatesGpu) {
    set_error("fs_mi_matrices: the GPU backend supports at most 32 states");
    return FS_EINVAL;
  }
  return FS_OK;
}

namespace cpu {

namespace {

// One thread, n = 2000, microseconds per pair, planes / walk: 3 states 0.33 /
// 1.57, 8 states 2.0 / 2.5, 10 states 3.1 / 3.0, 32 states 27 / 15.
constexpr int kPlaneStates = 8;

#if defined(__x86_64__) && defined(__GNUC__)
#define FS_MI_POPCNT __attribute__((target("popcnt")))
inline bool have_popcnt() { return __builtin_cpu_supports("popcnt"); }
#else
#define FS_MI_POPCNT
inline bool have_popcnt() { return false; }
#endif

// tab[a * S + b] = popcount(plane_i[a] & plane_j[b]) for a < ki, b < kj
template <bool HW>
__attribute__((always_inline)) inline void table_planes(const uint64_t* pi, const uint64_t* pj,
                                                        int64_t W, int S, int ki, int kj,
                                                        int32_t* tab) {
  for (int a = 0; a < ki; a++)
    for (int b = 0; b < kj; b++) {
      const uint64_t* x = pi + (size_t)a * W;
      const uint64_t* y = pj + (size_t)b * W;
      uint64_t c = 0;
      for (int64_t w = 0; w < W; w++) c += (uint64_t)__builtin_popcountll(x[w] & y[w]);
      tab[a * S + b] = (int32_t)c;
    }
}
void table_planes_sw(const uint64_t* pi, const uint64_t* pj, int64_t W, int S, int ki, int kj,
                     int32_t* tab) {
  table_planes<false>(pi, pj, W, S, ki, kj, tab);
}
FS_MI_POPCNT void table_planes_hw(const uint64_t* pi, const uint64_t* pj, int64_t W, int S,
                                  int ki, int kj, int32_t* tab) {
  table_planes<true>(pi, pj, W, S, ki, kj, tab);
}

}  // namespace

int mi_columns(MiColumns& m, const char* who, const uint8_t* codes, const uint8_t* ycodes,
               int64_t n, int64_t p, int n_states, int n_jobs) {
  const int S = n_states;
  const int64_t P1 = p + 1;  // y is column p
  m.n = n, m.p = p, m.S = S;
  m.planes_route = S <= kPlaneStates;
  m.W = (n + 63) / 64;
  const int64_t W = m.W;
  const bool planes_route = m.planes_route;
  std::vector<uint8_t>& colT = m.colT;
  std::vector<uint64_t>& planes = m.planes;
  std::vector<int32_t>& kcol = m.kcol;
  try {
    kcol.assign((size_t)P1, 1);
    colT.resize((size_t)P1 * n);
    if (planes_route) planes.assign((size_t)P1 * S * W, 0);
  } catch (const std::bad_alloc&) {
    set_error(std::string(who) + ": out of host memory for the column codes");
    return FS_EOOM;
  }
  const int nt_all = hardware_threads(n_jobs);
  std::atomic<int> bad{0};
  {
    // transpose (and pack) in blocks of 64 columns; a code >= n_states is an error
    const int64_t kBlock = 64;
    const int64_t tasks = (P1 + kBlock - 1) / kBlock;
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(nt_all, tasks));
    std::atomic<int64_t> next{0};
    auto work = [&]() {
      for (int64_t t = next++; t < tasks; t = next++) {
        const int64_t c0 = t * kBlock, c1 = std::min(P1, c0 + kBlock);
        for (int64_t i = 0; i < n; i++)
          for (int64_t c = c0; c < c1; c++)
            colT[(size_t)c * n + i] = c < p ? codes[(size_t)i * p + c] : ycodes[i];
        for (int64_t c = c0; c < c1; c++) {
          const uint8_t* col = &colT[(size_t)c * n];
          int mx = 0;
          for (int64_t i = 0; i < n; i++) mx = std::max<int>(mx, col[i]);
          if (mx >= S) {
            bad.store(1, std::memory_order_relaxed);
            continue;
          }
          kcol[c] = mx + 1;
          if (planes_route)
            for (int64_t i = 0; i < n; i++)
              planes[((size_t)c * S + col[i]) * W + (i >> 6)] |= 1ull << (i & 63);
        }
      }
    };
    std::vector<std::thread> th;
    for (int w = 1; w < nt; w++) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
  }
  if (bad.load()) {
    set_error(std::string(who) + ": a code is >= n_states");
    return FS_EINVAL;
  }
  return FS_OK;
}

void mi_pair_table(const MiColumns& m, int64_t i, int64_t j, int32_t* tab) {
  static const auto tabfn = have_popcnt() ? table_planes_hw : table_planes_sw;
  const int S = m.S, ki = m.kcol[i], kj = m.kcol[j];
  if (m.planes_route) {
    tabfn(&m.planes[(size_t)i * S * m.W], &m.planes[(size_t)j * S * m.W], m.W, S, ki, kj, tab);
  } else {
    for (int a = 0; a < ki; a++) std::memset(&tab[(size_t)a * S], 0, (size_t)kj * 4);
    const uint8_t* ci = &m.colT[(size_t)i * m.n];
    const uint8_t* cj = &m.colT[(size_t)j * m.n];
    for (int64_t s = 0; s < m.n; s++) tab[(size_t)ci[s] * S + cj[s]]++;
  }
}

int mi_matrices(const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p, int n_states,
                int unit, int n_jobs, double* relevance, double* redundancy,
                int32_t* counts_out) {
  const int S = n_states;
  MiColumns m;
  if (int rc = mi_columns(m, "fs_mi_matrices", codes, ycodes, n, p, n_states, n_jobs)) return rc;
  const std::vector<int32_t>& kcol = m.kcol;
  const int nt_all = hardware_threads(n_jobs);
  if (redundancy) std::memset(redundancy, 0, (size_t)p * p * sizeof(double));
  if (counts_out) std::memset(counts_out, 0, (size_t)p * p * S * S * sizeof(int32_t));

  // one task per first column i: its pair with y, then with every j > i
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(nt_all, p));
  std::atomic<int64_t> next{0};
  auto work = [&]() {
    std::vector<int32_t> tab((size_t)S * S);
    std::vector<double> p2((size_t)S);
    for (int64_t i = next++; i < p; i = next++) {
      const int ki = kcol[i];
      // j = p (the target) first, then the columns after i
      const int64_t jend = (redundancy || counts_out) ? p : i + 1;
      for (int64_t jj = i; jj < jend; jj++) {
        const int64_t j = jj == i ? p : jj;
        const int kj = kcol[j];
        mi_pair_table(m, i, j, tab.data());
        const double mi = mi_from_table(tab.data(), S, ki, kj, n, unit, p2.data());
        if (j == p) {
          relevance[i] = mi;
          continue;
        }
        if (redundancy) {
          redundancy[(size_t)i * p + j] = mi;
          redundancy[(size_t)j * p + i] = mi;
        }
        if (counts_out) {
          int32_t* out = counts_out + ((size_t)i * p + j) * S * S;
          for (int a = 0; a < ki; a++)
            std::memcpy(out + (size_t)a * S, &tab[(size_t)a * S], (size_t)kj * 4);
        }
      }
    }
  };
  std::vector<std::thread> th;
  for (int w = 1; w < nt; w++) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
  return FS_OK;
}

}  // namespace cpu
}  // namespace fs
