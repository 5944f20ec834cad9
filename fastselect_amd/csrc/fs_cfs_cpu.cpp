// fs_cfs_cpu.cpp -- the argument checks and the search driver of fs_cfs_*
// (both backends) and the CPU backend: the handle with its lazy rows of
// symmetrical uncertainty, and the step scan over host threads.  It replaces
// _entropy, _mutual_information, _symmetrical_uncertainty,
// _precompute_correlations_cpu and _best_first_search (CFS.py:26-162).
//
// Tables come the two ways of fs_mi_cpu.cpp: 64-bit state planes and
// popcount(AND) up to kPlaneStates states, the table walk above.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <functional>
#include <new>
#include <thread>
#include <unordered_map>

#include "fs_cfs.h"

namespace fs {

int cfs_check(int backend, const void* out, const uint8_t* codes, const uint8_t* ycodes, int64_t n,
              int64_t p, int n_states) {
  if (!out || !codes || !ycodes) {
    set_error("fs_cfs_create: out, codes and ycodes must not be NULL");
    return FS_EINVAL;
  }
  if (n < 1 || n >= kMiMaxN) {
    set_error("fs_cfs_create: n must be in [1, 2^31)");
    return FS_EINVAL;
  }
  if (p < 1) {
    set_error("fs_cfs_create: p must be >= 1");
    return FS_EINVAL;
  }
  if (n_states < 1 || n_states > kCfsMaxStates) {
    set_error("fs_cfs_create: n_states must be in 1..256");
    return FS_EINVAL;
  }
  if (backend == FS_BACKEND_GPU && n_states > kCfsMaxStatesGpu) {
    set_error("fs_cfs_create: the GPU backend supports at most 32 states");
    return FS_EINVAL;
  }
  return FS_OK;
}

int cfs_check_matrix(const float* r_cf, const float* r_ff, int64_t p, const int64_t* selected,
                     const int64_t* n_selected, const double* merits) {
  if (!r_cf || !r_ff || !selected || !n_selected || !merits) {
    set_error("fs_cfs_search_matrix: NULL argument");
    return FS_EINVAL;
  }
  if (p < 1) {
    set_error("fs_cfs_search_matrix: p must be >= 1");
    return FS_EINVAL;
  }
  return FS_OK;
}

int cfs_search_drive(CfsStepper& st, const float* r_cf, int64_t p, double min_r_cf,
                     int64_t* selected, int64_t* n_selected, double* merits) {
  *n_selected = 0;
  int64_t first = 0;  // np.argmax: the lowest index of the maximum
  for (int64_t i = 1; i < p; i++)
    if (r_cf[i] > r_cf[first]) first = i;
  if ((double)r_cf[first] < min_r_cf) return FS_OK;
  // ent[t][s] = r_ff[selected[t], selected[s]], s < t
  std::vector<std::vector<float>> ent;
  std::vector<float> entries;
  try {
    entries.resize((size_t)p);
    ent.emplace_back();
  } catch (const std::bad_alloc&) {
    set_error("fs_cfs_search: out of host memory");
    return FS_EOOM;
  }
  if (int rc = st.begin(first)) return rc;
  selected[0] = first;
  double current = (double)r_cf[first];  // the merit of one feature is its r_cf
  merits[0] = current;
  int64_t k = 1;
  while (k < p) {
    // the part of a candidate's sums that every candidate shares, in the
    // reference's order (CFS.py:137-144)
    double base_cf = 0.0, base_ff = 0.0;
    for (int64_t s = 0; s < k; s++) base_cf += (double)r_cf[selected[s]];
    for (int64_t a = 0; a < k; a++)
      for (int64_t b = 0; b < k; b++)
        if (selected[a] < selected[b]) base_ff += (double)(a > b ? ent[a][b] : ent[b][a]);
    int64_t best_i = -1;
    double best_merit = current;
    if (int rc = st.step(k, base_cf, base_ff, current, &best_i, &best_merit, entries.data()))
      return rc;
    if (best_i < 0) break;
    try {
      ent.emplace_back(entries.begin(), entries.begin() + k);
    } catch (const std::bad_alloc&) {
      set_error("fs_cfs_search: out of host memory");
      return FS_EOOM;
    }
    selected[k] = best_i;
    merits[k] = best_merit;
    current = best_merit;
    k++;
  }
  *n_selected = k;
  return FS_OK;
}

namespace cpu {

namespace {

constexpr int kPlaneStates = 8;  // fs_mi_cpu.cpp's measured crossover

#if defined(__x86_64__) && defined(__GNUC__)
#define FS_CFS_POPCNT __attribute__((target("popcnt")))
inline bool have_popcnt() { return __builtin_cpu_supports("popcnt"); }
#else
#define FS_CFS_POPCNT
inline bool have_popcnt() { return false; }
#endif

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
FS_CFS_POPCNT void table_planes_hw(const uint64_t* pi, const uint64_t* pj, int64_t W, int S,
                                   int ki, int kj, int32_t* tab) {
  table_planes<true>(pi, pj, W, S, ki, kj, tab);
}

template <class F>
void run_threads(int nt, F work) {
  std::vector<std::thread> th;
  for (int w = 1; w < nt; w++) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
}

// The step scan over host threads: contiguous index ranges, their results
// combined in range order by cfs_beats (the lowest index among equal merits).
struct CpuStepper : CfsStepper {
  const float* r_cf;
  int64_t p;
  double min_r_cf;
  int nt;
  std::vector<uint8_t> taken;
  std::vector<int64_t> sel, rowof;
  // makes the row of `feature` row k of the search: sets rowof[k]; base = the
  // rows' storage and stride (they may move when the storage grows)
  std::function<int(int64_t feature, int64_t k)> add_row;
  std::function<const float*()> base;
  int64_t stride;

  int begin(int64_t first) override {
    taken.assign((size_t)p, 0);
    sel.assign(1, first);
    rowof.assign((size_t)p, 0);
    taken[first] = 1;
    return add_row(first, 0);
  }
  int step(int64_t k, double base_cf, double base_ff, double current, int64_t* best_i,
           double* best_merit, float* entries) override {
    const float* rows = base();
    const int64_t kChunk = 4096;
    const int64_t tasks = (p + kChunk - 1) / kChunk;
    const int n_thr = (int)std::max<int64_t>(1, std::min<int64_t>(nt, tasks));
    std::vector<double> tm((size_t)tasks, current);
    std::vector<int64_t> ti((size_t)tasks, -1);
    std::atomic<int64_t> next{0};
    run_threads(n_thr, [&]() {
      for (int64_t t = next++; t < tasks; t = next++) {
        double bm = current;
        int64_t bi = -1;
        const int64_t i1 = std::min(p, (t + 1) * kChunk);
        for (int64_t i = t * kChunk; i < i1; i++) {
          if (!cfs_is_candidate(taken.data(), r_cf, min_r_cf, i)) continue;
          const double m =
              cfs_candidate_merit(base_cf, base_ff, r_cf, rows, rowof.data(), stride, k, i);
          if (cfs_beats(m, i, bm, bi)) bm = m, bi = i;
        }
        tm[t] = bm, ti[t] = bi;
      }
    });
    double bm = current;
    int64_t bi = -1;
    for (int64_t t = 0; t < tasks; t++)
      if (cfs_beats(tm[t], ti[t], bm, bi)) bm = tm[t], bi = ti[t];
    *best_i = bi;
    *best_merit = bm;
    if (bi < 0) return FS_OK;
    taken[bi] = 1;
    if (int rc = add_row(bi, k)) return rc;
    rows = base();
    for (int64_t s = 0; s < k; s++) entries[s] = rows[rowof[k] * stride + sel[s]];
    sel.push_back(bi);
    return FS_OK;
  }
};

struct CfsCpu : fs_cfs {
  int S = 0, n_jobs = -1;
  int64_t W = 0;
  bool planes_route = false;
  std::vector<uint8_t> colT;     // [p + 1][n] codes, column-major; y is column p
  std::vector<uint64_t> planes;  // [p + 1][S][W]
  std::vector<int32_t> kcol;     // state count of a column: max code + 1
  std::vector<double> hcol;      // entropy of a column
  std::vector<float> r_cf;
  std::vector<float> cache;      // rows of the search, in selection order
  std::unordered_map<int64_t, int64_t> slot;  // feature -> row of cache

  // out[c] = SU(anchor, c) for c < p (the diagonal 0); anchor = p: r_cf
  void compute_row(int64_t anchor, float* out) {
    const auto tabfn = have_popcnt() ? table_planes_hw : table_planes_sw;
    const int64_t kChunk = 256;
    const int64_t tasks = (p + kChunk - 1) / kChunk;
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(hardware_threads(n_jobs), tasks));
    std::atomic<int64_t> next{0};
    run_threads(nt, [&]() {
      std::vector<int32_t> tab((size_t)S * S);
      std::vector<double> py((size_t)S);
      for (int64_t t = next++; t < tasks; t = next++) {
        const int64_t c1 = std::min(p, (t + 1) * kChunk);
        for (int64_t c = t * kChunk; c < c1; c++) {
          if (c == anchor) {
            out[c] = 0.0f;
            continue;
          }
          // the column with the lower index supplies the rows (CFS.py:96-102)
          const int64_t i = std::min(anchor, c), j = std::max(anchor, c);
          const int ki = kcol[i], kj = kcol[j];
          if (planes_route) {
            tabfn(&planes[(size_t)i * S * W], &planes[(size_t)j * S * W], W, S, ki, kj,
                  tab.data());
          } else {
            for (int a = 0; a < ki; a++) std::memset(&tab[(size_t)a * S], 0, (size_t)kj * 4);
            const uint8_t* ci = &colT[(size_t)i * n];
            const uint8_t* cj = &colT[(size_t)j * n];
            for (int64_t s = 0; s < n; s++) tab[(size_t)ci[s] * S + cj[s]]++;
          }
          const double mi = cfs_mi_from_table(tab.data(), S, ki, kj, n, py.data());
          out[c] = cfs_su(mi, hcol[i], hcol[j]);
        }
      }
    });
  }

  int relevance(float* out) override {
    std::memcpy(out, r_cf.data(), (size_t)p * sizeof(float));
    return FS_OK;
  }
  int row(int64_t feature, float* out) override {
    auto it = slot.find(feature);
    if (it != slot.end())
      std::memcpy(out, &cache[(size_t)it->second * p], (size_t)p * sizeof(float));
    else
      compute_row(feature, out);
    return FS_OK;
  }
  int search(double min_r_cf, int64_t* selected, int64_t* n_selected, double* merits) override {
    slot.clear();
    cache.clear();
    CpuStepper st;
    st.r_cf = r_cf.data(), st.p = p, st.min_r_cf = min_r_cf, st.nt = hardware_threads(n_jobs);
    st.stride = p;
    st.base = [&]() { return cache.data(); };
    st.add_row = [&](int64_t f, int64_t k) {
      try {
        cache.resize((size_t)(k + 1) * p);
      } catch (const std::bad_alloc&) {
        set_error("fs_cfs_search: out of host memory for the row cache");
        return (int)FS_EOOM;
      }
      compute_row(f, &cache[(size_t)k * p]);
      slot[f] = k;
      st.rowof[k] = k;
      return (int)FS_OK;
    };
    return cfs_search_drive(st, r_cf.data(), p, min_r_cf, selected, n_selected, merits);
  }
};

}  // namespace

int cfs_create(fs_cfs** out, const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p,
               int n_states, int n_jobs) {
  CfsCpu* h = new (std::nothrow) CfsCpu();
  if (!h) {
    set_error("fs_cfs_create: out of host memory");
    return FS_EOOM;
  }
  const int S = n_states;
  const int64_t P1 = p + 1;
  h->n = n, h->p = p, h->S = S, h->n_jobs = n_jobs;
  h->planes_route = S <= kPlaneStates;
  h->W = (n + 63) / 64;
  const int64_t W = h->W;
  try {
    h->colT.resize((size_t)P1 * n);
    if (h->planes_route) h->planes.assign((size_t)P1 * S * W, 0);
    h->kcol.assign((size_t)P1, 1);
    h->hcol.assign((size_t)P1, 0.0);
    h->r_cf.assign((size_t)p, 0.0f);
  } catch (const std::bad_alloc&) {
    delete h;
    set_error("fs_cfs_create: out of host memory for the column codes");
    return FS_EOOM;
  }
  std::atomic<int> bad{0};
  {
    // transpose, pack and take each column's entropy, in blocks of 64 columns
    const int64_t kBlock = 64;
    const int64_t tasks = (P1 + kBlock - 1) / kBlock;
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(hardware_threads(n_jobs), tasks));
    std::atomic<int64_t> next{0};
    run_threads(nt, [&]() {
      std::vector<int32_t> cnt((size_t)S);
      for (int64_t t = next++; t < tasks; t = next++) {
        const int64_t c0 = t * kBlock, c1 = std::min(P1, c0 + kBlock);
        for (int64_t i = 0; i < n; i++)
          for (int64_t c = c0; c < c1; c++)
            h->colT[(size_t)c * n + i] = c < p ? codes[(size_t)i * p + c] : ycodes[i];
        for (int64_t c = c0; c < c1; c++) {
          const uint8_t* col = &h->colT[(size_t)c * n];
          int mx = 0;
          for (int64_t i = 0; i < n; i++) mx = std::max<int>(mx, col[i]);
          if (mx >= S) {
            bad.store(1, std::memory_order_relaxed);
            continue;
          }
          h->kcol[c] = mx + 1;
          std::fill(cnt.begin(), cnt.end(), 0);
          for (int64_t i = 0; i < n; i++) cnt[col[i]]++;
          h->hcol[c] = cfs_entropy(cnt.data(), mx + 1, (double)n);
          if (h->planes_route)
            for (int64_t i = 0; i < n; i++)
              h->planes[((size_t)c * S + col[i]) * W + (i >> 6)] |= 1ull << (i & 63);
        }
      }
    });
  }
  if (bad.load()) {
    delete h;
    set_error("fs_cfs_create: a code is >= n_states");
    return FS_EINVAL;
  }
  h->compute_row(p, h->r_cf.data());  // the target is column p: the feature supplies the rows
  *out = h;
  return FS_OK;
}

int cfs_search_matrix(const float* r_cf, const float* r_ff, int64_t p, double min_r_cf,
                      int n_jobs, int64_t* selected, int64_t* n_selected, double* merits) {
  CpuStepper st;
  st.r_cf = r_cf, st.p = p, st.min_r_cf = min_r_cf, st.nt = hardware_threads(n_jobs);
  st.stride = p;
  st.base = [&]() { return r_ff; };
  st.add_row = [&](int64_t f, int64_t k) {
    st.rowof[k] = f;
    return (int)FS_OK;
  };
  return cfs_search_drive(st, r_cf, p, min_r_cf, selected, n_selected, merits);
}

}  // namespace cpu
}  // namespace fs
