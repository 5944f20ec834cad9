// fs_pairscan_cpu.cpp -- the argument checks of fs_pair_screen (both backends)
// and the CPU backend: the relevance, then every pair's joint relevance by the
// table and mi_from_table code of fs_jmi_cpu.cpp (joint_table, rel_row), the
// C(p,2) pair ranks split into contiguous runs over host threads.  A thread
// keeps a bounded list of the n_top best of its run (PairTopN, fs_pairscan.h)
// and its own array of per-feature maxima; the lists are merged under
// pair_beats and the maxima reduced by max, both exact and independent of the
// order, so the result is the same bits for every n_jobs.
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "fs_pairscan.h"

namespace fs {

int pair_check(int backend, const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p,
               int n_states, int unit, int score_kind, int64_t n_top, const double* relevance,
               const double* top_score, const int64_t* top_i, const int64_t* top_j) {
  if (!relevance || !top_score || !top_i || !top_j) {
    set_error("fs_pair_screen: relevance, top_score, top_i and top_j must not be NULL");
    return FS_EINVAL;
  }
  if (int rc = jmi_check("fs_pair_screen", backend, codes, ycodes, n, p, n_states, unit)) return rc;
  if (p < 2) {
    set_error("fs_pair_screen: p must be >= 2");
    return FS_EINVAL;
  }
  if (score_kind != kPairJoint && score_kind != kPairGain) {
    set_error("fs_pair_screen: score_kind must be 0 (joint) or 1 (gain)");
    return FS_EINVAL;
  }
  if (n_top < 1 || n_top > kPairMaxTop) {
    set_error("fs_pair_screen: n_top must be in 1.." + std::to_string(kPairMaxTop));
    return FS_EINVAL;
  }
  return FS_OK;
}

namespace cpu {

int pair_screen(const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p, int n_states,
                int unit, int score_kind, int n_top, int n_jobs, double* relevance,
                double* top_score, int64_t* top_i, int64_t* top_j, double* feature_best) {
  MiColumns m;
  if (int rc = mi_columns(m, "fs_pair_screen", codes, ycodes, n, p, n_states, n_jobs)) return rc;
  int64_t cells = 0;
  if (int rc = joint_cells(m, "fs_pair_screen", cells)) return rc;
  const int64_t total = pair_count(p);
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(hardware_threads(n_jobs), total));
  std::vector<PairTopN> tops;
  std::vector<std::vector<uint64_t>> best((size_t)nt);
  try {
    for (int w = 0; w < nt; w++) tops.emplace_back((size_t)n_top);
    if (feature_best)
      for (auto& b : best) b.assign((size_t)p, kPairNoKey);
  } catch (const std::bad_alloc&) {
    set_error("fs_pair_screen: out of host memory");
    return FS_EOOM;
  }
  rel_row(m, unit, n_jobs, relevance);

  const int ky = m.kcol[p];
  // thread w: the ranks [total * w / nt, total * (w + 1) / nt)
  auto work = [&](int w) {
    std::vector<int32_t> tab((size_t)cells);
    std::vector<double> p2((size_t)ky);
    PairTopN& top = tops[(size_t)w];
    uint64_t* fb = feature_best ? best[(size_t)w].data() : nullptr;
    int64_t r = (int64_t)((__int128)total * w / nt);
    const int64_t r1 = (int64_t)((__int128)total * (w + 1) / nt);
    if (r >= r1) return;
    int64_t i, j;
    pair_unrank(p, r, i, j);
    for (; r < r1; r++) {
      joint_table(m, i, j, tab.data());
      const double jv =
          mi_from_table(tab.data(), ky, m.kcol[i] * m.kcol[j], ky, m.n, unit, p2.data());
      const uint64_t key = pair_key(pair_score_of(score_kind, jv, relevance[i], relevance[j]));
      top.push(key, r);
      if (fb) {
        fb[i] = key > fb[i] ? key : fb[i];
        fb[j] = key > fb[j] ? key : fb[j];
      }
      if (++j == p) i++, j = i + 1;
    }
  };
  std::vector<std::thread> th;
  for (int w = 1; w < nt; w++) th.emplace_back(work, w);
  work(0);
  for (auto& t : th) t.join();

  for (int w = 1; w < nt; w++) tops[0].merge(tops[(size_t)w]);
  tops[0].sorted_into(p, top_score, top_i, top_j);
  if (feature_best)
    for (int64_t f = 0; f < p; f++) {
      uint64_t k = kPairNoKey;
      for (int w = 0; w < nt; w++) k = best[(size_t)w][(size_t)f] > k ? best[(size_t)w][(size_t)f] : k;
      feature_best[f] = pair_score(k);
    }
  return FS_OK;
}

}  // namespace cpu
}  // namespace fs
