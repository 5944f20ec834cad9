// fs_pairscan_labels_cpu.cpp -- the argument checks of fs_pair_screen_labels
// (both backends) and the CPU backend: the columns are packed once
// (mi_columns), then per labelling only y, column p, is written again, and the
// labelling runs cpu::pair_screen's own steps: rel_row, then joint_table and
// mi_from_table per pair, with the labelling's own class count, so the bits
// are those of a single call by construction.  The pair ranks are split into
// contiguous runs over host threads; a thread keeps one (key, rank) best of
// its run and the runs are merged under pair_beats, exact and independent of
// the split.
#include <algorithm>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "fs_pairscan.h"

namespace fs {

int pair_labels_check(int backend, const uint8_t* codes, const uint8_t* labels,
                      int64_t n_labelings, int64_t n, int64_t p, int n_states, int unit,
                      int score_kind, const double* best_score, const int64_t* best_i,
                      const int64_t* best_j) {
  const char* who = "fs_pair_screen_labels";
  if (!best_score || !best_i || !best_j) {
    set_error(std::string(who) + ": best_score, best_i and best_j must not be NULL");
    return FS_EINVAL;
  }
  if (int rc = jmi_check(who, backend, codes, labels, n, p, n_states, unit)) return rc;
  if (p < 2) {
    set_error(std::string(who) + ": p must be >= 2");
    return FS_EINVAL;
  }
  if (score_kind != kPairJoint && score_kind != kPairGain) {
    set_error(std::string(who) + ": score_kind must be 0 (joint) or 1 (gain)");
    return FS_EINVAL;
  }
  if (n_labelings < 1 || n_labelings > kPairMaxLabelings) {
    set_error(std::string(who) + ": n_labelings must be in 1.." +
              std::to_string(kPairMaxLabelings));
    return FS_EINVAL;
  }
  return FS_OK;
}

int pair_labels_classes(const uint8_t* labels, int64_t n_labelings, int64_t n, int n_states,
                        int& C) {
  const size_t total = (size_t)n_labelings * (size_t)n;
  // Eight bytes at a time: the OR of all codes bounds the largest from above
  // and shares its highest bit.  Below 4 that leaves one question, whether a 3
  // occurs where the OR is 3 (it may be 1 | 2): a byte <= 3 is 3 exactly when
  // its two low bits are both set.
  uint64_t any = 0, both = 0;
  size_t i = 0;
  for (; i + 8 <= total; i += 8) {
    uint64_t w;
    std::memcpy(&w, labels + i, 8);
    any |= w;
    both |= w & (w >> 1);
  }
  for (; i < total; i++) any |= labels[i], both |= (uint64_t)(labels[i] & (labels[i] >> 1));
  uint64_t o = any;
  o |= o >> 32, o |= o >> 16, o |= o >> 8;
  o &= 0xff;
  int mx;
  if (o < 4) {
    mx = o < 3 ? (int)o : ((both & 0x0101010101010101ull) ? 3 : 2);
  } else {  // a code above 3 occurs: the plain maximum
    mx = 0;
    for (i = 0; i < total; i++) mx = labels[i] > mx ? labels[i] : mx;
  }
  if (mx >= n_states) {
    set_error("fs_pair_screen_labels: a label code is >= n_states");
    return FS_EINVAL;
  }
  C = mx + 1;
  return FS_OK;
}

namespace cpu {

namespace {

// Labelling `y` into column p of packed columns: the codes, the state count
// and, on the planes route, the planes (mi_columns' layout, fs_mi.h).
void set_target(MiColumns& m, const uint8_t* y) {
  const int64_t n = m.n, p = m.p;
  uint8_t* col = &m.colT[(size_t)p * n];
  int mx = 0;
  for (int64_t i = 0; i < n; i++) col[i] = y[i], mx = std::max<int>(mx, y[i]);
  m.kcol[(size_t)p] = mx + 1;
  if (m.planes_route) {
    uint64_t* pl = &m.planes[(size_t)p * m.S * m.W];
    std::fill(pl, pl + (size_t)m.S * m.W, 0);
    for (int64_t i = 0; i < n; i++) pl[(size_t)col[i] * m.W + (i >> 6)] |= 1ull << (i & 63);
  }
}

}  // namespace

int pair_screen_labels(const uint8_t* codes, const uint8_t* labels, int n_labelings, int64_t n,
                       int64_t p, int n_states, int unit, int score_kind, int n_jobs,
                       double* best_score, int64_t* best_i, int64_t* best_j, double* relevance) {
  const char* who = "fs_pair_screen_labels";
  int Cmax = 0;
  if (int rc = pair_labels_classes(labels, n_labelings, n, n_states, Cmax)) return rc;
  MiColumns m;
  if (int rc = mi_columns(m, who, codes, labels, n, p, n_states, n_jobs)) return rc;
  // the largest joint table of any labelling
  int64_t cells = 0;
  {
    const int32_t k0 = m.kcol[(size_t)p];
    m.kcol[(size_t)p] = Cmax;
    const int rc = joint_cells(m, who, cells);
    m.kcol[(size_t)p] = k0;
    if (rc) return rc;
  }
  const int64_t total = pair_count(p);
  // a run of fewer than 256 pairs is not worth a thread of its own
  const int nt = (int)std::max<int64_t>(
      1, std::min<int64_t>(hardware_threads(n_jobs), (total + 255) / 256));
  std::vector<PairCand> best;
  std::vector<double> rel;
  try {
    best.resize((size_t)nt);
    rel.resize((size_t)p);
  } catch (const std::bad_alloc&) {
    set_error(std::string(who) + ": out of host memory");
    return FS_EOOM;
  }

  for (int b = 0; b < n_labelings; b++) {
    if (b > 0) set_target(m, labels + (size_t)b * n);
    double* relb = relevance ? relevance + (size_t)b * p : rel.data();
    rel_row(m, unit, n_jobs, relb);
    const int ky = m.kcol[(size_t)p];
    // thread w: the ranks [total * w / nt, total * (w + 1) / nt)
    auto work = [&](int w) {
      std::vector<int32_t> tab((size_t)cells);
      std::vector<double> p2((size_t)ky);
      PairCand bc{kPairNoKey, INT64_MAX};
      int64_t r = (int64_t)((__int128)total * w / nt);
      const int64_t r1 = (int64_t)((__int128)total * (w + 1) / nt);
      if (r < r1) {
        int64_t i, j;
        pair_unrank(p, r, i, j);
        for (; r < r1; r++) {
          joint_table(m, i, j, tab.data());
          const double jv =
              mi_from_table(tab.data(), ky, m.kcol[i] * m.kcol[j], ky, m.n, unit, p2.data());
          const uint64_t key = pair_key(pair_score_of(score_kind, jv, relb[i], relb[j]));
          if (pair_beats(key, r, bc.key, bc.rank)) bc.key = key, bc.rank = r;
          if (++j == p) i++, j = i + 1;
        }
      }
      best[(size_t)w] = bc;
    };
    std::vector<std::thread> th;
    for (int w = 1; w < nt; w++) th.emplace_back(work, w);
    work(0);
    for (auto& t : th) t.join();
    PairCand bc = best[0];
    for (int w = 1; w < nt; w++)
      if (pair_cand_beats(best[(size_t)w], bc)) bc = best[(size_t)w];
    best_score[b] = pair_score(bc.key);
    pair_unrank(p, bc.rank, best_i[b], best_j[b]);
  }
  return FS_OK;
}

}  // namespace cpu
}  // namespace fs
