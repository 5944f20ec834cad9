// fs_pairscan.h -- what the two backends of fs_pair_screen (fs_pairscan_cpu.cpp,
// fs_pairscan.hip) share: the score of a pair, the rank of a pair, the total
// order of the ranked list, and the bounded list that keeps the n_top best.
//
// For columns i < j, J(i, j) = I(X_i, X_j; y) is the joint relevance of
// fs_jmi.h (the table T[(a * kcol[j] + b)][c] through mi_from_table's steps),
// rel[f] = I(X_f; y) the relevance of fs_mi_matrices, and the score
//   score_kind 0, "joint":  J(i, j);
//   score_kind 1, "gain":   (J(i, j) - rel[i]) - rel[j], in float64 in that
//                           order: the interaction information, positive for
//                           synergy, negative for redundancy.
// The rank of a pair is its place in itertools.combinations(range(p), 2),
//   i * (2p - i - 1) / 2 + (j - i - 1),
// and the list is ordered by (score descending, rank ascending).  There is no
// closeness rule.
//
// Keys.  The order of the scores is carried by pair_key(), a map from a double
// to a uint64 that preserves <, so that the device can take maxima and compare
// against a threshold with integer instructions (no float atomics) and the host
// merge, the device and the CPU backend compare by one definition.  The two
// zeros are one value to ==, so they get one key: -0.0 is mapped as +0.0, and
// pair_score() gives +0.0 back.  (No score here is -0.0 in the first place: an
// MI sum starts at +0.0 and x - x is +0.0 in round-to-nearest; the map does not
// rely on it.)  Key 0 belongs to a NaN no score can be and means "none".
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/fastselect_amd.h"
#include "fs_internal.h"
#include "fs_jmi.h"

namespace fs {

constexpr int kPairJoint = 0, kPairGain = 1;
constexpr int kPairMaxTop = 65536;
constexpr uint64_t kPairNoKey = 0;

FS_HD inline double pair_score_of(int score_kind, double j, double rel_i, double rel_j) {
  return score_kind == kPairJoint ? j : (j - rel_i) - rel_j;
}

// a < b as doubles  <=>  pair_key(a) < pair_key(b);  a == b  <=>  equal keys.
FS_HD inline uint64_t pair_key(double v) {
  if (v == 0.0) v = 0.0;  // -0.0 and +0.0: one key
  uint64_t u;
#if defined(__HIP_DEVICE_COMPILE__)
  u = (uint64_t)__double_as_longlong(v);
#else
  std::memcpy(&u, &v, 8);
#endif
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
FS_HD inline double pair_score(uint64_t key) {
  const uint64_t u = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
  double v;
#if defined(__HIP_DEVICE_COMPILE__)
  v = __longlong_as_double((long long)u);
#else
  std::memcpy(&v, &u, 8);
#endif
  return v;
}

// The total order: the higher score, the lower rank among equal scores.
FS_HD inline bool pair_beats(uint64_t ka, int64_t ra, uint64_t kb, int64_t rb) {
  return ka > kb || (ka == kb && ra < rb);
}

FS_HD inline int64_t pair_count(int64_t p) { return p * (p - 1) / 2; }
// i * (2p - i - 1) is even for every i.
FS_HD inline int64_t pair_rank(int64_t p, int64_t i, int64_t j) {
  return i * (2 * p - i - 1) / 2 + (j - i - 1);
}
// The pair at rank r in 0..C(p,2)-1: a float estimate of the row, corrected by
// the integer expression.
FS_HD inline void pair_unrank(int64_t p, int64_t r, int64_t& i, int64_t& j) {
  const double m = 2.0 * (double)p - 1.0;
  int64_t a = (int64_t)((m - sqrt(m * m - 8.0 * (double)r)) * 0.5);
  a = a < 0 ? 0 : (a > p - 2 ? p - 2 : a);
  while (a > 0 && pair_rank(p, a, a + 1) > r) a--;
  while (a + 1 < p - 1 && pair_rank(p, a + 1, a + 2) <= r) a++;
  i = a;
  j = a + 1 + (r - pair_rank(p, a, a + 1));
}

struct PairCand {
  uint64_t key;
  int64_t rank;
};
inline bool pair_cand_beats(const PairCand& a, const PairCand& b) {
  return pair_beats(a.key, a.rank, b.key, b.rank);
}

// The n best candidates pushed so far under pair_beats.  The list holds up to
// 2n entries between compactions; once n are known, `thr` is the worst of
// them and a candidate that does not beat it is dropped at the door.  The
// best n of a set under a strict total order do not depend on the order of
// the pushes, so every split of the work gives the same list.
struct PairTopN {
  size_t n;
  std::vector<PairCand> v;
  bool full = false;
  PairCand thr{kPairNoKey, INT64_MAX};  // beaten by every candidate until `full`

  explicit PairTopN(size_t n_) : n(n_) { v.reserve(2 * n_); }
  void push(uint64_t key, int64_t rank) {
    if (full && !pair_beats(key, rank, thr.key, thr.rank)) return;
    v.push_back(PairCand{key, rank});
    if (v.size() >= 2 * n) compact();
  }
  // Down to the n best; sets the threshold once n are held.
  void compact() {
    if (v.size() < n) return;
    std::nth_element(v.begin(), v.begin() + (n - 1), v.end(), pair_cand_beats);
    v.resize(n);
    thr = v[n - 1];
    full = true;
  }
  void merge(const PairTopN& o) {
    for (const PairCand& c : o.v) push(c.key, c.rank);
  }
  // Best first into the caller's arrays of n entries; entries past the held
  // ones are score 0.0, i = j = -1.
  void sorted_into(int64_t p, double* score, int64_t* ti, int64_t* tj) {
    compact();
    std::sort(v.begin(), v.end(), pair_cand_beats);
    for (size_t t = 0; t < n; t++) {
      if (t < v.size()) {
        score[t] = pair_score(v[t].key);
        pair_unrank(p, v[t].rank, ti[t], tj[t]);
      } else {
        score[t] = 0.0, ti[t] = -1, tj[t] = -1;
      }
    }
  }
};

// Argument checks shared by both backends (the codes themselves are checked
// while they are packed).
int pair_check(int backend, const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p,
               int n_states, int unit, int score_kind, int64_t n_top, const double* relevance,
               const double* top_score, const int64_t* top_i, const int64_t* top_j);

// ---- fs_pair_screen_labels: the best pair of many labellings of y ----------
//
// Row b of the result is (top_score[0], top_i[0], top_j[0]) and the relevance
// of fs_pair_screen(codes, labels[b], n_top = 1) on the same backend, bit for
// bit.  Classes.  The class count C of a batch is the largest code over all
// rows plus one.  A class that a row does not take adds exact zeros to that
// row's tables: mi_pxy(0) = 0.0, p1 + 0.0 = p1, the class's p2 is 0.0 and
// used2 counts p2 > 0 only, mi_term(0.0, ., .) = 0.0 and sum + 0.0 = sum.  So
// a kernel may give every row C classes where a single call gives the row its
// own count, and the bits are the same (the argument fs_jmi.h makes for the
// states of a column).
constexpr int kPairMaxLabelings = 65535;

// Argument checks shared by both backends; they read no array.
int pair_labels_check(int backend, const uint8_t* codes, const uint8_t* labels,
                      int64_t n_labelings, int64_t n, int64_t p, int n_states, int unit,
                      int score_kind, const double* best_score, const int64_t* best_i,
                      const int64_t* best_j);
// C of the batch; FS_EINVAL for a label code >= n_states.
int pair_labels_classes(const uint8_t* labels, int64_t n_labelings, int64_t n, int n_states,
                        int& C);

namespace cpu {
int pair_screen(const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p, int n_states,
                int unit, int score_kind, int n_top, int n_jobs, double* relevance,
                double* top_score, int64_t* top_i, int64_t* top_j, double* feature_best);
// relevance: NULL or [n_labelings][p]
int pair_screen_labels(const uint8_t* codes, const uint8_t* labels, int n_labelings, int64_t n,
                       int64_t p, int n_states, int unit, int score_kind, int n_jobs,
                       double* best_score, int64_t* best_i, int64_t* best_j, double* relevance);
}
namespace gpu {
// What the GPU backend refuses without a device: FS_EOOM when the bit-planes of
// the shape fit no device (decided before any array is read), then FS_EINVAL
// for a y code >= n_states or more than kJmiMaxClassesGpu classes.
int pair_limits(const uint8_t* ycodes, int64_t n, int64_t p, int n_states);
int pair_screen(int device, const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p,
                int n_states, int unit, int score_kind, int n_top, double* relevance,
                double* top_score, int64_t* top_i, int64_t* top_j, double* feature_best);
// Milliseconds of the calling thread's last GPU pair_screen: upload, pack,
// relevance, scan with the selection, download (HIP events on the call's
// stream; the scan phase includes the host merges between its launches).
void pair_last_timing(double* ms5);
// fs_pairscan_labels.hip.  pair_labels_limits: FS_EOOM on the sizes alone,
// then FS_EINVAL for a label code >= n_states or more than kJmiMaxClassesGpu
// classes over all rows; needs no device.  `classes`: the class count of the
// batch, which pair_screen_labels takes back (the labels are read once).
int pair_labels_limits(const uint8_t* labels, int n_labelings, int64_t n, int64_t p, int n_states,
                       int* classes);
int pair_screen_labels(int device, const uint8_t* codes, const uint8_t* labels, int n_labelings,
                       int classes, int64_t n, int64_t p, int n_states, int unit, int score_kind,
                       double* best_score, int64_t* best_i, int64_t* best_j, double* relevance);
// Milliseconds of the calling thread's last GPU pair_screen_labels: upload,
// pack, relevance, scan with the reduction, download.
void pair_labels_last_timing(double* ms5);
#if defined(__HIPCC__)
// The general route of pair_screen_labels (more than 4 states): one labelling
// through pair_screen's own relevance kernel and scan on planes the caller
// packed (fs_pairscan.hip).  `y` (device, n codes) is packed into column p
// first; best: the labelling's first pair under pair_beats.
struct DevArena;
struct MiPlanes;
struct PairScanBufs {
  double* rel = nullptr;          // p
  PairCand* cand = nullptr;       // cap
  unsigned int* cursor = nullptr; // 1
  int64_t cap = 0;
  std::vector<PairCand> host;     // cap
};
int pair_scan_geometry(MiPlanes& pl, const char* who, int64_t n, int64_t p, int n_states, int& T,
                       int& CPW);
int pair_scan_bufs(DevArena& mem, int64_t p, int n_top, PairScanBufs& b);
int pair_repack_y(const MiPlanes& pl, const uint8_t* y, hipStream_t s);
int pair_rel_launch(const MiPlanes& pl, int CPW, int unit, double* drel, hipStream_t s);
int pair_scan_planes(const MiPlanes& pl, int C, int T, int unit, int score_kind, int n_top,
                     unsigned long long* dfb, PairScanBufs& b, PairTopN& top, hipStream_t s);
#endif
}

}  // namespace fs
