// fs_mdr.h -- what the two MDR backends (fs_mdr_cpu.cpp, fs_mdr.hip) share:
// combination ranks, the sample layout and the balanced-accuracy epilogue.
//
// MDR (the reference's MDR.py) scores every k-combination of p SNP columns
// (genotypes 0/1/2) by the balanced accuracy of its 3^k-cell high/low-risk
// table.  Here a genotype column is three bit-planes over the samples, a
// cell count is popcount(AND of k planes), and the samples are permuted so
// that every (class, test fold) *segment* is a contiguous, word-aligned run:
// one walk over the words yields each fold's own counts, and a fold's
// training counts are the totals minus its own.  Every quantity is an
// integer until the three float64 operations of mdr_ba().
#pragma once

#include <cstdint>
#include <vector>

#include "fs_internal.h"

namespace fs {

constexpr int kMdrMaxK = 6;
constexpr int64_t kMdrMaxN = (int64_t)1 << 25;       // the integer risk test is exact below
constexpr int64_t kMdrMaxCount = (int64_t)1 << 62;   // C(p,k) above this is rejected
constexpr int64_t kMdrNoRank = INT64_MAX;

// c * m / d for a product that is known to be divisible by d (d <= 6),
// without overflowing where the result fits.
FS_HD inline uint64_t mdr_muldiv(uint64_t c, uint64_t m, uint64_t d) {
  return (c / d) * m + (c % d) * m / d;
}

// C(m, j) for 0 <= j <= 6; 0 when m < j.  Exact while the result is below
// 2^62 (the callers only evaluate it for m <= p, j <= k with C(p,k) checked).
// The loop is unrolled so that every divisor is a constant.
FS_HD inline uint64_t mdr_binom(int64_t m, int j) {
  if (m < j) return 0;
  uint64_t c = 1;
#if defined(__clang__)
#pragma unroll
#endif
  for (int i = 0; i < kMdrMaxK; i++)
    if (i < j) c = mdr_muldiv(c, (uint64_t)(m - i), (uint64_t)(i + 1));
  return c;
}

// C(p,k) into *count; false when it exceeds 2^62 (or the arguments are bad).
inline bool mdr_count(int64_t p, int k, int64_t* count) {
  if (k < 0 || k > kMdrMaxK || p < k) return false;
  long double c = 1.0L;
  for (int i = 0; i < k; i++) c = c * (long double)(p - i) / (long double)(i + 1);
  if (c > (long double)kMdrMaxCount) return false;
  *count = (int64_t)mdr_binom(p, k);
  return true;
}

// rank (itertools.combinations order over range(p)) -> ascending indices.
// Position t takes the largest a with #(combinations whose t-th element is
// below a) <= the remaining rank, found by bisection on C(p - a, j).
FS_HD inline void mdr_unrank(int64_t p, int k, int64_t rank, int32_t* f) {
  uint64_t r = (uint64_t)rank;
  int64_t lo = 0;
  for (int t = 0; t < k; t++) {
    const int j = k - t;
    if (j == 1) {
      f[t] = (int32_t)(lo + (int64_t)r);
      return;
    }
    const uint64_t all = mdr_binom(p - lo, j);
    int64_t a = lo, b = p - j;  // invariant: the answer lies in [a, b]
    while (a < b) {
      const int64_t mid = a + (b - a + 1) / 2;
      if (all - mdr_binom(p - mid, j) <= r) a = mid; else b = mid - 1;
    }
    r -= all - mdr_binom(p - a, j);
    f[t] = (int32_t)a;
    lo = a + 1;
  }
}

// The next combination in the same order (f is not the last one).
FS_HD inline void mdr_next(int64_t p, int k, int32_t* f) {
  int t = k - 1;
  while (t > 0 && f[t] == p - k + t) t--;
  f[t]++;
  for (int u = t + 1; u < k; u++) f[u] = f[u - 1] + 1;
}

// `step` combinations further (the result exists).  The last column moves
// by step; each time it runs past p - 1 the leading k-1 columns, a
// combination of range(p - 1), step once and the rest carries into their row.
FS_HD inline void mdr_advance(int64_t p, int k, int32_t* f, int64_t step) {
  int64_t last = f[k - 1] + step;
  while (k > 1 && last > p - 1) {
    const int64_t over = last - p;
    mdr_next(p - 1, k - 1, f);
    last = f[k - 2] + 1 + over;
  }
  f[k - 1] = (int32_t)last;
}

// High risk (MDR.py:66-75): no controls in the cell, or case / control >
// total_case / total_control, as the integer test that equals the float64
// comparison for n < 2^25 (two distinct ratios of integers <= n differ by
// more than an ulp; equal ratios round equally).
FS_HD inline bool mdr_high_risk(uint32_t cs, uint32_t ct, uint64_t tc, uint64_t tn) {
  return ct == 0 || (uint64_t)cs * tn > (uint64_t)ct * tc;
}

// (tp / total_case + tn / total_control) / 2.0 in float64, rounded to
// float32 (MDR.py:77-79, 125-127); 0 without training cases or controls.
FS_HD inline float mdr_ba(uint64_t tp, uint64_t tn, uint64_t tc, uint64_t tctl) {
  if (tc == 0 || tctl == 0) return 0.0f;
  const double sens = (double)tp / (double)tc;
  const double spec = (double)tn / (double)tctl;
  return (float)((sens + spec) / 2.0);
}

// (ba bits, rank) a beats b: larger BA (non-negative floats order as their
// bit patterns), then the smaller rank.
FS_HD inline bool mdr_better(uint32_t ba, int64_t ra, uint32_t bb, int64_t rb) {
  return ba > bb || (ba == bb && ra < rb);
}

// Sample layout.  Segment s = c * F + f holds the samples of class c (0 =
// case, 1 = control) whose test fold is f, padded to whole words; perm maps
// bit position -> sample index (-1 = padding).  Without folds F = 1 and
// nothing is subtracted: the one scan trains on every sample.
struct MdrLayout {
  int F = 1;
  int sub = 0;                    // 1: fold f trains on totals minus segment f
  int64_t words = 0;
  std::vector<int32_t> perm;      // words * wordbits
  std::vector<int32_t> seg_off;   // 2F + 1, in words
  std::vector<int64_t> tc, tn;    // F: training cases / controls of fold f
};

// FS_EINVAL (with the error set) for a fold id outside [0, n_folds).
int mdr_layout(int64_t n, const uint8_t* is_case, const int32_t* fold, int n_folds, int wordbits,
               MdrLayout& L);

// Argument checks of fs_mdr_scan shared by both backends; *count = C(p,k).
int mdr_check(const uint8_t* x, int64_t n, int64_t p, const uint8_t* is_case, int k,
              const int32_t* fold, int n_folds, const float* best_ba, const int64_t* best_rank,
              int64_t* count);

// fs_mdr_scan_labels: many labellings of one genotype matrix.  The class is
// not part of this layout: segment f holds every sample whose test fold is f,
// padded to whole words (seg_off has F + 1 entries; tc / tn stay empty).  A
// cell's cases in fold f under labelling b are popcount(cell & label words of
// b) over f's words and its controls are the cell's count minus that: the
// same integers as the (class, fold) layout gives, so the same BA bits.
constexpr int kMdrMaxLabelings = 65535;

int mdr_fold_layout(int64_t n, const int32_t* fold, int n_folds, int wordbits, MdrLayout& L);

// Training cases / controls of fold f under labelling b, at [f * n_labelings + b].
void mdr_label_totals(int64_t n, const uint8_t* labels, int n_labelings, const MdrLayout& L,
                      int n_jobs, std::vector<uint32_t>& tc, std::vector<uint32_t>& tn);

// The checks of mdr_check plus those on the labellings.
int mdr_check_labels(const uint8_t* x, int64_t n, int64_t p, const uint8_t* labels,
                     int n_labelings, int k, const int32_t* fold, int n_folds,
                     const float* best_ba, const int64_t* best_rank, int64_t* count);

// fs_mdr_scan_top: the n_top best combinations of every fold under
// mdr_better's order.  kMdrMaxTop bounds the lists both backends keep (a heap
// per host thread and fold; on the GPU the candidate buffers hold n_top plus
// one histogram bin's population); it is a buffer limit, not a measurement.
constexpr int kMdrMaxTop = 4096;

struct MdrCand {
  uint32_t bits;
  int64_t rank;
};
inline bool mdr_cand_before(const MdrCand& a, const MdrCand& b) {
  return mdr_better(a.bits, a.rank, b.bits, b.rank);
}

// The best `n` candidates pushed so far: a heap with the worst kept on top.
// (bits, rank) is a total order, so the result does not depend on push order.
struct MdrTopN {
  size_t n = 0;
  std::vector<MdrCand> h;
  explicit MdrTopN(size_t n_) : n(n_) { h.reserve(n_); }
  bool full() const { return h.size() >= n; }
  const MdrCand& worst() const { return h.front(); }
  void push(MdrCand c);
  // best first into ba[0..n_top) / rank[0..n_top); unused entries 0 / -1
  void sorted_into(float* ba, int64_t* rank, int n_top);
};

// The histogram of the GPU's first scan.  A training BA is 0 or lies in
// [0.5, 1], so bits >> 14 takes 513 values there: bin 0 holds every BA below
// 0.5, bin b >= 1 the BAs whose bits >> 14 is kMdrBinBase + b - 1.
constexpr uint32_t kMdrBinShift = 14;
constexpr uint32_t kMdrBinBase = 0x3F000000u >> kMdrBinShift;
constexpr int kMdrBins = (int)((0x3F800000u >> kMdrBinShift) - kMdrBinBase) + 2;
FS_HD inline uint32_t mdr_bin(uint32_t bits) {
  const uint32_t h = bits >> kMdrBinShift;
  if (h < kMdrBinBase) return 0;
  const uint32_t b = h - kMdrBinBase + 1;
  return b < (uint32_t)kMdrBins ? b : (uint32_t)kMdrBins - 1;
}
// the smallest bit pattern of bin b
FS_HD inline uint32_t mdr_bin_floor(uint32_t b) {
  return b == 0 ? 0u : (b - 1 + kMdrBinBase) << kMdrBinShift;
}
// The highest bin whose suffix count reaches `need` (1 <= need <= the
// histogram's total) and that suffix count: the number of BAs at or above
// the bin's floor.
void mdr_top_threshold(const uint64_t* hist, uint64_t need, uint32_t* bin, uint64_t* suffix);

namespace cpu {
int mdr_scan(const uint8_t* x, int64_t n, int64_t p, const uint8_t* is_case, int k,
             const int32_t* fold, int n_folds, int n_jobs, int64_t count, float* best_ba,
             int64_t* best_rank, float* ba_out);
int mdr_scan_top(const uint8_t* x, int64_t n, int64_t p, const uint8_t* is_case, int k,
                 const int32_t* fold, int n_folds, int n_jobs, int64_t count, int n_top,
                 float* top_ba, int64_t* top_rank);
int mdr_scan_labels(const uint8_t* x, int64_t n, int64_t p, const uint8_t* labels,
                    int n_labelings, int k, const int32_t* fold, int n_folds, int n_jobs,
                    int64_t count, float* best_ba, int64_t* best_rank, float* ba_out);
}
namespace gpu {
int mdr_scan(int device, const uint8_t* x, int64_t n, int64_t p, const uint8_t* is_case, int k,
             const int32_t* fold, int n_folds, int64_t count, float* best_ba, int64_t* best_rank,
             float* ba_out);
int mdr_scan_labels(int device, const uint8_t* x, int64_t n, int64_t p, const uint8_t* labels,
                    int n_labelings, int k, const int32_t* fold, int n_folds, int64_t count,
                    float* best_ba, int64_t* best_rank, float* ba_out);
// Milliseconds of the calling thread's last GPU mdr_scan_labels: upload, pack,
// scan with the reduction, download (HIP events on the call's stream).
void mdr_labels_last_timing(double* ms4);
int mdr_scan_top(int device, const uint8_t* x, int64_t n, int64_t p, const uint8_t* is_case,
                 int k, const int32_t* fold, int n_folds, int64_t count, int n_top, float* top_ba,
                 int64_t* top_rank);
// The same four phases of the last GPU mdr_scan_top; the scan phase holds both
// scans, the threshold search between them and the selection.
void mdr_top_last_timing(double* ms4);
}

}  // namespace fs
