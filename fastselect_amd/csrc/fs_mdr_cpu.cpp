// fs_mdr_cpu.cpp -- MDR's sample layout and argument checks (both backends)
// and the CPU backend of fs_mdr_scan: the bit-plane / popcount scheme of
// fs_mdr.h on 64-bit words, the rank range split over host threads.  It
// replaces _batch_balanced_accuracy_cpu (MDR.py:82-129) for all folds at once.
// fs_mdr_scan_labels (many labellings of one genotype matrix) follows the
// same scheme on the fold-only layout: a combination's cell masks are built
// once and every labelling adds one AND and one popcount per word.
// fs_mdr_scan_top runs fs_mdr_scan's loop and keeps a bounded heap of the
// n_top best (BA bits, rank) per thread and fold, merged at the end; the heap
// and the histogram threshold search of the GPU backend live here too.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <thread>

#include "../../include/fastselect_amd.h"
#include "fs_mdr.h"

namespace fs {

int mdr_layout(int64_t n, const uint8_t* is_case, const int32_t* fold, int n_folds, int wordbits,
               MdrLayout& L) {
  const int F = fold ? n_folds : 1;
  L.F = F;
  L.sub = fold ? 1 : 0;
  std::vector<int64_t> size(2 * (size_t)F, 0);
  for (int64_t i = 0; i < n; i++) {
    const int f = fold ? fold[i] : 0;
    if (f < 0 || f >= F) {
      set_error("fs_mdr_scan: fold id outside [0, n_folds)");
      return FS_EINVAL;
    }
    size[(size_t)(is_case[i] ? 0 : 1) * F + f]++;
  }
  L.seg_off.assign(2 * (size_t)F + 1, 0);
  int64_t w = 0;
  for (int s = 0; s < 2 * F; s++) {
    L.seg_off[s] = (int32_t)w;
    w += (size[s] + wordbits - 1) / wordbits;
  }
  L.seg_off[2 * F] = (int32_t)w;
  L.words = w;
  L.perm.assign((size_t)w * wordbits, -1);
  std::vector<int64_t> fill(2 * (size_t)F);
  for (int s = 0; s < 2 * F; s++) fill[s] = (int64_t)L.seg_off[s] * wordbits;
  for (int64_t i = 0; i < n; i++) {
    const size_t s = (size_t)(is_case[i] ? 0 : 1) * F + (fold ? fold[i] : 0);
    L.perm[fill[s]++] = (int32_t)i;
  }
  int64_t cases = 0;
  for (int f = 0; f < F; f++) cases += size[f];
  L.tc.resize(F);
  L.tn.resize(F);
  for (int f = 0; f < F; f++) {
    L.tc[f] = cases - (L.sub ? size[f] : 0);
    L.tn[f] = (n - cases) - (L.sub ? size[(size_t)F + f] : 0);
  }
  return FS_OK;
}

int mdr_check(const uint8_t* x, int64_t n, int64_t p, const uint8_t* is_case, int k,
              const int32_t* fold, int n_folds, const float* best_ba, const int64_t* best_rank,
              int64_t* count) {
  if (!x || !is_case || !best_ba || !best_rank) {
    set_error("fs_mdr_scan: x, is_case, best_ba and best_rank must not be NULL");
    return FS_EINVAL;
  }
  if (k < 1 || k > kMdrMaxK) {
    set_error("fs_mdr_scan: k must be in 1..6");
    return FS_EINVAL;
  }
  if (n < 1 || n >= kMdrMaxN) {
    set_error("fs_mdr_scan: n must be in [1, 2^25)");
    return FS_EINVAL;
  }
  if (p < k) {
    set_error("fs_mdr_scan: k must be <= the number of columns");
    return FS_EINVAL;
  }
  if ((fold == nullptr) != (n_folds == 0) || n_folds < 0 || n_folds > n) {
    set_error("fs_mdr_scan: fold and n_folds go together (NULL and 0, or ids and 1..n)");
    return FS_EINVAL;
  }
  if (!mdr_count(p, k, count)) {
    set_error("fs_mdr_scan: C(p,k) exceeds 2^62");
    return FS_EINVAL;
  }
  return FS_OK;
}

void MdrTopN::push(MdrCand c) {
  if (h.size() < n) {
    h.push_back(c);
    std::push_heap(h.begin(), h.end(), mdr_cand_before);
  } else if (n > 0 && mdr_cand_before(c, h.front())) {
    std::pop_heap(h.begin(), h.end(), mdr_cand_before);
    h.back() = c;
    std::push_heap(h.begin(), h.end(), mdr_cand_before);
  }
}

void MdrTopN::sorted_into(float* ba, int64_t* rank, int n_top) {
  std::sort_heap(h.begin(), h.end(), mdr_cand_before);  // ascending: the best first
  for (int j = 0; j < n_top; j++) {
    const bool have = (size_t)j < h.size();
    const uint32_t bits = have ? h[j].bits : 0u;
    std::memcpy(&ba[j], &bits, 4);
    rank[j] = have ? h[j].rank : -1;
  }
}

void mdr_top_threshold(const uint64_t* hist, uint64_t need, uint32_t* bin, uint64_t* suffix) {
  uint64_t sum = 0;
  int b = kMdrBins;
  while (b > 0 && sum < need) sum += hist[--b];
  *bin = (uint32_t)b;
  *suffix = sum;
}

int mdr_fold_layout(int64_t n, const int32_t* fold, int n_folds, int wordbits, MdrLayout& L) {
  const int F = fold ? n_folds : 1;
  L.F = F;
  L.sub = fold ? 1 : 0;
  L.tc.clear();
  L.tn.clear();
  std::vector<int64_t> size((size_t)F, 0);
  for (int64_t i = 0; i < n; i++) {
    const int f = fold ? fold[i] : 0;
    if (f < 0 || f >= F) {
      set_error("fs_mdr_scan_labels: fold id outside [0, n_folds)");
      return FS_EINVAL;
    }
    size[f]++;
  }
  L.seg_off.assign((size_t)F + 1, 0);
  int64_t w = 0;
  for (int f = 0; f < F; f++) {
    L.seg_off[f] = (int32_t)w;
    w += (size[f] + wordbits - 1) / wordbits;
  }
  L.seg_off[F] = (int32_t)w;
  L.words = w;
  L.perm.assign((size_t)w * wordbits, -1);
  std::vector<int64_t> fill((size_t)F);
  for (int f = 0; f < F; f++) fill[f] = (int64_t)L.seg_off[f] * wordbits;
  for (int64_t i = 0; i < n; i++) L.perm[fill[fold ? fold[i] : 0]++] = (int32_t)i;
  return FS_OK;
}

void mdr_label_totals(int64_t n, const uint8_t* labels, int n_labelings, const MdrLayout& L,
                      int n_jobs, std::vector<uint32_t>& tc, std::vector<uint32_t>& tn) {
  const int F = L.F;
  const size_t B = (size_t)n_labelings;
  tc.assign((size_t)F * B, 0);
  tn.assign((size_t)F * B, 0);
  // the samples in layout order, fold by fold: a fold's cases are one
  // branch-free sum over its run (random flags would mispredict every second
  // branch of a test per sample)
  const int64_t wordbits = L.words ? (int64_t)L.perm.size() / L.words : 0;
  std::vector<int32_t> order;
  std::vector<int64_t> start((size_t)F + 1, 0);
  order.reserve((size_t)n);
  for (int f = 0; f < F; f++) {
    for (int64_t pos = L.seg_off[f] * wordbits; pos < L.seg_off[f + 1] * wordbits; pos++)
      if (L.perm[pos] >= 0) order.push_back(L.perm[pos]);
    start[f + 1] = (int64_t)order.size();
  }
  auto rows = [&](size_t b0, size_t b1) {
    std::vector<uint32_t> in((size_t)F);
    for (size_t b = b0; b < b1; b++) {
      const uint8_t* lab = labels + b * (size_t)n;
      uint32_t cases = 0;
      for (int f = 0; f < F; f++) {
        uint32_t c = 0;
        for (int64_t j = start[f]; j < start[f + 1]; j++) c += lab[order[j]] != 0;
        in[f] = c;
        cases += c;
      }
      for (int f = 0; f < F; f++) {
        const uint32_t size = (uint32_t)(start[f + 1] - start[f]);
        tc[(size_t)f * B + b] = cases - (L.sub ? in[f] : 0);
        tn[(size_t)f * B + b] = ((uint32_t)n - cases) - (L.sub ? size - in[f] : 0);
      }
    }
  };
  // one thread per 2^18 flags, eight at most: the work is a few milliseconds
  const int nt = (int)std::max<int64_t>(
      1, std::min<int64_t>({(int64_t)hardware_threads(n_jobs), 8, (int64_t)(B * (size_t)n >> 18),
                            (int64_t)B}));
  std::vector<std::thread> th;
  for (int t = 1; t < nt; t++) th.emplace_back(rows, B * t / nt, B * (t + 1) / nt);
  rows(0, B / nt);
  for (auto& t : th) t.join();
}

int mdr_check_labels(const uint8_t* x, int64_t n, int64_t p, const uint8_t* labels,
                     int n_labelings, int k, const int32_t* fold, int n_folds,
                     const float* best_ba, const int64_t* best_rank, int64_t* count) {
  if (!x || !labels || !best_ba || !best_rank) {
    set_error("fs_mdr_scan_labels: x, labels, best_ba and best_rank must not be NULL");
    return FS_EINVAL;
  }
  if (n_labelings < 1 || n_labelings > kMdrMaxLabelings) {
    set_error("fs_mdr_scan_labels: n_labelings must be in 1..65535");
    return FS_EINVAL;
  }
  return mdr_check(x, n, p, labels, k, fold, n_folds, best_ba, best_rank, count);
}

namespace cpu {

namespace {

// planes[(j * 3 + g) * W + w]: bit b of word w is set iff the sample at
// position w * 64 + b of the layout has genotype g in column j.
int pack_planes(const uint8_t* x, int64_t p, const MdrLayout& L, int n_jobs,
                std::vector<uint64_t>& planes) {
  const int64_t W = L.words;
  planes.assign((size_t)p * 3 * W, 0);
  std::atomic<int> bad{0};
  const int64_t kBlock = 64;  // columns per task
  const int64_t tasks = (p + kBlock - 1) / kBlock;
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(hardware_threads(n_jobs), tasks));
  std::atomic<int64_t> next{0};
  auto work = [&]() {
    for (int64_t t = next++; t < tasks; t = next++) {
      const int64_t j0 = t * kBlock, j1 = std::min(p, j0 + kBlock);
      bool b = false;
      for (int64_t pos = 0; pos < W * 64; pos++) {
        const int32_t i = L.perm[pos];
        if (i < 0) continue;
        const uint8_t* row = x + (size_t)i * p;
        const uint64_t bit = 1ull << (pos & 63);
        for (int64_t j = j0; j < j1; j++) {
          const uint8_t g = row[j];
          if (g > 2) { b = true; continue; }
          planes[((size_t)j * 3 + g) * W + (pos >> 6)] |= bit;
        }
      }
      if (b) bad.store(1, std::memory_order_relaxed);
    }
  };
  std::vector<std::thread> th;
  for (int w = 1; w < nt; w++) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
  if (bad.load()) {
    set_error("fs_mdr_scan: genotypes must be coded 0/1/2");
    return FS_EINVAL;
  }
  return FS_OK;
}

struct Best {
  uint32_t bits = 0;
  int64_t rank = kMdrNoRank;
};

// The scan is popcounts: on x86-64 the build's baseline has no popcnt
// instruction, so the loop is compiled twice and the call picks the hardware
// one where the CPU has it (every x86-64 CPU of the last decade).
#if defined(__x86_64__) && defined(__GNUC__)
#define FS_MDR_POPCNT __attribute__((target("popcnt")))
inline bool have_popcnt() { return __builtin_cpu_supports("popcnt"); }
#else
#define FS_MDR_POPCNT
inline bool have_popcnt() { return false; }
#endif

// One combination: tp / tn of every fold.  cnt is 3 x 2F scratch.
template <bool HW>
__attribute__((always_inline)) inline void scan_one(const uint64_t* planes, int64_t W, const MdrLayout& L, int k,
                     const int32_t* f, uint32_t* cnt, uint64_t* tp, uint64_t* tn) {
  const int F = L.F, S = 2 * F;
  int cells = 1;
  for (int t = 1; t < k; t++) cells *= 3;
  for (int i = 0; i < F; i++) tp[i] = tn[i] = 0;
  const uint64_t* last = planes + (size_t)f[k - 1] * 3 * W;
  const uint64_t* pre[kMdrMaxK];
  for (int cell = 0; cell < cells; cell++) {
    for (int t = k - 2, c = cell; t >= 0; t--, c /= 3)
      pre[t] = planes + ((size_t)f[t] * 3 + c % 3) * W;
    uint32_t tot[3][2] = {{0, 0}, {0, 0}, {0, 0}};
    for (int s = 0; s < S; s++) {
      uint32_t a0 = 0, a1 = 0, a2 = 0;
      for (int64_t w = L.seg_off[s]; w < L.seg_off[s + 1]; w++) {
        uint64_t m = ~0ull;
        for (int t = 0; t < k - 1; t++) m &= pre[t][w];
        a0 += (uint32_t)__builtin_popcountll(m & last[w]);
        a1 += (uint32_t)__builtin_popcountll(m & last[W + w]);
        a2 += (uint32_t)__builtin_popcountll(m & last[2 * W + w]);
      }
      cnt[s] = a0, cnt[S + s] = a1, cnt[2 * S + s] = a2;
      const int c = s >= F;
      tot[0][c] += a0, tot[1][c] += a1, tot[2][c] += a2;
    }
    for (int g = 0; g < 3; g++)
      for (int i = 0; i < F; i++) {
        const uint32_t cs = tot[g][0] - (L.sub ? cnt[g * S + i] : 0);
        const uint32_t ct = tot[g][1] - (L.sub ? cnt[g * S + F + i] : 0);
        if (mdr_high_risk(cs, ct, (uint64_t)L.tc[i], (uint64_t)L.tn[i])) tp[i] += cs;
        else tn[i] += ct;
      }
  }
}

using ScanFn = void (*)(const uint64_t*, int64_t, const MdrLayout&, int, const int32_t*, uint32_t*,
                        uint64_t*, uint64_t*);
void scan_one_sw(const uint64_t* planes, int64_t W, const MdrLayout& L, int k, const int32_t* f,
                 uint32_t* cnt, uint64_t* tp, uint64_t* tn) {
  scan_one<false>(planes, W, L, k, f, cnt, tp, tn);
}
FS_MDR_POPCNT void scan_one_hw(const uint64_t* planes, int64_t W, const MdrLayout& L, int k,
                               const int32_t* f, uint32_t* cnt, uint64_t* tp, uint64_t* tn) {
  scan_one<true>(planes, W, L, k, f, cnt, tp, tn);
}

// What one thread of the labels scan keeps between combinations.
struct LabelScratch {
  std::vector<uint64_t> mask;       // 3 x W: a prefix cell ANDed with the last column
  std::vector<uint32_t> cell, own;  // 3 x F cell counts; F case counts
  std::vector<uint32_t> tp, tn;     // B x F
};

// One combination under every labelling: tp / tn at [b * F + fold].  A prefix
// cell's three mask rows and their per-fold counts are built once and serve
// all B labellings; per labelling only popcount(mask & label word) is left.
template <bool HW>
__attribute__((always_inline)) inline void scan_labels_one(
    const uint64_t* planes, int64_t W, const MdrLayout& L, int k, const int32_t* f,
    const uint64_t* Y, int B, const uint32_t* tc, const uint32_t* tn, LabelScratch& s) {
  const int F = L.F;
  int cells = 1;
  for (int t = 1; t < k; t++) cells *= 3;
  std::fill(s.tp.begin(), s.tp.end(), 0u);
  std::fill(s.tn.begin(), s.tn.end(), 0u);
  const uint64_t* last = planes + (size_t)f[k - 1] * 3 * W;
  const uint64_t* pre[kMdrMaxK];
  for (int cell = 0; cell < cells; cell++) {
    for (int t = k - 2, c = cell; t >= 0; t--, c /= 3)
      pre[t] = planes + ((size_t)f[t] * 3 + c % 3) * W;
    uint32_t ctot[3] = {0, 0, 0};
    for (int g = 0; g < 3; g++)
      for (int i = 0; i < F; i++) {
        uint32_t a = 0;
        for (int64_t w = L.seg_off[i]; w < L.seg_off[i + 1]; w++) {
          uint64_t m = last[g * W + w];
          for (int t = 0; t < k - 1; t++) m &= pre[t][w];
          s.mask[g * W + w] = m;
          a += (uint32_t)__builtin_popcountll(m);
        }
        s.cell[g * F + i] = a;
        ctot[g] += a;
      }
    for (int b = 0; b < B; b++) {
      const uint64_t* y = Y + (size_t)b * W;
      for (int g = 0; g < 3; g++) {
        const uint64_t* m = s.mask.data() + g * W;
        uint32_t tot = 0;
        for (int i = 0; i < F; i++) {
          uint32_t a = 0;
          for (int64_t w = L.seg_off[i]; w < L.seg_off[i + 1]; w++)
            a += (uint32_t)__builtin_popcountll(m[w] & y[w]);
          s.own[i] = a;
          tot += a;
        }
        for (int i = 0; i < F; i++) {
          const uint32_t cs = tot - (L.sub ? s.own[i] : 0);
          const uint32_t ct = (ctot[g] - tot) - (L.sub ? s.cell[g * F + i] - s.own[i] : 0);
          const size_t o = (size_t)i * B + b;
          if (mdr_high_risk(cs, ct, tc[o], tn[o])) s.tp[(size_t)b * F + i] += cs;
          else s.tn[(size_t)b * F + i] += ct;
        }
      }
    }
  }
}

using LabelScanFn = void (*)(const uint64_t*, int64_t, const MdrLayout&, int, const int32_t*,
                             const uint64_t*, int, const uint32_t*, const uint32_t*,
                             LabelScratch&);
void scan_labels_one_sw(const uint64_t* planes, int64_t W, const MdrLayout& L, int k,
                        const int32_t* f, const uint64_t* Y, int B, const uint32_t* tc,
                        const uint32_t* tn, LabelScratch& s) {
  scan_labels_one<false>(planes, W, L, k, f, Y, B, tc, tn, s);
}
FS_MDR_POPCNT void scan_labels_one_hw(const uint64_t* planes, int64_t W, const MdrLayout& L, int k,
                                      const int32_t* f, const uint64_t* Y, int B,
                                      const uint32_t* tc, const uint32_t* tn, LabelScratch& s) {
  scan_labels_one<true>(planes, W, L, k, f, Y, B, tc, tn, s);
}

}  // namespace

int mdr_scan_labels(const uint8_t* x, int64_t n, int64_t p, const uint8_t* labels,
                    int n_labelings, int k, const int32_t* fold, int n_folds, int n_jobs,
                    int64_t count, float* best_ba, int64_t* best_rank, float* ba_out) {
  MdrLayout L;
  if (int rc = mdr_fold_layout(n, fold, n_folds, 64, L)) return rc;
  const int F = L.F, B = n_labelings;
  const int64_t W = L.words;
  std::vector<uint64_t> planes, Y;
  std::vector<uint32_t> tc, tn;
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(hardware_threads(n_jobs), count));
  std::vector<std::vector<Best>> best((size_t)nt);
  try {
    if (int rc = pack_planes(x, p, L, n_jobs, planes)) return rc;
    Y.assign((size_t)B * W, 0);
    for (int b = 0; b < B; b++) {
      const uint8_t* lab = labels + (size_t)b * n;
      for (int64_t w = 0; w < W; w++) {
        uint64_t bits = 0;
        for (int i = 0; i < 64; i++) {
          const int32_t s = L.perm[w * 64 + i];
          bits |= (uint64_t)(s >= 0 && lab[s >= 0 ? s : 0] != 0) << i;
        }
        Y[(size_t)b * W + w] = bits;
      }
    }
    mdr_label_totals(n, labels, B, L, n_jobs, tc, tn);
    for (auto& v : best) v.assign((size_t)B * F, Best());
  } catch (const std::bad_alloc&) {
    set_error("fs_mdr_scan_labels: out of host memory for the bit-planes");
    return FS_EOOM;
  }
  const LabelScanFn scan = have_popcnt() ? scan_labels_one_hw : scan_labels_one_sw;
  // contiguous rank chunks handed out to the threads; a thread keeps its best
  // per (labelling, fold), and (BA bits, rank) is a total order, so neither
  // the hand-out nor the merge order shows in the result
  const int64_t chunks = std::min<int64_t>(count, (int64_t)nt * 8);
  std::atomic<int64_t> next{0};
  std::atomic<int> oom{0};
  auto work = [&](int me) {
    LabelScratch s;
    try {
      s.mask.resize(3 * (size_t)W);
      s.cell.resize(3 * (size_t)F);
      s.own.resize((size_t)F);
      s.tp.resize((size_t)B * F);
      s.tn.resize((size_t)B * F);
    } catch (const std::bad_alloc&) {
      oom.store(1);
      return;
    }
    int32_t f[kMdrMaxK];
    Best* mine = best[me].data();
    for (int64_t c = next++; c < chunks; c = next++) {
      const int64_t r0 = (int64_t)((__int128)count * c / chunks);
      const int64_t r1 = (int64_t)((__int128)count * (c + 1) / chunks);
      if (r0 >= r1) continue;
      mdr_unrank(p, k, r0, f);
      for (int64_t r = r0; r < r1; r++) {
        if (r > r0) mdr_next(p, k, f);
        scan(planes.data(), W, L, k, f, Y.data(), B, tc.data(), tn.data(), s);
        for (int b = 0; b < B; b++)
          for (int i = 0; i < F; i++) {
            const size_t o = (size_t)b * F + i, t = (size_t)i * B + b;
            const float ba = mdr_ba(s.tp[o], s.tn[o], tc[t], tn[t]);
            if (ba_out) ba_out[o * count + r] = ba;
            uint32_t bits;
            std::memcpy(&bits, &ba, 4);
            if (mdr_better(bits, r, mine[o].bits, mine[o].rank)) mine[o].bits = bits, mine[o].rank = r;
          }
      }
    }
  };
  std::vector<std::thread> th;
  for (int w = 1; w < nt; w++) th.emplace_back(work, w);
  work(0);
  for (auto& t : th) t.join();
  if (oom.load()) {
    set_error("fs_mdr_scan_labels: out of host memory for a thread's scratch");
    return FS_EOOM;
  }
  for (size_t o = 0; o < (size_t)B * F; o++) {
    Best m;
    for (int w = 0; w < nt; w++)
      if (mdr_better(best[w][o].bits, best[w][o].rank, m.bits, m.rank)) m = best[w][o];
    std::memcpy(&best_ba[o], &m.bits, 4);
    best_rank[o] = m.rank;
  }
  return FS_OK;
}

namespace {

// The scan both fs_mdr_scan and fs_mdr_scan_top run: contiguous rank chunks,
// several per thread, handed out to nt threads; visit(thread, chunk, rank,
// fold, ba, bits) sees every balanced accuracy, a chunk's in rank order.
template <class Visit>
void scan_chunks(const std::vector<uint64_t>& planes, const MdrLayout& L, int64_t p, int k,
                 int64_t count, int nt, int64_t chunks, Visit visit) {
  const int F = L.F;
  const int64_t W = L.words;
  const ScanFn scan = have_popcnt() ? scan_one_hw : scan_one_sw;
  std::atomic<int64_t> next{0};
  auto work = [&](int me) {
    std::vector<uint32_t> cnt(6 * (size_t)F);
    std::vector<uint64_t> tp(F), tn(F);
    int32_t f[kMdrMaxK];
    for (int64_t c = next++; c < chunks; c = next++) {
      const int64_t r0 = (int64_t)((__int128)count * c / chunks);
      const int64_t r1 = (int64_t)((__int128)count * (c + 1) / chunks);
      if (r0 >= r1) continue;
      mdr_unrank(p, k, r0, f);
      for (int64_t r = r0; r < r1; r++) {
        if (r > r0) mdr_next(p, k, f);
        scan(planes.data(), W, L, k, f, cnt.data(), tp.data(), tn.data());
        for (int i = 0; i < F; i++) {
          const float ba = mdr_ba(tp[i], tn[i], (uint64_t)L.tc[i], (uint64_t)L.tn[i]);
          uint32_t bits;
          std::memcpy(&bits, &ba, 4);
          visit(me, c, r, i, ba, bits);
        }
      }
    }
  };
  std::vector<std::thread> th;
  for (int w = 1; w < nt; w++) th.emplace_back(work, w);
  work(0);
  for (auto& t : th) t.join();
}

}  // namespace

int mdr_scan(const uint8_t* x, int64_t n, int64_t p, const uint8_t* is_case, int k,
             const int32_t* fold, int n_folds, int n_jobs, int64_t count, float* best_ba,
             int64_t* best_rank, float* ba_out) {
  MdrLayout L;
  if (int rc = mdr_layout(n, is_case, fold, n_folds, 64, L)) return rc;
  std::vector<uint64_t> planes;
  try {
    if (int rc = pack_planes(x, p, L, n_jobs, planes)) return rc;
  } catch (const std::bad_alloc&) {
    set_error("fs_mdr_scan: out of host memory for the genotype planes");
    return FS_EOOM;
  }
  const int F = L.F;
  // each chunk keeps its own best, and the chunks merge in rank order (the
  // result does not depend on threads)
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(hardware_threads(n_jobs), count));
  const int64_t chunks = std::min<int64_t>(count, (int64_t)nt * 8);
  std::vector<Best> best((size_t)chunks * F);
  scan_chunks(planes, L, p, k, count, nt, chunks,
              [&](int, int64_t c, int64_t r, int i, float ba, uint32_t bits) {
                if (ba_out) ba_out[(size_t)i * count + r] = ba;
                Best& b = best[(size_t)c * F + i];
                if (mdr_better(bits, r, b.bits, b.rank)) b.bits = bits, b.rank = r;
              });
  for (int i = 0; i < F; i++) {
    Best m;
    for (int64_t c = 0; c < chunks; c++) {
      const Best& b = best[(size_t)c * F + i];
      if (mdr_better(b.bits, b.rank, m.bits, m.rank)) m = b;
    }
    std::memcpy(&best_ba[i], &m.bits, 4);
    best_rank[i] = m.rank;
  }
  return FS_OK;
}

int mdr_scan_top(const uint8_t* x, int64_t n, int64_t p, const uint8_t* is_case, int k,
                 const int32_t* fold, int n_folds, int n_jobs, int64_t count, int n_top,
                 float* top_ba, int64_t* top_rank) {
  MdrLayout L;
  if (int rc = mdr_layout(n, is_case, fold, n_folds, 64, L)) return rc;
  std::vector<uint64_t> planes;
  const int F = L.F;
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(hardware_threads(n_jobs), count));
  const size_t keep = (size_t)std::min<int64_t>(n_top, count);
  // a bounded heap per (thread, fold); merged at the end
  std::vector<MdrTopN> heap;
  try {
    if (int rc = pack_planes(x, p, L, n_jobs, planes)) return rc;
    for (size_t i = 0; i < (size_t)nt * F; i++) heap.emplace_back(keep);
  } catch (const std::bad_alloc&) {
    set_error("fs_mdr_scan_top: out of host memory for the genotype planes");
    return FS_EOOM;
  }
  scan_chunks(planes, L, p, k, count, nt, std::min<int64_t>(count, (int64_t)nt * 8),
              [&](int me, int64_t, int64_t r, int i, float, uint32_t bits) {
                heap[(size_t)me * F + i].push({bits, r});
              });
  for (int i = 0; i < F; i++) {
    MdrTopN& m = heap[i];
    for (int w = 1; w < nt; w++)
      for (const MdrCand& c : heap[(size_t)w * F + i].h) m.push(c);
    m.sorted_into(top_ba + (size_t)i * n_top, top_rank + (size_t)i * n_top, n_top);
  }
  return FS_OK;
}

}  // namespace cpu
}  // namespace fs
