// fs_pairscan.hip -- the GPU backend of fs_pair_screen: the n_top best of all
// C(p,2) pairs by joint relevance J(i, j) = I(X_i, X_j; y) or by the
// interaction gain (fs_pairscan.h), in one tiled scan, with no p x p matrix.
//
//   k_mi_pack      (fs_mi.hip, through MiPlanes) unchanged; y is column p.
//   k_pair_rel     the relevance I(X_f; y): pt_row<MiTerms, true> with y as the
//                  anchor and k_mi_scan's finish, the instantiation k_jmi_rel
//                  makes, so the bits of fs_mi_matrices / fs_jmi_select.  The
//                  columns are padded to a common multiple of this kernel's
//                  columns per workgroup and the scan's tile side.
//   k_pair_scan<C> k_mi_scan's geometry with k_jmi_row's class dimension,
//                  C = kcol[y] in 2..4.  One workgroup per tile (column block
//                  I) x (column block J), I <= J, of the upper triangle over the
//                  blocks that hold a feature; T = 16 / NB columns a side,
//                  NB = SP / 4; a pair takes NB^2 lanes and a lane holds one
//                  4 x 4 block per class, cnt[C][16].  Per chunk of kPtWC words
//                  the workgroup stages both blocks' planes, [side][word][T * SP]
//                  (32 KB), and beside them the C class words of y per word (at
//                  most 1 KB): the column planes of a tile are read from HBM
//                  once, not once per class and not once per partner.
//                  The class mask is applied in registers: per word a lane reads
//                  its I-side and J-side vectors once (two 16-byte LDS reads,
//                  the widest and cheapest per byte: MI355X_MICROARCH.md §LDS,
//                  cdna_hip_programming.md §2 "Read wide") and per class one
//                  word of y, the same address in every lane (a broadcast), ANDs
//                  it into the four I-side words and runs pt_count: 4 ANDs on
//                  top of 32 AND / popcount-accumulate instructions per class.
//                  C masked copies of one side in LDS, k_jmi_row's choice for
//                  its single anchor, would here take (C + 1) x 16 KB of staging
//                  (80 KB at four classes against 33 KB) and C + 1 16-byte reads
//                  per word where this takes two and C 4-byte broadcasts, for
//                  saving those 4 ANDs.  The kernel holds 39 / 42 / 44 KB of
//                  LDS and 116 / 162 / 214 VGPRs at C = 2 / 3 / 4 (cnt[C][16] and
//                  p1[16]), no spills: the registers allow 4 / 3 / 2 waves per
//                  SIMD (MI355X_MICROARCH.md §Register files), LDS as many
//                  workgroups or more (cdna_hip_programming.md Guideline 1).
//                  The epilogue is k_jmi_row's without the transposition
//                  (i < j always), in mi_from_table's order: p1 per joint state
//                  over the classes in index order on the lane that counted it,
//                  p2 and then the terms added row-major by the pair's first
//                  lane, one table row of every pair of the tile at a time
//                  through LDS over the dead staging area (T^2 * SP * C doubles,
//                  at most 32 KB).  So J has the bits fs_jmi_rows gives for
//                  (c = j, anchor = i) and for (c = i, anchor = j).
//                  After the value the pair's first lane forms the score and its
//                  ordered key (pair_key).  The per-feature maxima are a
//                  per-tile reduction through LDS and one integer atomicMax on
//                  the key per row and per column of the tile (2T atomics a
//                  tile; cdna_hip_programming.md Guideline 12).  A pair that
//                  beats the launch's threshold (pair_beats) appends
//                  (key, rank) through an integer cursor.  No float atomics.
//   Selection      one scan.  Launches take ascending runs of tiles on one
//                  stream; after each the host merges the launch's candidates
//                  into the running list of n_top (PairTopN) and, once the list
//                  is full, hands the next launch the list's worst entry as its
//                  threshold: what does not beat it cannot enter the list.
//                  Until then a launch admits every pair and is sized so that
//                  they fit the candidate buffer; afterwards a launch grows to
//                  the tiles expected to yield a quarter of the buffer (among
//                  N pairs seen, about n_top * M / N of the next M beat the
//                  n_top-th best so far).  A launch whose cursor passes the
//                  capacity is run again in halves; a tile alone always fits
//                  (the buffer holds at least kPtThreads candidates), so no
//                  candidate is ever dropped.  The list under a strict total
//                  order is independent of the split.
#include <algorithm>

#include "fs_gpu_internal.h"
#include "fs_pairscan.h"
#include "fs_pairtab.h"

namespace fs {
namespace gpu {

namespace {

constexpr int kPairRow = 64;  // most words of one staged word row: T * SP
// one table row of every pair of a tile, [pair][SP][C] doubles, lies over the
// staging area: T^2 * SP <= 1024 for every NB
static_assert(2 * kPtWC * kPairRow * 4 >= 1024 * kJmiMaxClassesGpu * 8, "a table row must fit");
constexpr int64_t kPairMaxTiles = (int64_t)1 << 22;  // tiles a launch: its pairs fit the cursor

thread_local double g_pair_ms[5] = {-1.0, -1.0, -1.0, -1.0, -1.0};

struct PairRelArgs {
  PtRowArgs row;
  int unit;
  double* out;
};

__global__ __launch_bounds__(kPtThreads) void k_pair_rel(const PairRelArgs a) {
  int64_t c;
  PtPair r;
  if (!pt_row<MiTerms, true>(a.row, c, r)) return;
  a.out[c] = (r.lo == r.hi || mi_constant(r.used1, r.used2)) ? 0.0 : mi_finish(r.sum, a.unit);
}

struct PairScanArgs {
  const uint32_t* planes;
  const int32_t* kcol;  // P1 state counts
  int64_t n, p, P1p, W;
  int SP, NB, T;
  int64_t nbf;          // column blocks that hold a feature: ceil(p / T)
  int64_t t0;           // first tile of this launch
  int unit, score_kind;
  const double* rel;    // p
  unsigned long long* fbest;  // NULL, or p keys (kPairNoKey: none yet)
  uint64_t thr_key;     // a pair is a candidate when it beats (thr_key, thr_rank)
  int64_t thr_rank;
  PairCand* cand;
  unsigned int* cursor;
  unsigned int cap;
};

// tile t of the upper triangle (row-major, diagonal included) -> (bi, bj)
__device__ __forceinline__ void pair_tile(int64_t nb, int64_t t, int64_t& bi, int64_t& bj) {
  const double m = 2.0 * (double)nb + 1.0;
  int64_t r = (int64_t)((m - sqrt(m * m - 8.0 * (double)t)) * 0.5);
  r = r < 0 ? 0 : (r > nb - 1 ? nb - 1 : r);
  while (r > 0 && tile_linear(nb, r, r) > t) r--;
  while (r + 1 < nb && tile_linear(nb, r + 1, r + 1) <= t) r++;
  bi = r;
  bj = r + (t - tile_linear(nb, r, r));
}

template <int C>
__global__ __launch_bounds__(kPtThreads) void k_pair_scan(const PairScanArgs a) {
  // staging: [side][word][T * SP]; after the scan: one table row, [pair][SP][C]
  __shared__ __align__(16) uint32_t s_raw[2 * kPtWC * kPairRow];
  __shared__ uint32_t s_y[kPtWC * C];              // [word][class]
  __shared__ double s_p2[kPtThreads * C];          // [pair][C]
  __shared__ unsigned long long s_key[kPtThreads]; // [pair]: the tile's keys
  const int tid = threadIdx.x;
  const int SP = a.SP, NB = a.NB, T = a.T;
  const int NP = T * SP;  // words of one staged word row
  const int nv = NP / 4;  // ... in 16-byte vectors
  const int L = NB * NB;  // lanes per pair
  int64_t bi, bj;
  pair_tile(a.nbf, a.t0 + blockIdx.x, bi, bj);
  const int q = tid / L;
  const int blk = tid - q * L;
  const int ab = blk / NB, bb = blk - ab * NB;  // column i's / column j's block of 4 states
  const int ii = q / T, jj = q - ii * T;
  const bool lane_on = q < T * T;
  const int64_t i = bi * T + ii, j = bj * T + jj;
  const bool pair_on = lane_on && i < j && j < a.p;

  uint32_t cnt[C][16];
#pragma unroll
  for (int cls = 0; cls < C; cls++)
#pragma unroll
    for (int k = 0; k < 16; k++) cnt[cls][k] = 0;

  const size_t row = (size_t)a.P1p * SP;  // words of one word row in HBM
  const uint32_t* gi = a.planes + (size_t)bi * NP;
  const uint32_t* gj = a.planes + (size_t)bj * NP;
  const uint32_t* gy = a.planes + (size_t)a.p * SP;  // y is column p: its class planes
  uint4* si = reinterpret_cast<uint4*>(s_raw);
  uint4* sj = reinterpret_cast<uint4*>(s_raw + kPtWC * kPairRow);
  const int oi = (ii * SP + 4 * ab) / 4, oj = (jj * SP + 4 * bb) / 4;
  for (int64_t w0 = 0; w0 < a.W; w0 += kPtWC) {
    const int wn = a.W - w0 < kPtWC ? (int)(a.W - w0) : kPtWC;
    for (int v = tid; v < wn * nv; v += kPtThreads) {
      const int w = v / nv, xq = v - w * nv;
      const size_t gw = (size_t)(w0 + w) * row + 4 * (size_t)xq;
      si[v] = *reinterpret_cast<const uint4*>(gi + gw);
      sj[v] = *reinterpret_cast<const uint4*>(gj + gw);
    }
    for (int v = tid; v < wn * C; v += kPtThreads) {
      const int w = v / C, cls = v - w * C;  // C <= SP
      s_y[v] = gy[(size_t)(w0 + w) * row + cls];
    }
    __syncthreads();
    if (pair_on)
      for (int w = 0; w < wn; w++) {
        const uint4 A = si[w * nv + oi], B = sj[w * nv + oj];
#pragma unroll
        for (int cls = 0; cls < C; cls++) {
          const uint32_t m = s_y[w * C + cls];
          uint4 Am;
          Am.x = A.x & m, Am.y = A.y & m, Am.z = A.z & m, Am.w = A.w & m;
          pt_count(Am, B, cnt[cls]);
        }
      }
    __syncthreads();
  }

  // The epilogue: k_jmi_row's steps (fs_jmi.hip) without the transposition.
  // cnt[cls][r * 4 + k] counts (state 4 ab + r of column i, state 4 bb + k of
  // column j, class cls); column i supplies the high digit of the joint state.
  const double dn = (double)a.n;
  double* s_row = reinterpret_cast<double*>(s_raw);
  const int sq = q * SP + 4 * bb;  // the lane's first cell of a table row
  const bool first = pair_on && blk == 0;
  // a state count never exceeds SP on packed data (the codes were checked
  // before this launch); the bound keeps the loops inside the row regardless
  int k_lo = 0, k_hi = 0;
  if (first) {
    k_lo = a.kcol[i] < SP ? a.kcol[i] : SP;
    k_hi = a.kcol[j] < SP ? a.kcol[j] : SP;
  }

  // p1 of the lane's 16 joint states: the sum over the classes in index order
  double p1[16];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    double s = 0.0;
#pragma unroll
    for (int cls = 0; cls < C; cls++) s += mi_pxy((int32_t)cnt[cls][k], dn);
    p1[k] = s;
  }

  // p2[c]: pxy row-major over (a, b), one table row a per round
  double p2a[C];
#pragma unroll
  for (int cls = 0; cls < C; cls++) p2a[cls] = 0.0;
  int used1 = 0;
  for (int rb = 0; rb < NB; rb++) {
    // the counts as new values in every round: the compiler would otherwise
    // hoist every cell's pxy (and term) out of this loop into registers
#pragma unroll
    for (int cls = 0; cls < C; cls++)
#pragma unroll
      for (int k = 0; k < 16; k++) asm volatile("" : "+v"(cnt[cls][k]));
#pragma unroll
    for (int r = 0; r < 4; r++) {
      if (lane_on && ab == rb) {
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
          for (int cls = 0; cls < C; cls++)
            s_row[(sq + k) * C + cls] = mi_pxy((int32_t)cnt[cls][r * 4 + k], dn);
      }
      __syncthreads();
      if (first && 4 * rb + r < k_lo) {
        const double* t = s_row + q * SP * C;
        for (int b = 0; b < k_hi; b++) {
          bool any = false;  // p1 of (a, b) is a sum of these: > 0 with any of them
#pragma unroll
          for (int cls = 0; cls < C; cls++) {
            const double v = t[b * C + cls];
            p2a[cls] += v;
            any = any || v > 0.0;
          }
          used1 += any;
        }
      }
      __syncthreads();
    }
  }
  int used2 = 0;
  if (first) {
#pragma unroll
    for (int cls = 0; cls < C; cls++) {
      s_p2[q * C + cls] = p2a[cls];
      used2 += p2a[cls] > 0.0;
    }
  }
  __syncthreads();

  // the terms, row-major over ((a, b), c), one table row a per round
  double sum = 0.0;
  for (int rb = 0; rb < NB; rb++) {
#pragma unroll
    for (int cls = 0; cls < C; cls++)
#pragma unroll
      for (int k = 0; k < 16; k++) asm volatile("" : "+v"(cnt[cls][k]));
#pragma unroll
    for (int r = 0; r < 4; r++) {
      if (pair_on && ab == rb) {
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
          for (int cls = 0; cls < C; cls++)
            s_row[(sq + k) * C + cls] = mi_term(mi_pxy((int32_t)cnt[cls][r * 4 + k], dn),
                                                p1[r * 4 + k], s_p2[q * C + cls]);
      }
      __syncthreads();
      if (first && 4 * rb + r < k_lo) {
        const double* t = s_row + q * SP * C;
        for (int b = 0; b < k_hi; b++)
#pragma unroll
          for (int cls = 0; cls < C; cls++) sum += t[b * C + cls];
      }
      __syncthreads();
    }
  }

  // the score, its key, and the tile's keys for the per-feature maxima
  uint64_t key = kPairNoKey;
  if (first) {
    const double jv = mi_constant(used1, used2) ? 0.0 : mi_finish(sum, a.unit);
    key = pair_key(pair_score_of(a.score_kind, jv, a.rel[i], a.rel[j]));
    const int64_t rank = pair_rank(a.p, i, j);
    if (pair_beats(key, rank, a.thr_key, a.thr_rank)) {
      const unsigned int pos = atomicAdd(a.cursor, 1u);
      if (pos < a.cap) {
        PairCand c;
        c.key = key, c.rank = rank;
        a.cand[pos] = c;
      }
    }
  }
  if (!a.fbest) return;  // the same for the whole grid
  if (lane_on && blk == 0) s_key[q] = key;
  __syncthreads();
  if (tid < 2 * T) {
    // lanes 0..T-1: the rows of the tile (column i); T..2T-1: its columns (j)
    const bool is_row = tid < T;
    const int x = is_row ? tid : tid - T;
    unsigned long long m = kPairNoKey;
    for (int o = 0; o < T; o++) {
      const unsigned long long v = is_row ? s_key[x * T + o] : s_key[o * T + x];
      m = v > m ? v : m;
    }
    // a key other than "none" comes from a pair i < j < p
    if (m != kPairNoKey) atomicMax(&a.fbest[(is_row ? bi : bj) * T + x], m);
  }
}

// The classes of y (max code + 1) from the host's copy: k_pair_scan's template
// parameter.  FS_EINVAL for a code >= n_states (what the pack would report)
// and beyond kJmiMaxClassesGpu.
int pair_y_classes(const uint8_t* ycodes, int64_t n, int n_states, int& C) {
  int mx = 0;
  for (int64_t i = 0; i < n; i++) mx = ycodes[i] > mx ? ycodes[i] : mx;
  if (mx >= n_states) {
    set_error("fs_pair_screen: a code is >= n_states");
    return FS_EINVAL;
  }
  if (mx + 1 > kJmiMaxClassesGpu) {
    set_error("fs_pair_screen: the GPU backend supports at most 4 classes of y");
    return FS_EINVAL;
  }
  C = mx + 1;
  return FS_OK;
}

int64_t gcd64(int64_t x, int64_t y) { return y == 0 ? x : gcd64(y, x % y); }

}  // namespace

void pair_last_timing(double* ms5) {
  for (int k = 0; k < 5; k++) ms5[k] = g_pair_ms[k];
}

// The geometry of a call: FS_EOOM on the sizes alone, before any array is read.
int pair_scan_geometry(MiPlanes& pl, const char* who, int64_t n, int64_t p, int n_states, int& T,
                       int& CPW) {
  const int NB = (n_states + 3) / 4;
  T = 16 / NB;                   // columns of a tile's side
  CPW = kPtThreads / (NB * NB);  // columns per workgroup of k_pair_rel
  return pl.shape(who, n, p, n_states, (int)((int64_t)T * CPW / gcd64(T, CPW)));
}

// ... and y's classes: FS_EINVAL.  Needs no device.
static int pair_plan(MiPlanes& pl, const uint8_t* ycodes, int64_t n, int64_t p, int n_states,
                     int& T, int& CPW, int& C) {
  FS_TRY(pair_scan_geometry(pl, "fs_pair_screen", n, p, n_states, T, CPW));
  return pair_y_classes(ycodes, n, n_states, C);
}

int pair_limits(const uint8_t* ycodes, int64_t n, int64_t p, int n_states) {
  MiPlanes pl;
  int T, CPW, C;
  return pair_plan(pl, ycodes, n, p, n_states, T, CPW, C);
}

// The relevance, the candidate buffer and its cursor.  The buffer: a test's
// value, else room for a launch that expects a quarter of it to grow by a
// factor of two at least; one tile always fits.
int pair_scan_bufs(DevArena& mem, int64_t p, int n_top, PairScanBufs& b) {
  int64_t cap = test_hooks().pair_cap > 0 ? test_hooks().pair_cap
                                          : std::max<int64_t>(16384, 8 * (int64_t)n_top);
  b.cap = std::min<int64_t>(std::max<int64_t>(cap, kPtThreads), (int64_t)1 << 30);
  try {
    b.host.resize((size_t)b.cap);
  } catch (const std::bad_alloc&) {
    set_error("fs_pair_screen: out of host memory");
    return FS_EOOM;
  }
  FS_TRY(mem.alloc(&b.rel, (size_t)p));
  FS_TRY(mem.alloc(&b.cand, (size_t)b.cap));
  return mem.alloc(&b.cursor, 1);
}

int pair_rel_launch(const MiPlanes& pl, int CPW, int unit, double* drel, hipStream_t s) {
  PairRelArgs r;
  r.row.planes = pl.planes, r.row.kcol = pl.kcol, r.row.n = pl.n, r.row.p = pl.p;
  r.row.P1p = pl.P1p, r.row.W = pl.W, r.row.SP = pl.SP, r.row.NB = pl.NB, r.row.CPW = CPW;
  r.row.anchor = pl.p, r.row.anchor_dev = nullptr;  // the target is column p
  r.unit = unit, r.out = drel;
  k_pair_rel<<<(unsigned)(pl.P1p / CPW), kPtThreads, 0, s>>>(r);
  return launch_check("k_pair_rel");
}

// One thread per word: y (n codes on the device) into column p of packed
// planes, and its state count into kcol[p] (zeroed by the caller, as
// MiPlanes::upload does for a whole pack).  The labels were checked on the
// host.
__global__ __launch_bounds__(256) void k_pair_repack_y(const uint8_t* __restrict__ y, int64_t n,
                                                       int64_t p, int64_t P1p, int SP, int64_t W,
                                                       uint32_t* __restrict__ planes,
                                                       int32_t* __restrict__ kcol) {
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= W) return;
  uint32_t code[32];
  uint32_t mx = 0;
#pragma unroll
  for (int b = 0; b < 32; b++) {
    const int64_t i = w * 32 + b;
    uint32_t g = 0xffffffffu;  // padding: matches no state
    if (i < n) {
      g = y[i];
      mx = g > mx ? g : mx;
    }
    code[b] = g;
  }
  uint32_t* out = planes + ((size_t)w * P1p + p) * SP;
  for (int s = 0; s < SP; s++) {
    uint32_t word = 0;
#pragma unroll
    for (int b = 0; b < 32; b++) word |= (uint32_t)(code[b] == (uint32_t)s) << b;
    out[s] = word;
  }
  atomicMax(&kcol[p], (int32_t)mx + 1);
}

int pair_repack_y(const MiPlanes& pl, const uint8_t* y, hipStream_t s) {
  FS_HIP(hipMemsetAsync(pl.kcol + pl.p, 0, 4, s));
  k_pair_repack_y<<<(unsigned)((pl.W + 255) / 256), 256, 0, s>>>(y, pl.n, pl.p, pl.P1p, pl.SP,
                                                                 pl.W, pl.planes, pl.kcol);
  return launch_check("k_pair_repack_y");
}

// The scan of packed planes with the selection (the head of this file): the
// n_top best pairs into `top`.  C: the classes of column p, 2..4.
int pair_scan_planes(const MiPlanes& pl, int C, int T, int unit, int score_kind, int n_top,
                     unsigned long long* dfb, PairScanBufs& b, PairTopN& top, hipStream_t s) {
  const int64_t cap = b.cap;
  std::vector<PairCand>& hc = b.host;
  PairCand* dcand = b.cand;
  unsigned int* dcur = b.cursor;
  PairScanArgs a;
  a.planes = pl.planes, a.kcol = pl.kcol, a.n = pl.n, a.p = pl.p, a.P1p = pl.P1p, a.W = pl.W;
  a.SP = pl.SP, a.NB = pl.NB, a.T = T, a.nbf = (pl.p + T - 1) / T;
  a.unit = unit, a.score_kind = score_kind, a.rel = b.rel, a.fbest = dfb;
  a.cand = dcand, a.cursor = dcur, a.cap = (unsigned int)cap;
  const int64_t tiles = a.nbf * (a.nbf + 1) / 2;
  // a launch of about 2e11 lane operations at most (k_mi_scan's bound, times
  // the classes), so that no launch holds the device for long
  const double ops = 256.0 * 32.0 * C * (double)pl.W;
  const int64_t per_max =
      std::min<int64_t>(kPairMaxTiles, (int64_t)std::max(1024.0, std::min(2e11 / ops, 1e9)));
  const int64_t hook_tiles = test_hooks().pair_tiles;
  std::vector<std::pair<int64_t, int64_t>> todo;  // (first tile, tiles) still to run
  for (int64_t t0 = 0; t0 < tiles;) {
    int64_t per;
    if (hook_tiles > 0)
      per = std::min(hook_tiles, kPairMaxTiles);
    else if (!top.full)
      per = std::min(per_max, cap / (T * T));  // every pair is a candidate: T^2 a tile
    else
      per = (int64_t)std::min((double)per_max, (double)t0 * (double)cap / (4.0 * n_top));
    per = std::min(std::max<int64_t>(per, 1), tiles - t0);
    todo.assign(1, {t0, per});
    while (!todo.empty()) {
      const int64_t b0 = todo.back().first, cnt = todo.back().second;
      todo.pop_back();
      a.t0 = b0, a.thr_key = top.thr.key, a.thr_rank = top.thr.rank;
      FS_HIP(hipMemsetAsync(dcur, 0, 4, s));
      switch (C) {
        case 2: k_pair_scan<2><<<(unsigned)cnt, kPtThreads, 0, s>>>(a); break;
        case 3: k_pair_scan<3><<<(unsigned)cnt, kPtThreads, 0, s>>>(a); break;
        default: k_pair_scan<4><<<(unsigned)cnt, kPtThreads, 0, s>>>(a); break;
      }
      FS_TRY(launch_check("k_pair_scan"));
      unsigned int got = 0;
      FS_HIP(hipMemcpyAsync(&got, dcur, 4, hipMemcpyDeviceToHost, s));
      FS_HIP(hipStreamSynchronize(s));
      if ((int64_t)got > cap) {
        // cnt >= 2: one tile yields at most kPtThreads <= cap candidates.
        // The halves run in ascending order; what this launch did to the
        // per-feature maxima is a maximum and stands.
        todo.push_back({b0 + cnt / 2, cnt - cnt / 2});
        todo.push_back({b0, cnt / 2});
        continue;
      }
      if (got) {
        FS_HIP(hipMemcpyAsync(hc.data(), dcand, (size_t)got * sizeof(PairCand),
                              hipMemcpyDeviceToHost, s));
        FS_HIP(hipStreamSynchronize(s));
        for (unsigned int t = 0; t < got; t++) top.push(hc[t].key, hc[t].rank);
        top.compact();
      }
    }
    t0 += per;
  }
  return FS_OK;
}

int pair_screen(int device, const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p,
                int n_states, int unit, int score_kind, int n_top, double* relevance,
                double* top_score, int64_t* top_i, int64_t* top_j, double* feature_best) {
  if (device_count() <= 0) return no_device();
  for (double& v : g_pair_ms) v = -1.0;
  MiPlanes pl;
  int T = 0, CPW = 0, C = 0;
  FS_TRY(pair_plan(pl, ycodes, n, p, n_states, T, CPW, C));
  const int64_t total = pair_count(p);

  PairTopN top((size_t)n_top);
  std::vector<unsigned long long> hfb;
  try {
    if (feature_best) hfb.resize((size_t)p);
  } catch (const std::bad_alloc&) {
    set_error("fs_pair_screen: out of host memory");
    return FS_EOOM;
  }

  FS_HIP(hipSetDevice(device));
  DevArena mem(device);
  StreamLease lease(device);  // destroyed (and the stream synchronised) before `mem`
  FS_TRY(lease.open(6));
  hipStream_t s = lease.s;
  std::vector<hipEvent_t>& ev = lease.ev;
  PairScanBufs bufs;
  unsigned long long* dfb = nullptr;
  // every block is allocated before any array is uploaded
  FS_TRY(pl.alloc(mem, mem));
  if (feature_best) FS_TRY(mem.alloc(&dfb, (size_t)p));
  FS_TRY(pair_scan_bufs(mem, p, n_top, bufs));
  double* drel = bufs.rel;

  FS_HIP(hipEventRecord(ev[0], s));
  FS_TRY(pl.upload(codes, ycodes, s));
  if (dfb) FS_HIP(hipMemsetAsync(dfb, 0, (size_t)p * 8, s));  // kPairNoKey
  FS_HIP(hipEventRecord(ev[1], s));
  FS_TRY(pl.pack(s));
  FS_HIP(hipEventRecord(ev[2], s));
  FS_TRY(pair_rel_launch(pl, CPW, unit, drel, s));
  FS_HIP(hipEventRecord(ev[3], s));
  // the codes are checked before the scan reads a state count
  FS_TRY(pl.fetch_bad(s));
  FS_HIP(hipStreamSynchronize(s));
  FS_TRY(pl.check());

  if (C >= 2) {
    FS_TRY(pair_scan_planes(pl, C, T, unit, score_kind, n_top, dfb, bufs, top, s));
  } else {
    // a one-class y: every J and every relevance is exactly 0.0, so is either
    // score; no scan.  The list is the first ranks.
    const uint64_t zero = pair_key(0.0);
    for (int64_t r = 0; r < std::min<int64_t>(n_top, total); r++) top.push(zero, r);
    if (dfb) FS_HIP(hipMemsetAsync(dfb, 0, (size_t)p * 8, s));
  }
  FS_HIP(hipEventRecord(ev[4], s));
  FS_HIP(hipMemcpyAsync(relevance, drel, (size_t)p * 8, hipMemcpyDeviceToHost, s));
  if (dfb) FS_HIP(hipMemcpyAsync(hfb.data(), dfb, (size_t)p * 8, hipMemcpyDeviceToHost, s));
  FS_HIP(hipEventRecord(ev[5], s));
  FS_HIP(hipStreamSynchronize(s));
  top.sorted_into(p, top_score, top_i, top_j);
  if (feature_best)
    for (int64_t f = 0; f < p; f++)
      feature_best[f] = (C >= 2) ? pair_score(hfb[(size_t)f]) : 0.0;
  for (int k = 0; k < 5; k++) {
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess) g_pair_ms[k] = ms;
  }
  (void)hipGetLastError();
  return FS_OK;
}

}  // namespace gpu
}  // namespace fs
