// fs_pairscan_labels.hip -- the GPU backend of fs_pair_screen_labels: the best
// pair of the pair screen (fs_pairscan.h) under each of B labellings of y, in
// one pass over the pairs.  A pair's joint cells A_a & B_b do not depend on y;
// the labelling enters at popcount(cell & class word) only.
//
// Fast route, up to 4 states (SP == 4):
//   k_mi_pack           (fs_mi.hip, through MiPlanes) unchanged: it checks the
//                       codes and gives kcol.
//   k_pair_cols         its planes -> cols[(c * 4 + s) * Q + q], quads of four
//                       words (128 samples) with the word index fastest, zero
//                       past the last word: a wave reads a column's words in a
//                       row through the scalar cache (k_mdr_pack_cols' layout).
//   k_pair_pack_labels  labels (bytes) -> y[((q * (C - 1) + c) * B + b) * 4 + i]:
//                       word i of quad q of class c under labelling b, for the
//                       classes 0..C-2.  Within a quad and class the labelling
//                       index is fastest: a lane's four words are one aligned
//                       16-byte load, consecutive across the wave
//                       (k_mdr_pack_labels' layout).  The planes are zero past
//                       n, so the labels' padding bits never count.
//   k_pair_lab<C, REL>  one lane per labelling, a wave takes one pair (REL: one
//                       feature) at a time; a block's waves take interleaved
//                       ranks of the block's contiguous run.  The wave index
//                       and the unranked (i, j) go through readfirstlane and
//                       the planes are read through the constant address space,
//                       so the two columns' plane quads, the cell masks
//                       A_a & B_b and each cell's total are scalar loads and
//                       scalar ALU, once for 64 labellings.  Per word and cell
//                       a lane issues one AND with its class word and one
//                       popcount-accumulate for the classes 0..C-2; the last
//                       class is the cell's total minus the others.  The loops
//                       over the cells are unrolled with wave-uniform guards
//                       a < kcol[i], b < kcol[j]: the 16 * (C - 1) counters
//                       stay in registers.
//                       The epilogue is mi_from_table's sequence on the lane's
//                       own table, in k_pair_scan's order: p2[c] row-major over
//                       (a, b); per joint state p1 over the classes in index
//                       order, then the state's terms, row-major over
//                       ((a, b), c); used1 / used2; mi_constant, mi_finish; then
//                       pair_score_of with the labelling's own relevance, and
//                       pair_key.  Its two passes over the cells stay rolled
//                       (wave-uniform trip counts): unrolled, the 16 * C float64
//                       logarithms of a pair are some 100 KB of code, more than
//                       the instruction cache.  A rolled loop cannot index
//                       registers, so a lane first puts its counters into its
//                       own column of LDS ([counter][thread]: bank-conflict
//                       free, read by no other lane, no barrier) and the cell
//                       totals into the wave's 16 words.  No lane waits for
//                       another and none runs serially for its wave.
//                       REL is the same code with the second column a single
//                       all-ones state: the table [a][c] of the relevance, the
//                       bits of k_pair_rel / fs_mi_matrices, written as
//                       rel[f][b].  It runs before the scan on the same stream.
//                       Per labelling the block merges (max key, min rank) over
//                       its waves through LDS into the block's slot; one block
//                       owns a slot in every launch, so there are no atomics.
//   k_pair_lab_reduce   the slots of all blocks -> [B] on the device; ties go
//                       to the smaller rank at every level.
//   Launches            about 2e11 lane operations of the word loop per launch
//                       (32 (C - 1) per word, pair and labelling).  Labellings
//                       go into one launch in multiples of 64 as far as that
//                       allows, then pair ranks.  The slot array is bounded by
//                       kPairLabMaxSlots.  One stream; every device block is
//                       allocated before the first upload.
//
// General route, 5..32 states: the columns are packed once; per labelling y
// alone is packed again (k_pair_repack_y) and fs_pair_screen's own k_pair_rel
// and k_pair_scan run with a list of one (pair_scan_planes, fs_pairscan.hip).
// Correct and slow: a launch sequence per labelling.
#include <algorithm>

#include "fs_gpu_internal.h"
#include "fs_pairscan.h"

namespace fs {
namespace gpu {

namespace {

constexpr int kPlThreads = 256;
constexpr int kPlWaves = kPlThreads / 64;
constexpr int kPairLabMaxBlocks = 1024;  // rank runs (grid.x) per launch
constexpr size_t kPairLabMaxSlots = (size_t)1 << 24;

thread_local double g_pl_ms[5] = {-1.0, -1.0, -1.0, -1.0, -1.0};

typedef uint32_t Quad __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) Quad PlaneQuad;
typedef const __attribute__((address_space(4))) int32_t ConstInt;

// One thread per (column, quad): four words of k_mi_pack's planes -> the
// column's four state quads.  Q quads in all; this launch starts at q0.
__global__ __launch_bounds__(256) void k_pair_cols(const uint32_t* __restrict__ planes, int64_t p,
                                                   int64_t P1p, int64_t W, int64_t Q, int64_t q0,
                                                   Quad* __restrict__ cols) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t q = q0 + blockIdx.y;
  if (c >= p || q >= Q) return;
  uint32_t w4[4][4];  // [word][state]
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int64_t w = q * 4 + i;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (w < W) v = *reinterpret_cast<const uint4*>(planes + ((size_t)w * P1p + c) * 4);
    w4[i][0] = v.x, w4[i][1] = v.y, w4[i][2] = v.z, w4[i][3] = v.w;
  }
#pragma unroll
  for (int s = 0; s < 4; s++) {
    Quad o;
    o.x = w4[0][s], o.y = w4[1][s], o.z = w4[2][s], o.w = w4[3][s];
    cols[((size_t)c * 4 + s) * Q + q] = o;
  }
}

// One thread per (word, labelling); the words 0..4Q-1, those past n as zeros.
__global__ __launch_bounds__(256) void k_pair_pack_labels(const uint8_t* __restrict__ labels,
                                                          int64_t n, int B, int C1, int64_t words,
                                                          int64_t w0, uint32_t* __restrict__ y) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t w = w0 + blockIdx.y;
  if (b >= B || w >= words) return;
  uint32_t bits[kJmiMaxClassesGpu - 1] = {0, 0, 0};
  for (int i = 0; i < 32; i++) {
    const int64_t s = w * 32 + i;
    if (s < n) {
      const uint32_t code = labels[(size_t)b * n + s];
#pragma unroll
      for (int c = 0; c < kJmiMaxClassesGpu - 1; c++) bits[c] |= (uint32_t)(code == (uint32_t)c) << i;
    }
  }
#pragma unroll
  for (int c = 0; c < kJmiMaxClassesGpu - 1; c++)
    if (c < C1) y[((((size_t)(w >> 2)) * C1 + c) * B + b) * 4 + (w & 3)] = bits[c];
}

__global__ __launch_bounds__(256) void k_pair_lab_fill(unsigned long long* __restrict__ key,
                                                       int64_t* __restrict__ rank, size_t slots) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < slots) key[i] = kPairNoKey, rank[i] = INT64_MAX;
}

struct PairLabArgs {
  const Quad* cols;      // [(column * 4 + state) * Q + q]
  const int32_t* kcol;
  int64_t n, p, Q;
  const Quad* y;         // [(q * (C - 1) + c) * B + b]
  int B, b0;             // grid.y * 64 + lane + b0 is the lane's labelling
  int unit, score_kind;
  int64_t r0, r1;        // this launch's ranks (REL: features)
  int64_t per_block;     // ranks per block, a multiple of the waves per block
  double* rel;           // [p][B]: written by REL, read by the scan
  unsigned long long* part_key;  // blocks x B
  int64_t* part_rank;
};

__device__ __forceinline__ uint32_t popc4(Quad v) {
  return __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
}
__device__ __forceinline__ int64_t uniform64(int64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// The joint relevance of the pair (i, j) -- REL: the relevance of the feature
// i -- under the lane's labelling b.  NJ: the second column's states, 4 or
// (REL) the one all-ones state.  s_cnt: the lane's column of LDS,
// [counter][kPlThreads] from the lane's own entry; s_tot: the wave's NJ * 4
// cell totals.
template <int C, bool REL>
__device__ __forceinline__ double pl_value(const PairLabArgs& a, int64_t i, int64_t j, uint32_t b,
                                           uint32_t* s_cnt, uint32_t* s_tot) {
  constexpr int NJ = REL ? 1 : 4, C1 = C - 1;
  ConstInt* const kcol = (ConstInt*)a.kcol;
  // a state count never exceeds 4 on packed data (the codes are checked
  // before this launch); the bound keeps the loops inside the table regardless
  const int ki = min(kcol[i], 4), kj = REL ? 1 : min(kcol[j], 4);
  const size_t Q = (size_t)a.Q, B = (size_t)a.B;
  PlaneQuad* const cols = (PlaneQuad*)a.cols;
  PlaneQuad* const A = cols + (size_t)i * 4 * Q;
  PlaneQuad* const Bc = cols + (size_t)(REL ? i : j) * 4 * Q;
  const Quad* y = a.y;

  uint32_t cnt[4 * NJ][C1], tot[4 * NJ];
#pragma unroll
  for (int k = 0; k < 4 * NJ; k++) {
    tot[k] = 0;
#pragma unroll
    for (int c = 0; c < C1; c++) cnt[k][c] = 0;
  }
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
  for (size_t q = 0; q < Q; q++) {
    Quad yw[C1];
#pragma unroll
    for (int c = 0; c < C1; c++) yw[c] = (y + (q * C1 + c) * B)[b];
    Quad Aq[4], Bq[4];
#pragma unroll
    for (int s = 0; s < 4; s++) Aq[s] = A[s * Q + q];
    if (!REL) {
#pragma unroll
      for (int s = 0; s < 4; s++) Bq[s] = Bc[s * Q + q];
    }
#pragma unroll
    for (int sa = 0; sa < 4; sa++) {
      if (sa < ki) {
#pragma unroll
        for (int sb = 0; sb < NJ; sb++) {
          if (sb < kj) {
            const Quad m = REL ? Aq[sa] : (Aq[sa] & Bq[sb]);
            tot[sa * NJ + sb] += popc4(m);
#pragma unroll
            for (int c = 0; c < C1; c++) cnt[sa * NJ + sb][c] += popc4(m & yw[c]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4 * NJ; k++) {
    s_tot[k] = tot[k];  // the same value from every lane of the wave
#pragma unroll
    for (int c = 0; c < C1; c++) s_cnt[(k * C1 + c) * kPlThreads] = cnt[k][c];
  }

  const double dn = (double)a.n;
  // p2[c]: pxy row-major over (a, b)
  double p2[C];
#pragma unroll
  for (int c = 0; c < C; c++) p2[c] = 0.0;
#pragma unroll 1
  for (int sa = 0; sa < ki; sa++) {
#pragma unroll 1
    for (int sb = 0; sb < kj; sb++) {
      const int k = sa * NJ + sb;
      uint32_t rest = s_tot[k];
#pragma unroll
      for (int c = 0; c < C1; c++) {
        const uint32_t u = s_cnt[(k * C1 + c) * kPlThreads];
        p2[c] += mi_pxy((int32_t)u, dn);
        rest -= u;
      }
      p2[C1] += mi_pxy((int32_t)rest, dn);
    }
  }
  // per joint state p1 over the classes in index order, then its terms
  double sum = 0.0;
  int used1 = 0;
#pragma unroll 1
  for (int sa = 0; sa < ki; sa++) {
#pragma unroll 1
    for (int sb = 0; sb < kj; sb++) {
      const int k = sa * NJ + sb;
      uint32_t rest = s_tot[k];
      double px[C];
#pragma unroll
      for (int c = 0; c < C1; c++) {
        const uint32_t u = s_cnt[(k * C1 + c) * kPlThreads];
        px[c] = mi_pxy((int32_t)u, dn);
        rest -= u;
      }
      px[C1] = mi_pxy((int32_t)rest, dn);
      double p1 = 0.0;
#pragma unroll
      for (int c = 0; c < C; c++) p1 += px[c];
      used1 += p1 > 0.0;
#pragma unroll
      for (int c = 0; c < C; c++) sum += mi_term(px[c], p1, p2[c]);
    }
  }
  int used2 = 0;
#pragma unroll
  for (int c = 0; c < C; c++) used2 += p2[c] > 0.0;
  return mi_constant(used1, used2) ? 0.0 : mi_finish(sum, a.unit);
}

template <int C, bool REL>
__global__ __launch_bounds__(kPlThreads) void k_pair_lab(const PairLabArgs a) {
  constexpr int NC = (REL ? 4 : 16) * (C - 1);  // counters of a lane
  __shared__ uint32_t s_cnt[NC * kPlThreads];
  __shared__ uint32_t s_tot[kPlWaves][16];
  __shared__ unsigned long long s_key[kPlWaves][64];
  __shared__ int64_t s_rank[kPlWaves][64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t bl = (int64_t)a.b0 + (int64_t)blockIdx.y * 64 + lane;
  const bool live = bl < a.B;
  // a lane past the last labelling computes the last one's and writes nothing
  const uint32_t b = (uint32_t)(live ? bl : a.B - 1);
  const int64_t first = a.r0 + (int64_t)blockIdx.x * a.per_block + wave;
  const int64_t end = min(a.r1, a.r0 + ((int64_t)blockIdx.x + 1) * a.per_block);

  unsigned long long best_key = kPairNoKey;
  int64_t best_rank = INT64_MAX;
  for (int64_t r = first; r < end; r += kPlWaves) {
    if (REL) {
      const double v = pl_value<C, true>(a, r, r, b, s_cnt + tid, s_tot[wave]);
      if (live) a.rel[(size_t)r * a.B + b] = v;
    } else {
      int64_t i, j;
      pair_unrank(a.p, r, i, j);
      i = uniform64(i), j = uniform64(j);
      const double jv = pl_value<C, false>(a, i, j, b, s_cnt + tid, s_tot[wave]);
      const double ri = a.rel[(size_t)i * a.B + b], rj = a.rel[(size_t)j * a.B + b];
      const unsigned long long key = pair_key(pair_score_of(a.score_kind, jv, ri, rj));
      // ranks ascend, so a strict improvement keeps the smallest
      if (key > best_key) best_key = key, best_rank = r;
    }
  }
  if (REL) return;

  // the block's waves hold the same labellings: merge them, then the block's
  // slot (one block owns it in every launch: no atomics)
  s_key[wave][lane] = best_key;
  s_rank[wave][lane] = best_rank;
  __syncthreads();
  if (tid < 64 && live) {
    unsigned long long key = s_key[0][lane];
    int64_t rank = s_rank[0][lane];
    for (int w = 1; w < kPlWaves; w++)
      if (pair_beats(s_key[w][lane], s_rank[w][lane], key, rank))
        key = s_key[w][lane], rank = s_rank[w][lane];
    const size_t slot = (size_t)blockIdx.x * a.B + b;
    if (pair_beats(key, rank, a.part_key[slot], a.part_rank[slot]))
      a.part_key[slot] = key, a.part_rank[slot] = rank;
  }
}

// One thread per labelling: the best over the blocks' slots.
__global__ __launch_bounds__(256) void k_pair_lab_reduce(
    const unsigned long long* __restrict__ part_key, const int64_t* __restrict__ part_rank,
    int blocks, int B, unsigned long long* __restrict__ out_key, int64_t* __restrict__ out_rank) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  unsigned long long key = kPairNoKey;
  int64_t rank = INT64_MAX;
  for (int x = 0; x < blocks; x++) {
    const size_t slot = (size_t)x * B + b;
    if (pair_beats(part_key[slot], part_rank[slot], key, rank))
      key = part_key[slot], rank = part_rank[slot];
  }
  out_key[b] = key, out_rank[b] = rank;
}

template <bool REL>
void launch_lab(int C, const PairLabArgs& a, dim3 grid, hipStream_t s) {
  switch (C) {
    case 2: k_pair_lab<2, REL><<<grid, kPlThreads, 0, s>>>(a); break;
    case 3: k_pair_lab<3, REL><<<grid, kPlThreads, 0, s>>>(a); break;
    default: k_pair_lab<4, REL><<<grid, kPlThreads, 0, s>>>(a); break;
  }
}

// The geometry of a call: FS_EOOM on the sizes alone.  Needs no device.
int labels_plan(MiPlanes& pl, int n_labelings, int64_t n, int64_t p, int n_states, int& T,
                int& CPW) {
  const char* who = "fs_pair_screen_labels";
  if (n_states <= 4) {
    T = CPW = 0;
    FS_TRY(pl.shape(who, n, p, n_states, 1));
    // the column quads, the label quads at four classes, the relevance
    const double Q = (double)((pl.W + 3) / 4), B = (double)n_labelings;
    if (Q * 64.0 * (double)p + Q * 48.0 * B + 8.0 * (double)p * B + (double)n * B > kMiMaxBytes) {
      set_error(std::string(who) + ": the bit-planes do not fit the device memory");
      return FS_EOOM;
    }
  } else {
    FS_TRY(pair_scan_geometry(pl, who, n, p, n_states, T, CPW));
    if ((double)n * (double)n_labelings > kMiMaxBytes) {
      set_error(std::string(who) + ": the labels do not fit the device memory");
      return FS_EOOM;
    }
  }
  return FS_OK;
}

void store_times(const std::vector<hipEvent_t>& ev) {
  for (int k = 0; k < 5; k++) {
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess) g_pl_ms[k] = ms;
  }
  (void)hipGetLastError();
}

// 5..32 states: fs_pair_screen's kernels, one labelling at a time.
int labels_general(int device, MiPlanes& pl, int T, int CPW, const uint8_t* codes,
                   const uint8_t* labels, int B, int unit, int score_kind, double* best_score,
                   int64_t* best_i, int64_t* best_j, double* relevance) {
  const int64_t n = pl.n, p = pl.p;
  FS_HIP(hipSetDevice(device));
  DevArena mem(device);
  StreamLease lease(device);  // destroyed (and the stream synchronised) before `mem`
  FS_TRY(lease.open(6));
  hipStream_t s = lease.s;
  std::vector<hipEvent_t>& ev = lease.ev;
  PairScanBufs bufs;
  uint8_t* dlab = nullptr;
  // every block is allocated before any array is uploaded
  FS_TRY(pl.alloc(mem, mem));
  FS_TRY(mem.alloc(&dlab, (size_t)B * n));
  FS_TRY(pair_scan_bufs(mem, p, 1, bufs));

  FS_HIP(hipEventRecord(ev[0], s));
  FS_TRY(pl.upload(codes, labels, s));
  FS_HIP(hipMemcpyAsync(dlab, labels, (size_t)B * n, hipMemcpyHostToDevice, s));
  FS_HIP(hipEventRecord(ev[1], s));
  FS_TRY(pl.pack(s));
  FS_HIP(hipEventRecord(ev[2], s));
  // the relevance launches are per labelling: timed with the scan
  FS_HIP(hipEventRecord(ev[3], s));
  FS_TRY(pl.fetch_bad(s));
  FS_HIP(hipStreamSynchronize(s));
  FS_TRY(pl.check());
  for (int b = 0; b < B; b++) {
    const uint8_t* yb = labels + (size_t)b * n;
    int Cb = 0;
    for (int64_t i = 0; i < n; i++) Cb = yb[i] > Cb ? yb[i] : Cb;
    Cb++;
    if (b > 0) FS_TRY(pair_repack_y(pl, dlab + (size_t)b * n, s));
    FS_TRY(pair_rel_launch(pl, CPW, unit, bufs.rel, s));
    if (relevance)
      FS_HIP(hipMemcpyAsync(relevance + (size_t)b * p, bufs.rel, (size_t)p * 8,
                            hipMemcpyDeviceToHost, s));
    PairTopN top(1);
    if (Cb >= 2)
      FS_TRY(pair_scan_planes(pl, Cb, T, unit, score_kind, 1, nullptr, bufs, top, s));
    else
      top.push(pair_key(0.0), 0);  // a one-class row: every score is exactly 0.0
    top.sorted_into(p, best_score + b, best_i + b, best_j + b);
  }
  FS_HIP(hipEventRecord(ev[4], s));
  FS_HIP(hipEventRecord(ev[5], s));
  FS_HIP(hipStreamSynchronize(s));
  store_times(ev);
  return FS_OK;
}

}  // namespace

void pair_labels_last_timing(double* ms5) {
  for (int k = 0; k < 5; k++) ms5[k] = g_pl_ms[k];
}

// FS_EOOM before any array is read, then FS_EINVAL for the labels.
int pair_labels_limits(const uint8_t* labels, int n_labelings, int64_t n, int64_t p, int n_states,
                       int* classes) {
  MiPlanes pl;
  int T, CPW;
  FS_TRY(labels_plan(pl, n_labelings, n, p, n_states, T, CPW));
  FS_TRY(pair_labels_classes(labels, n_labelings, n, n_states, *classes));
  if (*classes > kJmiMaxClassesGpu) {
    set_error(
        "fs_pair_screen_labels: the GPU backend supports at most 4 classes over all labellings");
    return FS_EINVAL;
  }
  return FS_OK;
}

int pair_screen_labels(int device, const uint8_t* codes, const uint8_t* labels, int n_labelings,
                       int classes, int64_t n, int64_t p, int n_states, int unit, int score_kind,
                       double* best_score, int64_t* best_i, int64_t* best_j, double* relevance) {
  if (device_count() <= 0) return no_device();
  for (double& v : g_pl_ms) v = -1.0;
  MiPlanes pl;
  int T = 0, CPW = 0;
  const int B = n_labelings, C = classes;  // 1..kJmiMaxClassesGpu: pair_labels_limits
  FS_TRY(labels_plan(pl, B, n, p, n_states, T, CPW));
  if (pl.SP > 4)
    return labels_general(device, pl, T, CPW, codes, labels, B, unit, score_kind, best_score,
                          best_i, best_j, relevance);

  const int64_t total = pair_count(p);
  const int64_t Q = (pl.W + 3) / 4, W4 = Q * 4;
  const int C1 = std::max(C - 1, 1);
  // launches of about 2e11 lane operations of the word loop: per pair and
  // labelling 16 cells x (C - 1) classes x 2 per word.  The labellings go into
  // one launch as far as that allows, then the ranks.
  const double ops = (double)W4 * 32.0 * C1;
  const double work = std::max(2e11 / ops, 64.0 * kPlWaves);  // (pair, labelling) per launch
  const int64_t lab_chunk =
      test_hooks().pair_labels > 0
          ? std::max<int64_t>(64, test_hooks().pair_labels / 64 * 64)
          : std::max<int64_t>(64, std::min<int64_t>(((int64_t)B + 63) / 64 * 64,
                                                    (int64_t)(work / 256.0) / 64 * 64));
  const int64_t chunk =
      test_hooks().pair_lab_ranks > 0
          ? test_hooks().pair_lab_ranks
          : std::max<int64_t>(kPlWaves, (int64_t)std::min(work / (double)lab_chunk, 4e18));
  // blocks (rank runs) of the largest launch; every launch uses the first ones
  const int64_t max_bx = std::max<int64_t>(
      1, std::min<int64_t>(kPairLabMaxBlocks, (int64_t)(kPairLabMaxSlots / (size_t)B)));
  const int nbx =
      (int)std::min<int64_t>(max_bx, (std::min(total, chunk) + kPlWaves - 1) / kPlWaves);
  const size_t nslots = (size_t)nbx * B;

  std::vector<unsigned long long> hkey;
  std::vector<int64_t> hrank;
  std::vector<double> hrel;
  try {
    hkey.resize((size_t)B);
    hrank.resize((size_t)B);
    if (relevance) hrel.resize((size_t)p * B);
  } catch (const std::bad_alloc&) {
    set_error("fs_pair_screen_labels: out of host memory");
    return FS_EOOM;
  }

  FS_HIP(hipSetDevice(device));
  DevArena mem(device);
  StreamLease lease(device);  // destroyed (and the stream synchronised) before `mem`
  FS_TRY(lease.open(6));
  hipStream_t s = lease.s;
  std::vector<hipEvent_t>& ev = lease.ev;
  uint8_t* dlab = nullptr;
  Quad *dcols = nullptr, *dy = nullptr;
  double* drel = nullptr;
  unsigned long long *dpkey = nullptr, *dokey = nullptr;
  int64_t *dprank = nullptr, *dorank = nullptr;
  // every block is allocated before any array is uploaded
  FS_TRY(pl.alloc(mem, mem));
  FS_TRY(mem.alloc(&dlab, (size_t)B * n));
  FS_TRY(mem.alloc(&dcols, (size_t)p * 4 * Q));
  FS_TRY(mem.alloc(&dy, (size_t)Q * C1 * B));
  FS_TRY(mem.alloc(&drel, (size_t)p * B));
  FS_TRY(mem.alloc(&dpkey, nslots));
  FS_TRY(mem.alloc(&dprank, nslots));
  FS_TRY(mem.alloc(&dokey, (size_t)B));
  FS_TRY(mem.alloc(&dorank, (size_t)B));

  FS_HIP(hipEventRecord(ev[0], s));
  FS_TRY(pl.upload(codes, labels, s));  // y of the pack: the first labelling
  FS_HIP(hipMemcpyAsync(dlab, labels, (size_t)B * n, hipMemcpyHostToDevice, s));
  FS_HIP(hipEventRecord(ev[1], s));
  FS_TRY(pl.pack(s));
  {
    // grid.y is limited to 65535: pack the quads and words in slabs
    const unsigned gx = (unsigned)((p + 255) / 256), gb = (unsigned)((B + 255) / 256);
    for (int64_t q0 = 0; q0 < Q; q0 += 65535) {
      const int64_t qn = std::min<int64_t>(65535, Q - q0);
      k_pair_cols<<<dim3(gx, (unsigned)qn), 256, 0, s>>>(pl.planes, p, pl.P1p, pl.W, Q, q0, dcols);
      FS_TRY(launch_check("k_pair_cols"));
    }
    for (int64_t w0 = 0; w0 < W4 && C >= 2; w0 += 65535) {
      const int64_t wn = std::min<int64_t>(65535, W4 - w0);
      k_pair_pack_labels<<<dim3(gb, (unsigned)wn), 256, 0, s>>>(dlab, n, B, C1, W4, w0,
                                                                (uint32_t*)dy);
      FS_TRY(launch_check("k_pair_pack_labels"));
    }
    k_pair_lab_fill<<<(unsigned)((nslots + 255) / 256), 256, 0, s>>>(dpkey, dprank, nslots);
    FS_TRY(launch_check("k_pair_lab_fill"));
  }
  FS_HIP(hipEventRecord(ev[2], s));
  // the codes are checked before a kernel reads a state count
  FS_TRY(pl.fetch_bad(s));
  FS_HIP(hipStreamSynchronize(s));
  FS_TRY(pl.check());

  if (C >= 2) {
    PairLabArgs a;
    a.cols = dcols, a.kcol = pl.kcol, a.n = n, a.p = p, a.Q = Q, a.y = dy, a.B = B;
    a.unit = unit, a.score_kind = score_kind, a.rel = drel;
    a.part_key = dpkey, a.part_rank = dprank;
    // the relevance: a wave per feature, every feature in one launch per
    // label chunk (4 cells a feature: a sixteenth of a pair's work)
    for (int64_t b0 = 0; b0 < B; b0 += lab_chunk) {
      a.b0 = (int)b0, a.r0 = 0, a.r1 = p;
      const unsigned gy = (unsigned)((std::min<int64_t>(lab_chunk, B - b0) + 63) / 64);
      const int64_t runs = (p + kPlWaves - 1) / kPlWaves;
      const int64_t blocks = std::min<int64_t>(runs, 65535);
      a.per_block = (runs + blocks - 1) / blocks * kPlWaves;
      launch_lab<true>(C, a, dim3((unsigned)blocks, gy), s);
      FS_TRY(launch_check("k_pair_lab (relevance)"));
    }
    FS_HIP(hipEventRecord(ev[3], s));
    for (int64_t r0 = 0; r0 < total; r0 += chunk) {
      a.r0 = r0, a.r1 = std::min(total, r0 + chunk);
      const int64_t runs = (a.r1 - a.r0 + kPlWaves - 1) / kPlWaves;
      const int blocks = (int)std::min<int64_t>(nbx, runs);
      a.per_block = (runs + blocks - 1) / blocks * kPlWaves;
      for (int64_t b0 = 0; b0 < B; b0 += lab_chunk) {
        a.b0 = (int)b0;
        const unsigned gy = (unsigned)((std::min<int64_t>(lab_chunk, B - b0) + 63) / 64);
        launch_lab<false>(C, a, dim3((unsigned)blocks, gy), s);
        FS_TRY(launch_check("k_pair_lab"));
      }
    }
    k_pair_lab_reduce<<<(unsigned)((B + 255) / 256), 256, 0, s>>>(dpkey, dprank, nbx, B, dokey,
                                                                  dorank);
    FS_TRY(launch_check("k_pair_lab_reduce"));
    FS_HIP(hipEventRecord(ev[4], s));
    FS_HIP(hipMemcpyAsync(hkey.data(), dokey, (size_t)B * 8, hipMemcpyDeviceToHost, s));
    FS_HIP(hipMemcpyAsync(hrank.data(), dorank, (size_t)B * 8, hipMemcpyDeviceToHost, s));
    if (relevance)
      FS_HIP(hipMemcpyAsync(hrel.data(), drel, (size_t)p * B * 8, hipMemcpyDeviceToHost, s));
  } else {
    // one class over all rows: every J and every relevance is exactly 0.0
    FS_HIP(hipEventRecord(ev[3], s));
    FS_HIP(hipEventRecord(ev[4], s));
    for (int b = 0; b < B; b++) hkey[(size_t)b] = pair_key(0.0), hrank[(size_t)b] = 0;
    std::fill(hrel.begin(), hrel.end(), 0.0);
  }
  FS_HIP(hipEventRecord(ev[5], s));
  FS_HIP(hipStreamSynchronize(s));
  for (int b = 0; b < B; b++) {
    best_score[b] = pair_score(hkey[(size_t)b]);
    pair_unrank(p, hrank[(size_t)b], best_i[b], best_j[b]);
  }
  if (relevance)  // the device holds rel[f][b]
    for (int b = 0; b < B; b++)
      for (int64_t f = 0; f < p; f++)
        relevance[(size_t)b * p + f] = hrel[(size_t)f * B + b];
  store_times(ev);
  return FS_OK;
}

}  // namespace gpu
}  // namespace fs
