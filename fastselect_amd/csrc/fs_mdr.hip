// fs_mdr.hip -- the GPU backend of fs_mdr_scan (MDR.py:20-79 mdr_kernel, for
// every fold at once).
//
//   k_mdr_pack   X (bytes, uploaded once) -> genotype bit-planes in the
//                segment layout of fs_mdr.h: planes[(w * 3 + g) * p + j], u32
//                words, column index fastest.  Lanes that scan neighbouring
//                ranks differ in their last column only, so their plane loads
//                are consecutive words and the leading columns' loads are one
//                word for the whole wave.
//   k_mdr_scan   one lane per combination rank, unranked on the device from
//                its int64 rank.  Cell-major: for a cell of the first k-1
//                columns the lane walks the words segment by segment and keeps
//                popcount(AND) per (fold, class) for the last column's three
//                genotypes in registers; a fold's training counts are the
//                totals minus its own.  No 3^k table exists.  Up to kMdrG
//                folds per launch; more run in groups, each walking the other
//                folds' words for the totals.  A lane takes its ranks
//                in ascending order and keeps its best (BA bits, iteration);
//                the block reduces (max BA, min rank) per fold and merges it
//                into its slot of the partials, which the host reduces.  No
//                atomics: the result is deterministic.  A block owns a
//                contiguous run of ranks: a lane unranks once and then steps
//                its combination by the block size (mdr_advance).
//
//                fs_mdr_scan_top runs the same kernel in two more modes (a
//                histogram of the BAs, then an append of those above a
//                threshold): see mdr_scan_top below.
//
// The GPU backend of fs_mdr_scan_labels (one lane per labelling) follows
// below, with its own layout and kernels.
#include <type_traits>

#include "fs_gpu_internal.h"
#include "fs_mdr.h"

namespace fs {
namespace gpu {

namespace {

constexpr int kMdrG = 16;          // folds held in registers per launch
constexpr int kMdrThreads = 256;
constexpr int kMdrMaxBlocks = 2048;
constexpr uint32_t kNoIter = 0xffffffffu;

// Launch sizes.  The test hooks "mdr_ranks" and "mdr_blocks" shrink them so
// that a small search takes several launches and a block several steps of
// mdr_advance; at 0 the arguments come back as they are.
inline int64_t launch_ranks(int64_t computed) {
  const int64_t h = test_hooks().mdr_ranks;
  return h > 0 ? h : computed;
}
inline int64_t launch_blocks(int64_t cap) {
  const int64_t h = test_hooks().mdr_blocks;
  return h > 0 ? std::min(h, cap) : cap;
}

// The 32 samples at perm[0..32) of column j -> the column's three genotype
// words; true when a genotype is above 2.
__device__ __forceinline__ bool pack_word(const uint8_t* __restrict__ x, int64_t p,
                                          const int32_t* __restrict__ perm, int64_t j,
                                          uint32_t& b0, uint32_t& b1, uint32_t& b2) {
  b0 = b1 = b2 = 0;
  bool wrong = false;
  for (int b = 0; b < 32; b++) {
    const int32_t i = perm[b];
    if (i < 0) continue;
    const uint8_t g = x[(size_t)i * p + j];
    b0 |= (uint32_t)(g == 0) << b;
    b1 |= (uint32_t)(g == 1) << b;
    b2 |= (uint32_t)(g == 2) << b;
    wrong |= g > 2;
  }
  return wrong;
}

// One thread per (word, column): 32 samples of one column -> three words.
__global__ __launch_bounds__(256) void k_mdr_pack(const uint8_t* __restrict__ x, int64_t p,
                                                  const int32_t* __restrict__ perm, int64_t words,
                                                  uint32_t* __restrict__ planes,
                                                  int* __restrict__ bad) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t w = blockIdx.y;
  if (j >= p || w >= words) return;
  uint32_t b0, b1, b2;
  const bool wrong = pack_word(x, p, perm + w * 32, j, b0, b1, b2);
  planes[((size_t)w * 3 + 0) * p + j] = b0;
  planes[((size_t)w * 3 + 1) * p + j] = b1;
  planes[((size_t)w * 3 + 2) * p + j] = b2;
  if (wrong) atomicOr(bad, 1);
}

struct MdrScanArgs {
  const uint32_t* planes;
  int64_t p;
  const int32_t* seg_off;   // 2F + 1 word offsets, segment c * F + f
  const int64_t* tc;        // F training cases
  const int64_t* tn;        // F training controls
  int F, f0, gn, sub;       // this launch scores folds [f0, f0 + gn)
  int64_t count, r0, r1;    // C(p,k) and this launch's rank range
  int64_t per_block;        // ranks per block, a multiple of the block size
  float* ba_out;            // NULL or F x count
  uint32_t* part_bits;      // kMdrMaxBlocks x F
  int64_t* part_rank;
  // fs_mdr_scan_top's two scans only
  unsigned long long* hist = nullptr;  // F x kMdrBins
  const uint32_t* thr = nullptr;       // F: a candidate of fold f has bits >= thr[f]
  uint32_t* cursor = nullptr;          // F: candidates of fold f appended so far
  const uint32_t* cand_off = nullptr;  // F + 1: fold f owns [cand_off[f], cand_off[f + 1])
  uint32_t* cand_bits = nullptr;
  int64_t* cand_rank = nullptr;
};

// What a scan does with a combination's balanced accuracies: keep the best
// (fs_mdr_scan), count them per histogram bin, or append those at or above a
// fold's threshold to the fold's candidates (the two scans of fs_mdr_scan_top).
enum { kScanBest = 0, kScanHist = 1, kScanCollect = 2 };

// popcount(AND) over the words [w0, w1) for the last column's three genotypes
template <int K>
__device__ __forceinline__ void count3(const uint32_t* const* pre, const uint32_t* last,
                                       size_t p, int w0, int w1, uint32_t& a0, uint32_t& a1,
                                       uint32_t& a2) {
  for (int w = w0; w < w1; w++) {
    const size_t o = (size_t)w * 3 * p;
    uint32_t m = 0xffffffffu;
#pragma unroll
    for (int t = 0; t < K - 1; t++) m &= pre[t][o];
    a0 += __popc(m & last[o]);
    a1 += __popc(m & last[o + p]);
    a2 += __popc(m & last[o + 2 * p]);
  }
}

// A read-only table of a launch, as k_mdr_scan reads it in mode MODE.
template <class T>
using ConstSpace = const __attribute__((address_space(4))) T;
template <int MODE, class T>
using Table = std::conditional_t<MODE == kScanCollect, ConstSpace<T>, const T>;

template <int K, int G, int MODE = kScanBest>
__global__ __launch_bounds__(kMdrThreads) void k_mdr_scan(const MdrScanArgs a) {
  __shared__ uint32_t s_bits[kMdrThreads / 64];
  __shared__ int64_t s_rank[kMdrThreads / 64];
  // kScanHist: the block's own histogram, added to the global one at the end
  // (integer sums: the order of the adds does not show)
  __shared__ uint32_t s_hist[MODE == kScanHist ? G * kMdrBins : 1];
  const int tid = threadIdx.x;
  const int F = a.F, f0 = a.f0, gn = a.gn;
  const size_t p = (size_t)a.p;
  // The launch's small tables.  kScanCollect stores inside the rank loop, and
  // a kernel that stores reads its wave-uniform tables with vector loads
  // unless they come through the constant address space (as the planes of
  // k_mdr_scan_labels do); the other modes read them as before.
  Table<MODE, int32_t>* const seg_off = (Table<MODE, int32_t>*)a.seg_off;
  Table<MODE, int64_t>* const tot_c = (Table<MODE, int64_t>*)a.tc;
  Table<MODE, int64_t>* const tot_n = (Table<MODE, int64_t>*)a.tn;
  [[maybe_unused]] Table<MODE, uint32_t>* const thr = (Table<MODE, uint32_t>*)a.thr;
  [[maybe_unused]] Table<MODE, uint32_t>* const cand_off = (Table<MODE, uint32_t>*)a.cand_off;
  // the block owns a contiguous run of ranks and takes it 256 at a time
  const int64_t first = a.r0 + (int64_t)blockIdx.x * a.per_block + tid;
  const int64_t end = min(a.r1, a.r0 + ((int64_t)blockIdx.x + 1) * a.per_block);
  int cells = 1;
#pragma unroll
  for (int t = 1; t < K; t++) cells *= 3;

  uint32_t best_bits[G], best_it[G];
#pragma unroll
  for (int i = 0; i < G; i++) best_bits[i] = 0, best_it[i] = kNoIter;
  if constexpr (MODE == kScanHist) {
    for (int j = tid; j < gn * kMdrBins; j += kMdrThreads) s_hist[j] = 0;
    __syncthreads();
  }

  uint32_t it = 0;
  int32_t f[K];
  for (int64_t r = first; r < end; r += kMdrThreads, it++) {
    if (it == 0) mdr_unrank(a.p, K, r, f);
    else mdr_advance(a.p, K, f, kMdrThreads);
    uint32_t tp[G], tn[G];
#pragma unroll
    for (int i = 0; i < G; i++) tp[i] = tn[i] = 0;
    const uint32_t* last = a.planes + f[K - 1];
    for (int cell = 0; cell < cells; cell++) {
      const uint32_t* pre[K > 1 ? K - 1 : 1];
      {
        int c = cell;
#pragma unroll
        for (int t = K - 2; t >= 0; t--) {
          pre[t] = a.planes + (size_t)(c % 3) * p + f[t];
          c /= 3;
        }
      }
      uint32_t cc[3][G], ct[3][G], totc[3] = {0, 0, 0}, totn[3] = {0, 0, 0};
      if (gn < F) {  // the other folds' words count towards the totals only
        count3<K>(pre, last, p, seg_off[0], seg_off[f0], totc[0], totc[1], totc[2]);
        count3<K>(pre, last, p, seg_off[f0 + gn], seg_off[F], totc[0], totc[1], totc[2]);
        count3<K>(pre, last, p, seg_off[F], seg_off[F + f0], totn[0], totn[1], totn[2]);
        count3<K>(pre, last, p, seg_off[F + f0 + gn], seg_off[2 * F], totn[0], totn[1],
                  totn[2]);
      }
#pragma unroll
      for (int i = 0; i < G; i++) {
#pragma unroll
        for (int g = 0; g < 3; g++) cc[g][i] = ct[g][i] = 0;
        if (i < gn) {
          count3<K>(pre, last, p, seg_off[f0 + i], seg_off[f0 + i + 1], cc[0][i], cc[1][i],
                    cc[2][i]);
          count3<K>(pre, last, p, seg_off[F + f0 + i], seg_off[F + f0 + i + 1], ct[0][i],
                    ct[1][i], ct[2][i]);
#pragma unroll
          for (int g = 0; g < 3; g++) totc[g] += cc[g][i], totn[g] += ct[g][i];
        }
      }
#pragma unroll
      for (int i = 0; i < G; i++) {
        if (i < gn) {
          const uint64_t TC = (uint64_t)tot_c[f0 + i], TN = (uint64_t)tot_n[f0 + i];
#pragma unroll
          for (int g = 0; g < 3; g++) {
            const uint32_t cs = totc[g] - (a.sub ? cc[g][i] : 0);
            const uint32_t cn = totn[g] - (a.sub ? ct[g][i] : 0);
            const bool high = mdr_high_risk(cs, cn, TC, TN);
            tp[i] += high ? cs : 0;
            tn[i] += high ? 0 : cn;
          }
        }
      }
    }
    uint32_t hit = 0, hit_bits[MODE == kScanCollect ? G : 1];  // kScanCollect: folds to append to
#pragma unroll
    for (int i = 0; i < G; i++) {
      if (i < gn) {
        const float ba = mdr_ba(tp[i], tn[i], (uint64_t)tot_c[f0 + i], (uint64_t)tot_n[f0 + i]);
        if (a.ba_out) a.ba_out[(size_t)(f0 + i) * a.count + r] = ba;
        const uint32_t bits = __float_as_uint(ba);
        if constexpr (MODE == kScanHist) {
          atomicAdd(&s_hist[i * kMdrBins + mdr_bin(bits)], 1u);  // mdr_bin() < kMdrBins
        } else if constexpr (MODE == kScanCollect) {
          hit_bits[i] = bits;
          hit |= bits >= thr[f0 + i] ? 1u << i : 0u;
        } else {
          // ranks ascend with `it`, so a strict improvement keeps the smallest
          if (best_it[i] == kNoIter || bits > best_bits[i]) best_bits[i] = bits, best_it[i] = it;
        }
      }
    }
    if constexpr (MODE == kScanCollect) {
      // rare (about n_top lanes of the whole scan), so one branch for all the
      // folds keeps it out of the loop's way.  Any append order will do: the
      // candidates are sorted by a total order afterwards
      if (hit) {
#pragma unroll
        for (int i = 0; i < G; i++) {
          if (hit & (1u << i)) {
            const uint32_t o = cand_off[f0 + i], room = cand_off[f0 + i + 1] - o;
            const uint32_t at = atomicAdd(&a.cursor[f0 + i], 1u);
            if (at < room) a.cand_bits[o + at] = hit_bits[i], a.cand_rank[o + at] = r;
          }
        }
      }
    }
  }
  if constexpr (MODE == kScanHist) {
    __syncthreads();
    for (int j = tid; j < gn * kMdrBins; j += kMdrThreads)
      if (s_hist[j]) atomicAdd(&a.hist[(size_t)f0 * kMdrBins + j], (unsigned long long)s_hist[j]);
  }
  if constexpr (MODE != kScanBest) return;

  // per fold: wave reduce, then the block's four waves, then the block's slot
#pragma unroll
  for (int i = 0; i < G; i++) {
    if (i < gn) {
      uint32_t bits = best_bits[i];
      int64_t rank = best_it[i] == kNoIter ? kMdrNoRank : first + (int64_t)best_it[i] * kMdrThreads;
      for (int d = 32; d > 0; d >>= 1) {
        const uint32_t ob = __shfl_xor(bits, d, 64);
        const int64_t orank = __shfl_xor((long long)rank, d, 64);
        if (mdr_better(ob, orank, bits, rank)) bits = ob, rank = orank;
      }
      if ((tid & 63) == 0) s_bits[tid >> 6] = bits, s_rank[tid >> 6] = rank;
      __syncthreads();
      if (tid == 0) {
        for (int w = 1; w < kMdrThreads / 64; w++)
          if (mdr_better(s_bits[w], s_rank[w], bits, rank)) bits = s_bits[w], rank = s_rank[w];
        const size_t slot = (size_t)blockIdx.x * F + f0 + i;
        if (mdr_better(bits, rank, a.part_bits[slot], a.part_rank[slot]))
          a.part_bits[slot] = bits, a.part_rank[slot] = rank;
      }
      __syncthreads();
    }
  }
}

template <int K>
void launch_scan(const MdrScanArgs& a, int blocks, hipStream_t s) {
  if (a.F == 1)
    k_mdr_scan<K, 1><<<blocks, kMdrThreads, 0, s>>>(a);
  else
    k_mdr_scan<K, kMdrG><<<blocks, kMdrThreads, 0, s>>>(a);
}

// The two scans of fs_mdr_scan_top; MODE is kScanHist or kScanCollect.
template <int K, int MODE>
void launch_top(const MdrScanArgs& a, int blocks, hipStream_t s) {
  if (a.F == 1)
    k_mdr_scan<K, 1, MODE><<<blocks, kMdrThreads, 0, s>>>(a);
  else
    k_mdr_scan<K, kMdrG, MODE><<<blocks, kMdrThreads, 0, s>>>(a);
}

template <int MODE>
void launch_top_k(int k, const MdrScanArgs& a, int blocks, hipStream_t s) {
  switch (k) {
    case 1: launch_top<1, MODE>(a, blocks, s); break;
    case 2: launch_top<2, MODE>(a, blocks, s); break;
    case 3: launch_top<3, MODE>(a, blocks, s); break;
    case 4: launch_top<4, MODE>(a, blocks, s); break;
    case 5: launch_top<5, MODE>(a, blocks, s); break;
    default: launch_top<6, MODE>(a, blocks, s); break;
  }
}

// ---- fs_mdr_scan_labels: one lane per labelling ---------------------------
//
//   The fold-only layout (mdr_fold_layout) is built on quads, four words =
//   128 samples: a fold's segment is a whole number of quads, so every quad
//   of a plane is one aligned 16-byte load.
//   k_mdr_pack_cols    as k_mdr_pack on that layout, word index fastest
//   k_mdr_pack_labels  labels (bytes) -> y[(q * B + b) * 4 + i]: word i of quad
//                      q under labelling b; within a quad the labelling index
//                      is fastest, so a wave's 16-byte loads are consecutive
//   k_mdr_scan_labels  a wave takes one combination at a time and its 64 lanes
//                      take 64 labellings.  The combination is wave-uniform,
//                      so the plane loads, the ANDs of the k columns and the
//                      per-(genotype, fold) cell counts are scalar work done
//                      once for 64 labellings; a lane adds popcount(cell &
//                      its label word) and keeps case counts only (controls =
//                      cell count - cases).  The four waves of a block take
//                      interleaved ranks of the block's run; the block merges
//                      (max BA, min rank) per (labelling, fold) into its slot
//   k_mdr_labels_reduce  the slots of all blocks -> [B][F], on the device
constexpr int kMdrLabWaves = kMdrThreads / 64;
constexpr int kMdrLabMaxBlocks = 1024;         // rank runs (grid.x) per launch
constexpr size_t kMdrLabMaxSlots = (size_t)1 << 24;

// k_mdr_pack with the word index fastest: planes[(j * 3 + g) * words + w].
// A wave of the labels scan reads one column's words in a row through the
// scalar cache.  One thread per (word, column); perm covers all the words.
__global__ __launch_bounds__(256) void k_mdr_pack_cols(const uint8_t* __restrict__ x, int64_t p,
                                                       const int32_t* __restrict__ perm,
                                                       int64_t words, int64_t w0,
                                                       uint32_t* __restrict__ planes,
                                                       int* __restrict__ bad) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t w = w0 + blockIdx.y;
  if (j >= p || w >= words) return;
  uint32_t b0, b1, b2;
  const bool wrong = pack_word(x, p, perm + w * 32, j, b0, b1, b2);
  planes[((size_t)j * 3 + 0) * words + w] = b0;
  planes[((size_t)j * 3 + 1) * words + w] = b1;
  planes[((size_t)j * 3 + 2) * words + w] = b2;
  if (wrong) atomicOr(bad, 1);
}

// One thread per (word, labelling).
__global__ __launch_bounds__(256) void k_mdr_pack_labels(const uint8_t* __restrict__ labels,
                                                         int64_t n, int B,
                                                         const int32_t* __restrict__ perm,
                                                         int64_t words, int64_t w0,
                                                         uint32_t* __restrict__ y) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t w = w0 + blockIdx.y;
  if (b >= B || w >= words) return;
  uint32_t bits = 0;
  for (int i = 0; i < 32; i++) {
    const int32_t s = perm[w * 32 + i];
    if (s >= 0) bits |= (uint32_t)(labels[(size_t)b * n + s] != 0) << i;
  }
  y[((size_t)(w >> 2) * B + b) * 4 + (w & 3)] = bits;
}

__global__ __launch_bounds__(256) void k_mdr_labels_fill(uint32_t* __restrict__ bits,
                                                         int64_t* __restrict__ rank, size_t slots) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < slots) bits[i] = 0, rank[i] = kMdrNoRank;
}

// A quad: four words = 128 samples.  The planes are read-only for the whole
// kernel and every wave reads them at wave-uniform addresses: loads through
// the constant address space stay on the scalar unit whatever the kernel
// stores elsewhere.
typedef uint32_t Quad __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) Quad PlaneQuad;

struct MdrLabelArgs {
  const Quad* planes;      // [(column * 3 + genotype) * quads + q]
  int64_t p, quads;
  const Quad* y;            // quads x B
  const int32_t* seg_off;   // F + 1 quad offsets
  const uint32_t* tc;       // F x B training cases
  const uint32_t* tn;       // F x B training controls
  int B, b0;                // grid.y * 64 + lane + b0 is the lane's labelling
  int F, f0, gn, sub;       // this launch scores folds [f0, f0 + gn)
  int64_t count, r0, r1;    // C(p,k) and this launch's rank range
  int64_t per_block;        // ranks per block, a multiple of the waves per block
  float* ba_out;            // NULL or B x F x count
  uint32_t* part_bits;      // blocks x F x B
  int64_t* part_rank;
};

__device__ __forceinline__ uint32_t popc4(Quad v) {
  return __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
}

// Over the quads [q0, q1): the cell's count (wave-uniform) and the lane's
// case count for the last column's three genotypes.  A plane's quad is one
// 16-byte scalar load and the lane's four label words one 16-byte vector load.
template <int K>
__device__ __forceinline__ void count3_labels(PlaneQuad* const* pre, PlaneQuad* last,
                                              size_t Q, const Quad* y, size_t B, uint32_t b,
                                              uint32_t q0, uint32_t q1, uint32_t* n, uint32_t& a0,
                                              uint32_t& a1, uint32_t& a2) {
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
  for (uint32_t q = q0; q < q1; q++) {
    Quad m = ~(Quad)0u;
#pragma unroll
    for (int t = 0; t < K - 1; t++) m &= pre[t][q];
    const Quad c0 = m & last[q], c1 = m & last[Q + q], c2 = m & last[2 * Q + q];
    const Quad yw = (y + (size_t)q * B)[b];
    n[0] += popc4(c0), n[1] += popc4(c1), n[2] += popc4(c2);
    a0 += popc4(c0 & yw), a1 += popc4(c1 & yw), a2 += popc4(c2 & yw);
  }
}

template <int K, int G>
__global__ __launch_bounds__(kMdrThreads) void k_mdr_scan_labels(const MdrLabelArgs a) {
  __shared__ uint32_t s_bits[kMdrLabWaves][64];
  __shared__ int64_t s_rank[kMdrLabWaves][64];
  __shared__ uint32_t s_tp[G][kMdrThreads], s_tn[G][kMdrThreads];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int F = a.F, f0 = a.f0, gn = a.gn;
  const size_t Q = (size_t)a.quads, B = (size_t)a.B;
  const int64_t bl = (int64_t)a.b0 + (int64_t)blockIdx.y * 64 + lane;
  const bool live = bl < a.B;
  // a lane past the last labelling computes the last one's and writes nothing
  const uint32_t b = (uint32_t)(live ? bl : a.B - 1);
  const Quad* y = a.y;
  const int64_t first = a.r0 + (int64_t)blockIdx.x * a.per_block + wave;
  const int64_t end = min(a.r1, a.r0 + ((int64_t)blockIdx.x + 1) * a.per_block);
  int cells = 1;
#pragma unroll
  for (int t = 1; t < K; t++) cells *= 3;

  uint32_t best_bits[G], best_it[G];
#pragma unroll
  for (int i = 0; i < G; i++) best_bits[i] = 0, best_it[i] = kNoIter;

  uint32_t it = 0;
  int32_t f[K];
  for (int64_t r = first; r < end; r += kMdrLabWaves, it++) {
    if (it == 0) mdr_unrank(a.p, K, r, f);
    else mdr_advance(a.p, K, f, kMdrLabWaves);
#pragma unroll
    for (int t = 0; t < K; t++) f[t] = __builtin_amdgcn_readfirstlane(f[t]);
    uint32_t tp[G], tn[G];
#pragma unroll
    for (int i = 0; i < G; i++) tp[i] = tn[i] = 0;
    PlaneQuad* const planes = (PlaneQuad*)a.planes;
    PlaneQuad* last = planes + (size_t)f[K - 1] * 3 * Q;
    for (int cell = 0; cell < cells; cell++) {
      PlaneQuad* pre[K > 1 ? K - 1 : 1];
      {
        int c = cell;
#pragma unroll
        for (int t = K - 2; t >= 0; t--) {
          pre[t] = planes + ((size_t)f[t] * 3 + c % 3) * Q;
          c /= 3;
        }
      }
      // cn: the cell's count in a fold (uniform); cs: the lane's cases there
      uint32_t cn[G][3], cs[3][G], totn[3] = {0, 0, 0}, tots[3] = {0, 0, 0};
      if (gn < F) {  // the other folds' words count towards the totals only
        count3_labels<K>(pre, last, Q, y, B, b, a.seg_off[0], a.seg_off[f0], totn, tots[0],
                         tots[1], tots[2]);
        count3_labels<K>(pre, last, Q, y, B, b, a.seg_off[f0 + gn], a.seg_off[F], totn, tots[0],
                         tots[1], tots[2]);
      }
#pragma unroll
      for (int i = 0; i < G; i++) {
#pragma unroll
        for (int g = 0; g < 3; g++) cn[i][g] = cs[g][i] = 0;
        if (i < gn) {
          count3_labels<K>(pre, last, Q, y, B, b, a.seg_off[f0 + i], a.seg_off[f0 + i + 1],
                           cn[i], cs[0][i], cs[1][i], cs[2][i]);
#pragma unroll
          for (int g = 0; g < 3; g++) totn[g] += cn[i][g], tots[g] += cs[g][i];
        }
      }
#pragma unroll
      for (int i = 0; i < G; i++) {
        if (i < gn) {
          const uint64_t TC = (a.tc + (size_t)(f0 + i) * B)[b], TN = (a.tn + (size_t)(f0 + i) * B)[b];
#pragma unroll
          for (int g = 0; g < 3; g++) {
            const uint32_t s = tots[g] - (a.sub ? cs[g][i] : 0);
            const uint32_t c = (totn[g] - tots[g]) - (a.sub ? cn[i][g] - cs[g][i] : 0);
            const bool high = mdr_high_risk(s, c, TC, TN);
            tp[i] += high ? s : 0;
            tn[i] += high ? 0 : c;
          }
        }
      }
    }
    // The BAs come out of a loop that stays rolled, through the lane's own
    // column of LDS.  Unrolled, the float64 divisions by a fold's totals are
    // loop-invariant in part; the compiler hoists those parts out of the rank
    // loop for all G folds at once, which costs some 200 registers.
#pragma unroll
    for (int i = 0; i < G; i++)
      if (i < gn) s_tp[i][tid] = tp[i], s_tn[i][tid] = tn[i];
#pragma unroll 1
    for (int i = 0; i < gn; i++) {
      const float ba = mdr_ba(s_tp[i][tid], s_tn[i][tid], (a.tc + (size_t)(f0 + i) * B)[b],
                              (a.tn + (size_t)(f0 + i) * B)[b]);
      if (a.ba_out && live) a.ba_out[((size_t)b * F + f0 + i) * (size_t)a.count + r] = ba;
      s_tp[i][tid] = __float_as_uint(ba);
    }
#pragma unroll
    for (int i = 0; i < G; i++) {
      if (i < gn) {
        const uint32_t bits = s_tp[i][tid];
        // ranks ascend with `it`, so a strict improvement keeps the smallest
        if (best_it[i] == kNoIter || bits > best_bits[i]) best_bits[i] = bits, best_it[i] = it;
      }
    }
  }

  // per fold: the block's waves hold the same labellings; merge them, then
  // the block's slot (one block owns it in every launch: no atomics)
#pragma unroll
  for (int i = 0; i < G; i++) {
    if (i < gn) {
      s_bits[wave][lane] = best_bits[i];
      s_rank[wave][lane] =
          best_it[i] == kNoIter ? kMdrNoRank : first + (int64_t)best_it[i] * kMdrLabWaves;
      __syncthreads();
      if (tid < 64 && live) {
        uint32_t bits = s_bits[0][lane];
        int64_t rank = s_rank[0][lane];
        for (int w = 1; w < kMdrLabWaves; w++)
          if (mdr_better(s_bits[w][lane], s_rank[w][lane], bits, rank))
            bits = s_bits[w][lane], rank = s_rank[w][lane];
        const size_t slot = ((size_t)blockIdx.x * F + f0 + i) * B + b;
        if (mdr_better(bits, rank, a.part_bits[slot], a.part_rank[slot]))
          a.part_bits[slot] = bits, a.part_rank[slot] = rank;
      }
      __syncthreads();
    }
  }
}

// One thread per (fold, labelling): the best over the blocks' slots.
__global__ __launch_bounds__(256) void k_mdr_labels_reduce(const uint32_t* __restrict__ part_bits,
                                                           const int64_t* __restrict__ part_rank,
                                                           int blocks, int F, int B,
                                                           uint32_t* __restrict__ out_bits,
                                                           int64_t* __restrict__ out_rank) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, FB = (size_t)F * B;
  if (i >= FB) return;
  uint32_t bits = 0;
  int64_t rank = kMdrNoRank;
  for (int x = 0; x < blocks; x++) {
    const size_t slot = (size_t)x * FB + i;
    if (mdr_better(part_bits[slot], part_rank[slot], bits, rank))
      bits = part_bits[slot], rank = part_rank[slot];
  }
  const size_t o = (i % B) * F + i / B;  // [labelling][fold]
  out_bits[o] = bits, out_rank[o] = rank;
}

template <int K>
void launch_scan_labels(const MdrLabelArgs& a, dim3 grid, hipStream_t s) {
  // the usual cv = 5 and cv = 10 get kernels that hold just their folds: the
  // registers a fold takes decide how many waves a SIMD holds
  if (a.gn == 1)
    k_mdr_scan_labels<K, 1><<<grid, kMdrThreads, 0, s>>>(a);
  else if (a.gn <= 5)
    k_mdr_scan_labels<K, 5><<<grid, kMdrThreads, 0, s>>>(a);
  else if (a.gn <= 10)
    k_mdr_scan_labels<K, 10><<<grid, kMdrThreads, 0, s>>>(a);
  else
    k_mdr_scan_labels<K, kMdrG><<<grid, kMdrThreads, 0, s>>>(a);
}

}  // namespace

int mdr_scan(int device, const uint8_t* x, int64_t n, int64_t p, const uint8_t* is_case, int k,
             const int32_t* fold, int n_folds, int64_t count, float* best_ba, int64_t* best_rank,
             float* ba_out) {
  if (device_count() <= 0) {
    set_error("backend='gpu' requested but no HIP device is visible");
    return FS_ENODEV;
  }
  MdrLayout L;
  if (int rc = mdr_layout(n, is_case, fold, n_folds, 32, L)) return rc;
  const int F = L.F;
  const int64_t W = L.words;
  const size_t nslots = (size_t)kMdrMaxBlocks * F;
  std::vector<uint32_t> h_bits(nslots, 0);
  std::vector<int64_t> h_rank(nslots, kMdrNoRank);

  uint8_t* dx = nullptr;
  int32_t *dperm = nullptr, *dseg = nullptr;
  int64_t *dtc = nullptr, *dtn = nullptr, *dprank = nullptr;
  uint32_t *dplanes = nullptr, *dpbits = nullptr;
  float* dba = nullptr;
  int* dbad = nullptr;
  hipStream_t s = nullptr;
  int rc = FS_OK;
  auto fail = [&](const char* what, hipError_t e) {
    set_error(std::string("fs_mdr_scan: ") + what + ": " + hipGetErrorString(e));
    (void)hipGetLastError();
    rc = (e == hipErrorOutOfMemory) ? FS_EOOM : FS_EHIP;
  };
  auto up = [&](void* dst, const void* src, size_t bytes, const char* what) {
    hipError_t e;
    if (rc == FS_OK && (e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s)) != hipSuccess)
      fail(what, e);
  };
  hipError_t e;
  if ((e = hipSetDevice(device)) != hipSuccess) fail("hipSetDevice", e);
  if (rc == FS_OK && (e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) != hipSuccess)
    fail("hipStreamCreate", e);
  const size_t plane_words = (size_t)W * 3 * (size_t)p;
  DevArena mem(device);  // freed on return, after the stream is synchronised
  if (rc == FS_OK) rc = mem.alloc(&dx, (size_t)n * p);
  if (rc == FS_OK) rc = mem.alloc(&dperm, L.perm.size());
  if (rc == FS_OK) rc = mem.alloc(&dseg, L.seg_off.size());
  if (rc == FS_OK) rc = mem.alloc(&dtc, (size_t)F);
  if (rc == FS_OK) rc = mem.alloc(&dtn, (size_t)F);
  if (rc == FS_OK) rc = mem.alloc(&dplanes, plane_words);
  if (rc == FS_OK) rc = mem.alloc(&dpbits, nslots);
  if (rc == FS_OK) rc = mem.alloc(&dprank, nslots);
  if (rc == FS_OK) rc = mem.alloc(&dbad, 1);
  if (rc == FS_OK && ba_out) rc = mem.alloc(&dba, (size_t)F * count);
  up(dx, x, (size_t)n * p, "upload of X");
  up(dperm, L.perm.data(), L.perm.size() * 4, "upload of the sample order");
  up(dseg, L.seg_off.data(), L.seg_off.size() * 4, "upload of the segments");
  up(dtc, L.tc.data(), (size_t)F * 8, "upload of the totals");
  up(dtn, L.tn.data(), (size_t)F * 8, "upload of the totals");
  up(dpbits, h_bits.data(), nslots * 4, "upload of the partials");
  up(dprank, h_rank.data(), nslots * 8, "upload of the partials");
  if (rc == FS_OK && (e = hipMemsetAsync(dbad, 0, 4, s)) != hipSuccess) fail("hipMemset", e);

  if (rc == FS_OK) {
    // grid.y is limited to 65535: pack the words in slabs
    const unsigned gx = (unsigned)((p + 255) / 256);
    for (int64_t w0 = 0; w0 < W && rc == FS_OK; w0 += 65535) {
      const int64_t wn = std::min<int64_t>(65535, W - w0);
      k_mdr_pack<<<dim3(gx, (unsigned)wn), 256, 0, s>>>(dx, p, dperm + w0 * 32, wn,
                                                        dplanes + (size_t)w0 * 3 * p, dbad);
      if ((e = hipGetLastError()) != hipSuccess) fail("pack kernel", e);
    }
  }
  int bad = 0;
  if (rc == FS_OK && ((e = hipMemcpyAsync(&bad, dbad, 4, hipMemcpyDeviceToHost, s)) != hipSuccess ||
                      (e = hipStreamSynchronize(s)) != hipSuccess))
    fail("pack", e);
  if (rc == FS_OK && bad) {
    set_error("fs_mdr_scan: genotypes must be coded 0/1/2");
    rc = FS_EINVAL;
  }

  if (rc == FS_OK) {
    // launches of about 2e11 lane operations each (a few milliseconds at the
    // VALU peak), so that no launch holds the device for long
    int cells = 1;
    for (int t = 1; t < k; t++) cells *= 3;
    const int groups = (F + kMdrG - 1) / kMdrG;
    const double ops = (double)cells * (double)W * (k + 5) * (groups > 1 ? 2.0 : 1.0);
    const int64_t chunk = launch_ranks((int64_t)std::max(65536.0, std::min(2e11 / ops, 4e18)));
    MdrScanArgs a;
    a.planes = dplanes, a.p = p, a.seg_off = dseg, a.tc = dtc, a.tn = dtn;
    a.F = F, a.sub = L.sub, a.count = count, a.ba_out = dba;
    a.part_bits = dpbits, a.part_rank = dprank;
    for (int64_t r0 = 0; r0 < count && rc == FS_OK; r0 += chunk) {
      a.r0 = r0, a.r1 = std::min(count, r0 + chunk);
      const int blocks = (int)std::min<int64_t>(
          launch_blocks(kMdrMaxBlocks), (a.r1 - a.r0 + kMdrThreads - 1) / kMdrThreads);
      const int64_t iters = (a.r1 - a.r0 + (int64_t)blocks * kMdrThreads - 1) /
                            ((int64_t)blocks * kMdrThreads);
      a.per_block = iters * kMdrThreads;
      for (int f0 = 0; f0 < F && rc == FS_OK; f0 += kMdrG) {
        a.f0 = f0, a.gn = std::min(kMdrG, F - f0);
        switch (k) {
          case 1: launch_scan<1>(a, blocks, s); break;
          case 2: launch_scan<2>(a, blocks, s); break;
          case 3: launch_scan<3>(a, blocks, s); break;
          case 4: launch_scan<4>(a, blocks, s); break;
          case 5: launch_scan<5>(a, blocks, s); break;
          default: launch_scan<6>(a, blocks, s); break;
        }
        if ((e = hipGetLastError()) != hipSuccess) fail("scan kernel", e);
      }
    }
  }
  if (rc == FS_OK &&
      ((e = hipMemcpyAsync(h_bits.data(), dpbits, nslots * 4, hipMemcpyDeviceToHost, s)) !=
           hipSuccess ||
       (e = hipMemcpyAsync(h_rank.data(), dprank, nslots * 8, hipMemcpyDeviceToHost, s)) !=
           hipSuccess))
    fail("download of the partials", e);
  if (rc == FS_OK && ba_out &&
      (e = hipMemcpyAsync(ba_out, dba, (size_t)F * count * 4, hipMemcpyDeviceToHost, s)) !=
          hipSuccess)
    fail("download of the balanced accuracies", e);
  if (rc == FS_OK && (e = hipStreamSynchronize(s)) != hipSuccess) fail("scan", e);
  if (s) (void)hipStreamSynchronize(s);
  if (rc == FS_OK)
    for (int i = 0; i < F; i++) {
      uint32_t bits = 0;
      int64_t rank = kMdrNoRank;
      for (int b = 0; b < kMdrMaxBlocks; b++) {
        const size_t slot = (size_t)b * F + i;
        if (mdr_better(h_bits[slot], h_rank[slot], bits, rank))
          bits = h_bits[slot], rank = h_rank[slot];
      }
      memcpy(&best_ba[i], &bits, 4);
      best_rank[i] = rank;
    }
  if (s) (void)hipStreamDestroy(s);
  return rc;
}

// ---- fs_mdr_scan_top: the n_top best combinations of every fold -----------
//
//   Scan A   k_mdr_scan<kScanHist>: per fold a histogram of the BAs' leading
//            bits (mdr_bin: 514 bins), kept per block in LDS and added to the
//            global one with integer atomics at the block's end.
//   Threshold (host, 4 KiB per fold): the highest bin h* whose suffix count
//            M reaches min(n_top, C(p,k)).  M is the exact number of BAs at
//            or above the bin's floor, known before any is collected.
//   Scan B   k_mdr_scan<kScanCollect>: the BAs again; a lane at or above its
//            fold's floor appends (bits, rank) to the fold's M entries through
//            an integer cursor.  The host keeps the first n_top under
//            mdr_better's total order, so the append order does not show.
//   Ties     When the folds' M together exceed the candidate cap (masses of
//            equal BAs: monomorphic columns, tiny n, one class), scan B runs
//            over rank chunks small enough for the cap instead, in ascending
//            rank order.  The host merges each chunk into the folds' running
//            lists and raises a full list's threshold to one above its worst
//            BA: a later rank with an equal BA loses the tie anyway.
// Device memory: the planes, F x 514 counters and at most max(cap, F)
// candidates, whatever C(p,k) is.
namespace {
constexpr int64_t kMdrTopCap = (int64_t)1 << 20;  // candidates; test hook "mdr_top_cap"
thread_local double g_mdr_top_ms[4] = {-1.0, -1.0, -1.0, -1.0};
}  // namespace

void mdr_top_last_timing(double* ms4) {
  for (int i = 0; i < 4; i++) ms4[i] = g_mdr_top_ms[i];
}

int mdr_scan_top(int device, const uint8_t* x, int64_t n, int64_t p, const uint8_t* is_case,
                 int k, const int32_t* fold, int n_folds, int64_t count, int n_top, float* top_ba,
                 int64_t* top_rank) {
  if (device_count() <= 0) return no_device();
  for (double& v : g_mdr_top_ms) v = -1.0;
  MdrLayout L;
  FS_TRY(mdr_layout(n, is_case, fold, n_folds, 32, L));
  const int F = L.F;
  const int64_t W = L.words;
  const uint64_t need = (uint64_t)std::min<int64_t>(n_top, count);
  const int64_t cap = test_hooks().mdr_top_cap > 0
                          ? std::min<int64_t>(test_hooks().mdr_top_cap, (int64_t)1 << 30)
                          : kMdrTopCap;
  const int64_t chunk_ranks = std::max<int64_t>(1, cap / F);  // of the tie route

  FS_HIP(hipSetDevice(device));
  DevArena mem(device);
  StreamLease lease(device);  // destroyed (and the stream synchronised) before `mem`
  FS_TRY(lease.open(5));
  hipStream_t s = lease.s;
  std::vector<hipEvent_t>& ev = lease.ev;
  uint8_t* dx = nullptr;
  int32_t *dperm = nullptr, *dseg = nullptr;
  int64_t *dtc = nullptr, *dtn = nullptr, *dcrank = nullptr;
  uint32_t *dplanes = nullptr, *dthr = nullptr, *dcursor = nullptr, *doff = nullptr,
           *dcbits = nullptr;
  unsigned long long* dhist = nullptr;
  int* dbad = nullptr;
  const size_t nhist = (size_t)F * kMdrBins;
  FS_TRY(mem.alloc(&dx, (size_t)n * p));
  FS_TRY(mem.alloc(&dperm, L.perm.size()));
  FS_TRY(mem.alloc(&dseg, L.seg_off.size()));
  FS_TRY(mem.alloc(&dtc, (size_t)F));
  FS_TRY(mem.alloc(&dtn, (size_t)F));
  FS_TRY(mem.alloc(&dplanes, (size_t)W * 3 * (size_t)p));
  FS_TRY(mem.alloc(&dhist, nhist));
  FS_TRY(mem.alloc(&dthr, (size_t)F));
  FS_TRY(mem.alloc(&dcursor, (size_t)F));
  FS_TRY(mem.alloc(&doff, (size_t)F + 1));
  FS_TRY(mem.alloc(&dbad, 1));

  FS_HIP(hipEventRecord(ev[0], s));
  FS_HIP(hipMemcpyAsync(dx, x, (size_t)n * p, hipMemcpyHostToDevice, s));
  FS_HIP(hipMemcpyAsync(dperm, L.perm.data(), L.perm.size() * 4, hipMemcpyHostToDevice, s));
  FS_HIP(hipMemcpyAsync(dseg, L.seg_off.data(), L.seg_off.size() * 4, hipMemcpyHostToDevice, s));
  FS_HIP(hipMemcpyAsync(dtc, L.tc.data(), (size_t)F * 8, hipMemcpyHostToDevice, s));
  FS_HIP(hipMemcpyAsync(dtn, L.tn.data(), (size_t)F * 8, hipMemcpyHostToDevice, s));
  FS_HIP(hipMemsetAsync(dbad, 0, 4, s));
  FS_HIP(hipMemsetAsync(dhist, 0, nhist * 8, s));
  FS_HIP(hipEventRecord(ev[1], s));
  {
    // grid.y is limited to 65535: pack the words in slabs
    const unsigned gx = (unsigned)((p + 255) / 256);
    for (int64_t w0 = 0; w0 < W; w0 += 65535) {
      const int64_t wn = std::min<int64_t>(65535, W - w0);
      k_mdr_pack<<<dim3(gx, (unsigned)wn), 256, 0, s>>>(dx, p, dperm + w0 * 32, wn,
                                                        dplanes + (size_t)w0 * 3 * p, dbad);
      FS_TRY(launch_check("k_mdr_pack"));
    }
  }
  FS_HIP(hipEventRecord(ev[2], s));
  int bad = 0;
  FS_HIP(hipMemcpyAsync(&bad, dbad, 4, hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  if (bad) {
    set_error("fs_mdr_scan_top: genotypes must be coded 0/1/2");
    return FS_EINVAL;
  }

  MdrScanArgs a;
  a.planes = dplanes, a.p = p, a.seg_off = dseg, a.tc = dtc, a.tn = dtn;
  a.F = F, a.sub = L.sub, a.count = count, a.ba_out = nullptr;
  a.part_bits = nullptr, a.part_rank = nullptr;
  a.hist = dhist, a.thr = dthr, a.cursor = dcursor, a.cand_off = doff;
  // one scan of the ranks [r0, r1), every fold group
  auto scan = [&](int mode, int64_t r0, int64_t r1) -> int {
    a.r0 = r0, a.r1 = r1;
    const int blocks = (int)std::min<int64_t>(launch_blocks(kMdrMaxBlocks),
                                              (r1 - r0 + kMdrThreads - 1) / kMdrThreads);
    const int64_t iters =
        (r1 - r0 + (int64_t)blocks * kMdrThreads - 1) / ((int64_t)blocks * kMdrThreads);
    a.per_block = iters * kMdrThreads;
    for (int f0 = 0; f0 < F; f0 += kMdrG) {
      a.f0 = f0, a.gn = std::min(kMdrG, F - f0);
      if (mode == kScanHist) launch_top_k<kScanHist>(k, a, blocks, s);
      else launch_top_k<kScanCollect>(k, a, blocks, s);
      FS_TRY(launch_check("k_mdr_scan"));
    }
    return FS_OK;
  };
  // launches of about 2e11 lane operations each, as in mdr_scan
  int cells = 1;
  for (int t = 1; t < k; t++) cells *= 3;
  const int groups = (F + kMdrG - 1) / kMdrG;
  const double ops = (double)cells * (double)W * (k + 5) * (groups > 1 ? 2.0 : 1.0);
  const int64_t chunk = launch_ranks((int64_t)std::max(65536.0, std::min(2e11 / ops, 4e18)));

  for (int64_t r0 = 0; r0 < count; r0 += chunk)
    FS_TRY(scan(kScanHist, r0, std::min(count, r0 + chunk)));
  std::vector<uint64_t> hist(nhist);
  FS_HIP(hipMemcpyAsync(hist.data(), dhist, nhist * 8, hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  std::vector<uint32_t> thr((size_t)F), off((size_t)F + 1, 0), cursor((size_t)F);
  uint64_t total = 0;
  for (int i = 0; i < F; i++) {
    uint32_t bin;
    uint64_t m;
    mdr_top_threshold(&hist[(size_t)i * kMdrBins], need, &bin, &m);
    if (m < need) {
      set_error("fs_mdr_scan_top: the histogram holds fewer balanced accuracies than combinations");
      return FS_EHIP;
    }
    thr[i] = mdr_bin_floor(bin);
    total += m;
    off[i + 1] = (uint32_t)std::min<uint64_t>(total, UINT32_MAX);
  }
  const bool ties = total > (uint64_t)cap;
  if (ties)
    for (int i = 0; i <= F; i++) off[i] = (uint32_t)(i * chunk_ranks);
  const size_t ncand = off[F];
  FS_TRY(mem.alloc(&dcbits, ncand));
  FS_TRY(mem.alloc(&dcrank, ncand));
  a.cand_bits = dcbits, a.cand_rank = dcrank;
  FS_HIP(hipMemcpyAsync(doff, off.data(), ((size_t)F + 1) * 4, hipMemcpyHostToDevice, s));

  std::vector<MdrTopN> top;
  for (int i = 0; i < F; i++) top.emplace_back((size_t)need);
  std::vector<uint32_t> cbits(ncand);
  std::vector<int64_t> crank(ncand);
  // ranks [r0, r1): collect, then merge the folds' candidates into `top`
  auto collect = [&](int64_t r0, int64_t r1, bool last) -> int {
    FS_HIP(hipMemcpyAsync(dthr, thr.data(), (size_t)F * 4, hipMemcpyHostToDevice, s));
    FS_HIP(hipMemsetAsync(dcursor, 0, (size_t)F * 4, s));
    for (int64_t q0 = r0; q0 < r1; q0 += chunk)
      FS_TRY(scan(kScanCollect, q0, std::min(r1, q0 + chunk)));
    if (last) FS_HIP(hipEventRecord(ev[3], s));
    FS_HIP(hipMemcpyAsync(cursor.data(), dcursor, (size_t)F * 4, hipMemcpyDeviceToHost, s));
    if (ties) {  // the folds' counts first: a chunk leaves most buffers empty
      FS_HIP(hipStreamSynchronize(s));
      for (int i = 0; i < F; i++) {
        const size_t m = std::min<size_t>(cursor[i], off[i + 1] - off[i]);
        if (m == 0) continue;
        FS_HIP(hipMemcpyAsync(&cbits[off[i]], dcbits + off[i], m * 4, hipMemcpyDeviceToHost, s));
        FS_HIP(hipMemcpyAsync(&crank[off[i]], dcrank + off[i], m * 8, hipMemcpyDeviceToHost, s));
      }
    } else if (ncand) {  // every buffer is full: its size is the histogram's count
      FS_HIP(hipMemcpyAsync(cbits.data(), dcbits, ncand * 4, hipMemcpyDeviceToHost, s));
      FS_HIP(hipMemcpyAsync(crank.data(), dcrank, ncand * 8, hipMemcpyDeviceToHost, s));
    }
    FS_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < F; i++) {
      const size_t m = cursor[i], room = off[i + 1] - off[i];
      if (m > room || (!ties && m != room)) {
        set_error("fs_mdr_scan_top: the two scans disagree on the number of candidates");
        return FS_EHIP;
      }
      for (size_t j = off[i]; j < off[i] + m; j++) top[i].push({cbits[j], crank[j]});
      // later ranks lose a tie with the list's worst: only larger BAs count
      if (top[i].full()) thr[i] = std::max(thr[i], top[i].worst().bits + 1);
    }
    return FS_OK;
  };
  if (!ties) {
    FS_TRY(collect(0, count, true));
  } else {
    for (int64_t r0 = 0; r0 < count; r0 += chunk_ranks)
      FS_TRY(collect(r0, std::min(count, r0 + chunk_ranks), r0 + chunk_ranks >= count));
  }
  FS_HIP(hipEventRecord(ev[4], s));
  FS_HIP(hipStreamSynchronize(s));
  for (int i = 0; i < F; i++)
    top[i].sorted_into(top_ba + (size_t)i * n_top, top_rank + (size_t)i * n_top, n_top);
  for (int i = 0; i < 4; i++) {
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) g_mdr_top_ms[i] = ms;
  }
  (void)hipGetLastError();
  return FS_OK;
}

namespace {
thread_local double g_mdr_labels_ms[4] = {-1.0, -1.0, -1.0, -1.0};
}

void mdr_labels_last_timing(double* ms4) {
  for (int i = 0; i < 4; i++) ms4[i] = g_mdr_labels_ms[i];
}

int mdr_scan_labels(int device, const uint8_t* x, int64_t n, int64_t p, const uint8_t* labels,
                    int n_labelings, int k, const int32_t* fold, int n_folds, int64_t count,
                    float* best_ba, int64_t* best_rank, float* ba_out) {
  if (device_count() <= 0) {
    set_error("backend='gpu' requested but no HIP device is visible");
    return FS_ENODEV;
  }
  for (double& v : g_mdr_labels_ms) v = -1.0;
  MdrLayout L;
  if (int rc = mdr_fold_layout(n, fold, n_folds, 128, L)) return rc;
  const int F = L.F, B = n_labelings;
  const int64_t W = L.words * 4;  // L counts quads
  const size_t FB = (size_t)F * B;
  std::vector<uint32_t> tc, tn;
  mdr_label_totals(n, labels, B, L, -1, tc, tn);

  // launches of about 2e11 lane operations each, as in mdr_scan: per
  // (combination, labelling) the word loop issues 6 per cell and word.  The
  // labellings go into one launch as far as that allows, then the ranks.
  int cells = 1;
  for (int t = 1; t < k; t++) cells *= 3;
  const int groups = (F + kMdrG - 1) / kMdrG;
  const double ops = (double)cells * (double)W * 6.0 * (groups > 1 ? 2.0 : 1.0);
  const double pairs = std::max(2e11 / ops, 64.0 * kMdrLabWaves);
  // test hook "mdr_labels": labellings per launch
  const int64_t lab_chunk =
      test_hooks().mdr_labels > 0
          ? std::max<int64_t>(64, test_hooks().mdr_labels / 64 * 64)
          : std::max<int64_t>(64, std::min<int64_t>((B + 63) / 64 * 64,
                                                    (int64_t)(pairs / 256.0) / 64 * 64));
  const int64_t chunk = launch_ranks(
      std::max<int64_t>(kMdrLabWaves, (int64_t)std::min(pairs / (double)lab_chunk, 4e18)));
  // blocks (rank runs) of the largest launch; every launch uses the first ones
  const int64_t max_bx = std::max<int64_t>(
      1, std::min<int64_t>(launch_blocks(kMdrLabMaxBlocks), (int64_t)(kMdrLabMaxSlots / FB)));
  const int nbx = (int)std::min<int64_t>(
      max_bx, (std::min(count, chunk) + kMdrLabWaves - 1) / kMdrLabWaves);
  const size_t nslots = (size_t)nbx * FB;

  uint8_t *dx = nullptr, *dlab = nullptr;
  int32_t *dperm = nullptr, *dseg = nullptr;
  uint32_t *dtc = nullptr, *dtn = nullptr, *dplanes = nullptr, *dy = nullptr, *dpbits = nullptr,
           *dobits = nullptr;
  int64_t *dprank = nullptr, *dorank = nullptr;
  float* dba = nullptr;
  int* dbad = nullptr;
  hipStream_t s = nullptr;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int rc = FS_OK;
  auto fail = [&](const char* what, hipError_t e) {
    set_error(std::string("fs_mdr_scan_labels: ") + what + ": " + hipGetErrorString(e));
    (void)hipGetLastError();
    rc = (e == hipErrorOutOfMemory) ? FS_EOOM : FS_EHIP;
  };
  auto up = [&](void* dst, const void* src, size_t bytes, const char* what) {
    hipError_t e;
    if (rc == FS_OK && (e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s)) != hipSuccess)
      fail(what, e);
  };
  auto mark = [&](int i) {
    hipError_t e;
    if (rc == FS_OK && (e = hipEventRecord(ev[i], s)) != hipSuccess) fail("hipEventRecord", e);
  };
  hipError_t e;
  if ((e = hipSetDevice(device)) != hipSuccess) fail("hipSetDevice", e);
  if (rc == FS_OK && (e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) != hipSuccess)
    fail("hipStreamCreate", e);
  for (int i = 0; i < 5 && rc == FS_OK; i++)
    if ((e = hipEventCreate(&ev[i])) != hipSuccess) fail("hipEventCreate", e);
  DevArena mem(device);  // freed on return, after the stream is synchronised
  if (rc == FS_OK) rc = mem.alloc(&dx, (size_t)n * p);
  if (rc == FS_OK) rc = mem.alloc(&dlab, (size_t)B * n);
  if (rc == FS_OK) rc = mem.alloc(&dperm, L.perm.size());
  if (rc == FS_OK) rc = mem.alloc(&dseg, L.seg_off.size());
  if (rc == FS_OK) rc = mem.alloc(&dtc, FB);
  if (rc == FS_OK) rc = mem.alloc(&dtn, FB);
  if (rc == FS_OK) rc = mem.alloc(&dplanes, (size_t)W * 3 * (size_t)p);
  if (rc == FS_OK) rc = mem.alloc(&dy, (size_t)W * B);
  if (rc == FS_OK) rc = mem.alloc(&dpbits, nslots);
  if (rc == FS_OK) rc = mem.alloc(&dprank, nslots);
  if (rc == FS_OK) rc = mem.alloc(&dobits, FB);
  if (rc == FS_OK) rc = mem.alloc(&dorank, FB);
  if (rc == FS_OK) rc = mem.alloc(&dbad, 1);
  if (rc == FS_OK && ba_out) rc = mem.alloc(&dba, FB * (size_t)count);
  mark(0);
  up(dx, x, (size_t)n * p, "upload of X");
  up(dlab, labels, (size_t)B * n, "upload of the labels");
  up(dperm, L.perm.data(), L.perm.size() * 4, "upload of the sample order");
  up(dseg, L.seg_off.data(), L.seg_off.size() * 4, "upload of the segments");
  up(dtc, tc.data(), FB * 4, "upload of the totals");
  up(dtn, tn.data(), FB * 4, "upload of the totals");
  if (rc == FS_OK && (e = hipMemsetAsync(dbad, 0, 4, s)) != hipSuccess) fail("hipMemset", e);
  mark(1);

  if (rc == FS_OK) {
    // grid.y is limited to 65535: pack the words in slabs
    const unsigned gx = (unsigned)((p + 255) / 256), gb = (unsigned)((B + 255) / 256);
    for (int64_t w0 = 0; w0 < W && rc == FS_OK; w0 += 65535) {
      const int64_t wn = std::min<int64_t>(65535, W - w0);
      k_mdr_pack_cols<<<dim3(gx, (unsigned)wn), 256, 0, s>>>(dx, p, dperm, W, w0, dplanes, dbad);
      if ((e = hipGetLastError()) != hipSuccess) fail("pack kernel", e);
      k_mdr_pack_labels<<<dim3(gb, (unsigned)wn), 256, 0, s>>>(dlab, n, B, dperm, W, w0, dy);
      if (rc == FS_OK && (e = hipGetLastError()) != hipSuccess) fail("label pack kernel", e);
    }
    k_mdr_labels_fill<<<(unsigned)((nslots + 255) / 256), 256, 0, s>>>(dpbits, dprank, nslots);
    if (rc == FS_OK && (e = hipGetLastError()) != hipSuccess) fail("fill kernel", e);
  }
  mark(2);
  int bad = 0;
  if (rc == FS_OK && ((e = hipMemcpyAsync(&bad, dbad, 4, hipMemcpyDeviceToHost, s)) != hipSuccess ||
                      (e = hipStreamSynchronize(s)) != hipSuccess))
    fail("pack", e);
  if (rc == FS_OK && bad) {
    set_error("fs_mdr_scan_labels: genotypes must be coded 0/1/2");
    rc = FS_EINVAL;
  }

  if (rc == FS_OK) {
    MdrLabelArgs a;
    a.planes = (const Quad*)dplanes, a.p = p, a.quads = L.words, a.y = (const Quad*)dy, a.seg_off = dseg, a.tc = dtc, a.tn = dtn;
    a.B = B, a.F = F, a.sub = L.sub, a.count = count, a.ba_out = dba;
    a.part_bits = dpbits, a.part_rank = dprank;
    for (int64_t r0 = 0; r0 < count && rc == FS_OK; r0 += chunk) {
      a.r0 = r0, a.r1 = std::min(count, r0 + chunk);
      const int64_t runs = (a.r1 - a.r0 + kMdrLabWaves - 1) / kMdrLabWaves;
      const int blocks = (int)std::min<int64_t>(nbx, runs);
      a.per_block = (runs + blocks - 1) / blocks * kMdrLabWaves;
      for (int64_t b0 = 0; b0 < B && rc == FS_OK; b0 += lab_chunk) {
        a.b0 = (int)b0;
        const unsigned gy = (unsigned)((std::min<int64_t>(lab_chunk, B - b0) + 63) / 64);
        for (int f0 = 0; f0 < F && rc == FS_OK; f0 += kMdrG) {
          a.f0 = f0, a.gn = std::min(kMdrG, F - f0);
          const dim3 grid((unsigned)blocks, gy);
          switch (k) {
            case 1: launch_scan_labels<1>(a, grid, s); break;
            case 2: launch_scan_labels<2>(a, grid, s); break;
            case 3: launch_scan_labels<3>(a, grid, s); break;
            case 4: launch_scan_labels<4>(a, grid, s); break;
            case 5: launch_scan_labels<5>(a, grid, s); break;
            default: launch_scan_labels<6>(a, grid, s); break;
          }
          if ((e = hipGetLastError()) != hipSuccess) fail("scan kernel", e);
        }
      }
    }
  }
  if (rc == FS_OK) {
    k_mdr_labels_reduce<<<(unsigned)((FB + 255) / 256), 256, 0, s>>>(dpbits, dprank, nbx, F, B,
                                                                      dobits, dorank);
    if ((e = hipGetLastError()) != hipSuccess) fail("reduce kernel", e);
  }
  mark(3);
  if (rc == FS_OK &&
      ((e = hipMemcpyAsync(best_ba, dobits, FB * 4, hipMemcpyDeviceToHost, s)) != hipSuccess ||
       (e = hipMemcpyAsync(best_rank, dorank, FB * 8, hipMemcpyDeviceToHost, s)) != hipSuccess))
    fail("download of the results", e);
  if (rc == FS_OK && ba_out &&
      (e = hipMemcpyAsync(ba_out, dba, FB * (size_t)count * 4, hipMemcpyDeviceToHost, s)) !=
          hipSuccess)
    fail("download of the balanced accuracies", e);
  mark(4);
  if (rc == FS_OK && (e = hipStreamSynchronize(s)) != hipSuccess) fail("scan", e);
  if (s) (void)hipStreamSynchronize(s);
  if (rc == FS_OK)
    for (int i = 0; i < 4; i++) {
      float ms = -1.0f;
      if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) g_mdr_labels_ms[i] = ms;
    }
  for (hipEvent_t v : ev)
    if (v) (void)hipEventDestroy(v);
  if (s) (void)hipStreamDestroy(s);
  return rc;
}

}  // namespace gpu
}  // namespace fs
