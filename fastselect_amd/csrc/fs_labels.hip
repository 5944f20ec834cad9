// fs_labels.hip -- the MultiSURF permutation test on the GPU: the score sums
// of B labellings of the plan's samples on what fs_plan_select left on the
// device (the distance tiles, the thresholds, the pass-2 operands xs).
//
// Pass 1 and the select stage do not read the labels, so the near sets
// N_i = { j : D_ij < thr_i } hold for every labelling, and a near pair's weight
// is never zero (-1/H from a near side of a hit, +1/M from a near side of a
// miss): the sparse structure pass 2 walks is label-independent too.  Over B
// labellings
//
//   S[f, b] = sum over the weighted pairs (i < j) of diff_f(i, j) * W[(i, j), b]
//
// is a contraction over the pairs, with diff_f computed once and used B times.
// Three stages, all in this file:
//
//  1. records (once per call): k_lab_count / k_lab_scan / k_lab_fill walk the
//     tiles and emit every weighted pair as (i, j, near_i, near_j), the
//     decisions exactly as pair_weight (fs_pass2.hip) takes them, the diagonal
//     tiles as k_weights treats them (ii < jj).  A tile's records are padded
//     with zero-weight records to whole groups of kLabGroup = 256; Nn[i], the
//     size of N_i, is counted on the way.
//  2. counts (per chunk of at most 32 labellings): k_lab_counts adds a near
//     side of a hit to H[i][b] (integer atomics: exact in any order); M is
//     Nn - H.  k_lab_recip turns them into u = (-1/H, +1/M) per (sample,
//     labelling), in float64 as pair_weight divides.
//     k_lab_weights forms the weight of every record for every labelling of
//     the chunk, (float)(near_i u(i) + near_j u(j)), into W[record][32]
//     (DESIGN.md "MultiSURF permutation test" says why not inside the score
//     kernel: there the 32 weights of a record cost two gathered 1 KB rows of
//     labels and u per feature block, here one coalesced 128-byte read and
//     one VGPR a step).
//  3. score: k_lab_score.  One v_mfma_f32_32x32x2_f32 multiplies the diffs of
//     32 features x 2 records with the weights of 2 records x 32 labellings.
//     A wave holds 128 features (4 independent accumulators of 16 VGPRs);
//     after one group (128 MFMAs a block: 256 records) the float32
//     accumulators fold into float64 ones.  Groups are cut per tile, so the
//     float32 partials do not depend on how tiles are dealt to workgroups
//     (labels_seg_len) nor on the chunk (labels_chunk: a labelling is one
//     column of the B operand): those regroup float64 sums only.  No float
//     atomics; the segments' partials are added in segment order
//     (k_lab_reduce).
// Shared state and helpers: fs_gpu_internal.h.
#include "fs_gpu_internal.h"

namespace fs {
namespace gpu {

constexpr int kLabB = 32;        // labellings per chunk (the N of the MFMA)
constexpr int kLabGroup = 256;   // records per float32 fold (128 MFMAs of K = 2)
constexpr int kLabFeat = 128;    // features per wave (4 blocks of the MFMA's M = 32)
constexpr int kLabWaves = 4;     // waves per workgroup: 512 features on one record stream
// workgroups aimed at (k_lab_score; the labels_seg_len test hook sets the
// tiles per workgroup instead)
constexpr int64_t kLabWorkgroups = 2048;

typedef float lab_f16 __attribute__((ext_vector_type(16)));

// near flags of pair (i0 + ii, j0 + jj) of owned tile t: bit 0 = j in N_i,
// bit 1 = i in N_j; 0 for pairs outside the triangle.  The decisions of
// pair_weight: d < thr on the stored distance; SURF: on its float32 value
// (what the integer route stores already, and what the float64 route rounds to).
template <bool SURF>
__device__ __forceinline__ uint32_t lab_flags(const double* __restrict__ D, int64_t n,
                                              int64_t n_pad, int tiled, int2 win, int64_t t,
                                              int2 tl, int ii, int jj,
                                              const double* __restrict__ thr) {
  const int64_t i0 = (int64_t)tl.x * kTile, j0 = (int64_t)tl.y * kTile;
  const int64_t i = i0 + ii, j = j0 + jj;
  if (!(i < n && j < n && (tl.x < tl.y || ii < jj))) return 0u;
  double d = D[d_rd(tiled, win, n_pad, t, i0, j0, ii, jj)];  // == D[i][j]
  if (SURF) d = (double)(float)d;
  return (d < thr[i] ? 1u : 0u) | (d < thr[j] ? 2u : 0u);
}

// Weighted pairs per wave quarter of every tile: wave w of the workgroup
// walks elements e = jj * 128 + ii in [w * 4096, (w + 1) * 4096), 64
// consecutive ii at a time.  wcnt[t * 4 + w].
template <bool SURF>
__global__ __launch_bounds__(256) void k_lab_count(const double* __restrict__ D, int64_t n,
                                                   int64_t n_pad, int tiled, int2 win,
                                                   const int2* __restrict__ tiles,
                                                   const double* __restrict__ thr,
                                                   uint32_t* __restrict__ wcnt) {
  const int64_t t = blockIdx.x;
  const int2 tl = tiles[t];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t c = 0;
  for (int it = 0; it < 64; it++) {
    const int e = wave * 4096 + it * 64 + lane;
    const uint32_t fl = lab_flags<SURF>(D, n, n_pad, tiled, win, t, tl, e % kTile, e / kTile, thr);
    c += (uint32_t)__popcll(__ballot(fl != 0u));
  }
  if (lane == 0) wcnt[t * 4 + wave] = c;
}

// goff[t] = groups before tile t, goff[n_tiles] = all groups: an exclusive
// scan of ceil(count_t / kLabGroup) by one workgroup.
__global__ __launch_bounds__(256) void k_lab_scan(const uint32_t* __restrict__ wcnt,
                                                  int64_t n_tiles, int64_t* __restrict__ goff) {
  __shared__ int64_t part[256];
  const int tid = threadIdx.x;
  const int64_t per = (n_tiles + 255) / 256;
  const int64_t lo = tid * per < n_tiles ? tid * per : n_tiles;
  const int64_t hi = lo + per < n_tiles ? lo + per : n_tiles;
  int64_t s = 0;
  for (int64_t t = lo; t < hi; t++) {
    const int64_t c = (int64_t)wcnt[4 * t] + wcnt[4 * t + 1] + wcnt[4 * t + 2] + wcnt[4 * t + 3];
    s += (c + kLabGroup - 1) / kLabGroup;
  }
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    int64_t run = 0;
    for (int k = 0; k < 256; k++) {
      const int64_t v = part[k];
      part[k] = run;
      run += v;
    }
    goff[n_tiles] = run;
  }
  __syncthreads();
  int64_t run = part[tid];
  for (int64_t t = lo; t < hi; t++) {
    goff[t] = run;
    const int64_t c = (int64_t)wcnt[4 * t] + wcnt[4 * t + 1] + wcnt[4 * t + 2] + wcnt[4 * t + 3];
    run += (c + kLabGroup - 1) / kLabGroup;
  }
}

// The records of every tile in element order (rec zeroed by the caller: the
// padding of a tile's last group is (0, 0, no flags)), and Nn[i] += the near
// sides of sample i.  rec[r] = (i, j | flags << 30).
template <bool SURF>
__global__ __launch_bounds__(256) void k_lab_fill(const double* __restrict__ D, int64_t n,
                                                  int64_t n_pad, int tiled, int2 win,
                                                  const int2* __restrict__ tiles,
                                                  const double* __restrict__ thr,
                                                  const uint32_t* __restrict__ wcnt,
                                                  const int64_t* __restrict__ goff,
                                                  int2* __restrict__ rec,
                                                  uint32_t* __restrict__ Nn) {
  const int64_t t = blockIdx.x;
  const int2 tl = tiles[t];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t pos = goff[t] * kLabGroup;
  for (int w = 0; w < wave; w++) pos += wcnt[t * 4 + w];
  const int64_t end = goff[t + 1] * kLabGroup;  // never reached: the counts are k_lab_count's
  for (int it = 0; it < 64; it++) {
    const int e = wave * 4096 + it * 64 + lane;
    const int ii = e % kTile, jj = e / kTile;
    const uint32_t fl = lab_flags<SURF>(D, n, n_pad, tiled, win, t, tl, ii, jj, thr);
    const uint64_t m = __ballot(fl != 0u);
    if (fl != 0u) {
      const int64_t r = pos + __popcll(m & ((1ull << lane) - 1ull));
      const int32_t i = tl.x * kTile + ii, j = tl.y * kTile + jj;
      if (r < end) rec[r] = make_int2(i, (int32_t)((uint32_t)j | (fl << 30)));
      if (fl & 1u) atomicAdd(&Nn[i], 1u);
    }
    // the 64 lanes share jj: one add for sample j
    const uint32_t cj = (uint32_t)__popcll(__ballot((fl & 2u) != 0u));
    if (lane == 0 && cj != 0u) atomicAdd(&Nn[tl.y * kTile + jj], cj);
    pos += __popcll(m);
  }
}

// labT[i * 32 + b] = labels of labelling b0 + b (lab_raw[b][n], nb rows);
// columns b >= nb are never read as labels of a weight (their u is 0).
__global__ __launch_bounds__(256) void k_lab_transpose(const int32_t* __restrict__ lab_raw,
                                                       int64_t n, int nb,
                                                       int32_t* __restrict__ labT) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t i = g / kLabB;
  const int b = (int)(g % kLabB);
  if (i >= n) return;
  labT[g] = b < nb ? lab_raw[(int64_t)b * n + i] : 0;
}

// H[i * 32 + b] += 1 per near side of sample i whose pair is a hit under
// labelling b (zeroed by the caller).  Thread (record, b).
__global__ __launch_bounds__(256) void k_lab_counts(const int2* __restrict__ rec, int64_t nrec,
                                                    const int32_t* __restrict__ labT, int nb,
                                                    uint32_t* __restrict__ H) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r = g / kLabB;
  const int b = (int)(g % kLabB);
  if (r >= nrec || b >= nb) return;
  const int2 rc = rec[r];
  const uint32_t fl = (uint32_t)rc.y >> 30;
  if (fl == 0u) return;
  const int64_t i = rc.x, j = rc.y & 0x3fffffff;
  if (labT[i * kLabB + b] != labT[j * kLabB + b]) return;
  if (fl & 1u) atomicAdd(&H[i * kLabB + b], 1u);
  if (fl & 2u) atomicAdd(&H[j * kLabB + b], 1u);
}

// U[i * 32 + b] = (-1 / H, +1 / M), M = Nn - H, 0 where the count is 0 (no
// near pair of that kind reads it) and for the padding labellings b >= nb.
__global__ __launch_bounds__(256) void k_lab_recip(const uint32_t* __restrict__ H,
                                                   const uint32_t* __restrict__ Nn, int64_t n,
                                                   int nb, double2* __restrict__ U) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t i = g / kLabB;
  const int b = (int)(g % kLabB);
  if (i >= n) return;
  double2 u = make_double2(0.0, 0.0);
  if (b < nb) {
    const uint32_t h = H[g], m = Nn[i] - h;
    if (h) u.x = multisurf_weight(true, true, 0, (double)h, (double)m);
    if (m) u.y = multisurf_weight(true, false, 0, (double)h, (double)m);
  }
  U[g] = u;
}

// W[r * 32 + b] = the weight of record r under labelling b of the chunk:
// (float)(near_i u(i) + near_j u(j)), the float64 sum rounded once as
// pair_weight rounds it; 0 for padding records and padding labellings (their
// u is 0).  Thread (record, b).
__global__ __launch_bounds__(256) void k_lab_weights(const int2* __restrict__ rec, int64_t nrec,
                                                     const int32_t* __restrict__ labT,
                                                     const double2* __restrict__ U,
                                                     float* __restrict__ W) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r = g / kLabB;
  const int b = (int)(g % kLabB);
  if (r >= nrec) return;
  const int2 rc = rec[r];
  const uint32_t fl = (uint32_t)rc.y >> 30;
  float w = 0.0f;
  if (fl != 0u) {
    const int64_t i = rc.x, j = rc.y & 0x3fffffff;
    const bool hit = labT[i * kLabB + b] == labT[j * kLabB + b];
    const double2 ui = U[i * kLabB + b], uj = U[j * kLabB + b];
    const double wi = (fl & 1u) ? (hit ? ui.x : ui.y) : 0.0;
    const double wj = (fl & 2u) ? (hit ? uj.x : uj.y) : 0.0;
    w = (float)(wi + wj);
  }
  W[g] = w;
}

// MODE 0: the wave's 128 features are continuous, 1: discrete, 2: the first
// 64 continuous and the last 64 discrete (PC is a multiple of 64).
template <int MODE>
__device__ __forceinline__ float lab_diff(float a, float b, bool disc) {
  const float c = __builtin_fabsf(a - b), d = a != b ? 1.0f : 0.0f;
  if (MODE == 0) return c;
  if (MODE == 1) return d;
  return disc ? d : c;
}

// One step's operands in flight: the two sample rows' 4 features and the
// weight (9 VGPRs).
struct LabSlot {
  float4 a, b;
  float w;
};
// steps in flight per wave (divides 32).  16 slots do not fit beside the 128
// VGPRs of float64 sums (spills); with the sums in LDS they fit, and measured
// no faster (cfg2: 104 ms against 92 ms): past 8 the gathers' bandwidth, not
// their latency, is the limit
constexpr int kLabRing = 8;
constexpr int kLabBlock = 64;  // records per register block (one per lane)

// Request step `step` (0..31) of record block blk, whose records the wave
// holds one per lane in R: lane l = 32 k + m takes record 2 step + k.
__device__ __forceinline__ void lab_issue(LabSlot& sl, const float* __restrict__ xs, int64_t PW,
                                          int64_t c, const float* __restrict__ W, int2 R,
                                          int64_t blk, int step, int k, int m) {
  const int src = (2 * step + k) << 2;
  const int64_t i = __builtin_amdgcn_ds_bpermute(src, R.x);
  const int64_t j = __builtin_amdgcn_ds_bpermute(src, R.y) & 0x3fffffff;
  sl.a = *(const float4*)(xs + i * PW + c);
  sl.b = *(const float4*)(xs + j * PW + c);
  sl.w = W[(blk * kLabBlock + 2 * step + k) * kLabB + m];
}

// Groups [g_begin, g_end) of the record list for the wave's 128 features.
// Lane l = 32 k + m: in the A operand record k of the step's two, feature row
// m of each of the 4 blocks (feature c + q for block q, c = c0 + 4 m: one
// 16-byte load per sample row); in the B operand record k, labelling m.
// The records come 64 at a time, one per lane (blocks of kLabBlock; a group
// is 4 blocks), two blocks ahead of their use; a step's row gathers and its
// weight are requested kLabRing steps (2048 MFMA cycles) before the step's
// MFMAs, into a ring of register slots: at one wave per SIMD that distance,
// not occupancy, is what covers the gathers' latency.  The requests run past
// the last block into a repeat of it, whose operands are dropped.
template <int MODE>
__device__ __forceinline__ void lab_groups(const float* __restrict__ xs, int64_t PW, int64_t c,
                                           bool disc, const int2* __restrict__ rec,
                                           const float* __restrict__ W, int64_t g_begin,
                                           int64_t g_end, int lane, double (&s)[64]) {
  const int k = lane >> 5, m = lane & 31;
  const int64_t q_begin = g_begin * 4, q_last = g_end * 4 - 1;
  if (q_begin > q_last) return;
  lab_f16 acc[4];
#pragma unroll
  for (int q = 0; q < 4; q++)
#pragma unroll
    for (int v = 0; v < 16; v++) acc[q][v] = 0.0f;
  int2 rlo = rec[q_begin * kLabBlock + lane];
  int64_t qn = q_begin + 1 < q_last ? q_begin + 1 : q_last;  // the block rhi holds
  int2 rhi = rec[qn * kLabBlock + lane];
  LabSlot ring[kLabRing];
#pragma unroll
  for (int st = 0; st < kLabRing; st++) lab_issue(ring[st], xs, PW, c, W, rlo, q_begin, st, k, m);
  for (int64_t q = q_begin; q <= q_last; q++) {
    const int64_t qp = q + 2 < q_last ? q + 2 : q_last;
    const int2 rpre = rec[qp * kLabBlock + lane];
#pragma unroll
    for (int st = 0; st < 32; st++) {
      LabSlot& sl = ring[st % kLabRing];
      const float w = sl.w;
      const float d0 = lab_diff<MODE>(sl.a.x, sl.b.x, disc), d1 = lab_diff<MODE>(sl.a.y, sl.b.y, disc);
      const float d2 = lab_diff<MODE>(sl.a.z, sl.b.z, disc), d3 = lab_diff<MODE>(sl.a.w, sl.b.w, disc);
      if (st < 32 - kLabRing) lab_issue(sl, xs, PW, c, W, rlo, q, st + kLabRing, k, m);
      else lab_issue(sl, xs, PW, c, W, rhi, qn, st + kLabRing - 32, k, m);
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(d0, w, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(d1, w, acc[1], 0, 0, 0);
      acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(d2, w, acc[2], 0, 0, 0);
      acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(d3, w, acc[3], 0, 0, 0);
      // a step's requests stay with its MFMAs: left to itself the scheduler
      // sinks them behind a turn's MFMAs and the ring drains every turn
      __builtin_amdgcn_sched_barrier(0);
    }
    if ((q & 3) == 3) {  // a group's 256 records: fold
#pragma unroll
      for (int qq = 0; qq < 4; qq++)
#pragma unroll
        for (int v = 0; v < 16; v++) {
          s[qq * 16 + v] += (double)acc[qq][v];
          acc[qq][v] = 0.0f;
        }
    }
    rlo = rhi;
    rhi = rpre;
    qn = qp;
  }
}

// Row of the 32 x 32 result that accumulator register v of lane l holds (its
// column is l % 32): v_mfma_f32_32x32x2_f32's output layout.
__device__ __forceinline__ int lab_acc_row(int v, int lane) {
  return 8 * (v / 4) + 4 * (lane / 32) + (v % 4);
}

// part[(b * nseg + seg) * PW + c]: labelling b of the chunk, segment seg
// (seg_len consecutive tiles), permuted column c.  Grid as k_stir_score's
// (XCD-aware: the feature blocks of a segment share an XCD's L2 for the
// record stream); wave w of a workgroup takes features fb * 512 + w * 128.
__global__ __launch_bounds__(64 * kLabWaves) void k_lab_score(
    const float* __restrict__ xs, int64_t PW, int64_t PC, const int2* __restrict__ rec,
    const int64_t* __restrict__ goff, const float* __restrict__ W, int64_t n_tiles,
    int64_t seg_len, int64_t nseg, int64_t nfb, int nb, double* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t w = blockIdx.x;
  const int64_t xcd = w % kXcds, kk = w / kXcds;
  const int64_t seg = xcd + kXcds * (kk / nfb), fb = kk % nfb;
  if (seg >= nseg) return;
  const int64_t f0 = fb * (kLabFeat * kLabWaves) + (int64_t)wave * kLabFeat;
  if (f0 >= PW) return;
  const int m = lane & 31;
  const int64_t c = f0 + 4 * m;
  // PW is a multiple of 64: the 4 features of a lane go together.  A lane
  // past PW reads column 0 instead; its sums are not written below
  const int64_t cl = c < PW ? c : 0;
  const bool disc = c >= PC;
  const int64_t t_begin = seg * seg_len;
  const int64_t t_end = t_begin + seg_len < n_tiles ? t_begin + seg_len : n_tiles;
  const int64_t g_begin = goff[t_begin], g_end = goff[t_end];
  double s[64];
#pragma unroll
  for (int q = 0; q < 64; q++) s[q] = 0.0;
  const bool d0 = f0 >= PC, d1 = f0 + 64 >= PC;
  if (!d1) lab_groups<0>(xs, PW, cl, disc, rec, W, g_begin, g_end, lane, s);
  else if (d0) lab_groups<1>(xs, PW, cl, disc, rec, W, g_begin, g_end, lane, s);
  else lab_groups<2>(xs, PW, cl, disc, rec, W, g_begin, g_end, lane, s);
  // lane l holds labelling l % 32 of rows lab_acc_row(v, l) of the 4 blocks
  if (m >= nb) return;
  double* __restrict__ out = part + ((int64_t)m * nseg + seg) * PW + f0;
#pragma unroll
  for (int q = 0; q < 4; q++)
#pragma unroll
    for (int v = 0; v < 16; v++) {
      const int64_t col = 4 * lab_acc_row(v, lane) + q;
      if (f0 + col < PW) out[col] = s[q * 16 + v];
    }
}

// scores[b * n_kept + out_pos[c]] = the sum of part[b][0..nseg)[c] in segment
// order.
__global__ __launch_bounds__(256) void k_lab_reduce(const double* __restrict__ part, int64_t nseg,
                                                    int64_t PW, const int64_t* __restrict__ out_pos,
                                                    int64_t n_kept, double* __restrict__ scores) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t b = blockIdx.y;
  if (c >= PW) return;
  const int64_t o = out_pos[c];
  if (o < 0) return;
  const double* __restrict__ p = part + b * nseg * PW + c;
  double s = 0.0;
  for (int64_t g = 0; g < nseg; g++) s += p[g * PW];
  scores[b * n_kept + o] = s;
}

int lab_transpose(Plan* g, const int32_t* lab_raw, int nb, int32_t* labT) {
  const int64_t n = g->P.n;
  k_lab_transpose<<<(unsigned)((n * kLabB + 255) / 256), 256, 0, g->stream>>>(lab_raw, n, nb, labT);
  return launch_check("k_lab_transpose");
}

void lab_score_split(const Plan* g, int64_t n_tiles, int64_t* seg_len, int64_t* nseg) {
  const int64_t nfb = (g->P.PW + kLabFeat * kLabWaves - 1) / (kLabFeat * kLabWaves);
  *seg_len = std::max<int64_t>(1, (n_tiles * nfb + kLabWorkgroups - 1) / kLabWorkgroups);
  if (test_hooks().labels_seg_len >= 1) *seg_len = test_hooks().labels_seg_len;
  *nseg = (n_tiles + *seg_len - 1) / *seg_len;
}

int lab_score_reduce(Plan* g, const int2* rec, const int64_t* goff, const float* W,
                     int64_t n_tiles, int64_t seg_len, int64_t nseg, int nb, double* part,
                     double* scores, hipEvent_t scored) {
  const Prepared& Q = g->P;
  const int64_t nfb = (Q.PW + kLabFeat * kLabWaves - 1) / (kLabFeat * kLabWaves);
  const int64_t seg_per_xcd = (nseg + kXcds - 1) / kXcds;
  k_lab_score<<<(unsigned)(kXcds * seg_per_xcd * nfb), 64 * kLabWaves, 0, g->stream>>>(
      g->xs, Q.PW, Q.PC, rec, goff, W, n_tiles, seg_len, nseg, nfb, nb, part);
  FS_TRY(launch_check("k_lab_score"));
  if (scored) FS_HIP(hipEventRecord(scored, g->stream));
  k_lab_reduce<<<dim3((unsigned)((Q.PW + 255) / 256), (unsigned)nb), 256, 0, g->stream>>>(
      part, nseg, Q.PW, g->out_pos, Q.n_kept, scores);
  return launch_check("k_lab_reduce");
}

// The record stage of one call (buffers in g->mem_call): the weighted pairs
// of every owned tile into rec (nrec records, whole groups per tile: goff),
// Nn[i] = |N_i|, wcnt the counts per wave quarter.  surf: SURF's decisions.
// One host synchronisation (the record count).
int lab_records(Plan* g, bool surf, uint32_t** wcnt_out, int64_t** goff_out, uint32_t** Nn_out,
                int2** rec_out, int64_t* nrec_out) {
  const Prepared& Q = g->P;
  const int64_t n = Q.n;
  hipStream_t st = g->stream;
  uint32_t *wcnt = nullptr, *Nn = nullptr;
  int64_t* goff = nullptr;
  FS_TRY(g->mem_call.alloc(&wcnt, (size_t)4 * g->n_tiles));
  FS_TRY(g->mem_call.alloc(&goff, (size_t)g->n_tiles + 1));
  FS_TRY(g->mem_call.alloc(&Nn, (size_t)n));
  if (surf)
    k_lab_count<true><<<(unsigned)g->n_tiles, 256, 0, st>>>(g->D, n, Q.n_pad, g->tiled, g->win,
                                                            g->tiles, g->thr, wcnt);
  else
    k_lab_count<false><<<(unsigned)g->n_tiles, 256, 0, st>>>(g->D, n, Q.n_pad, g->tiled, g->win,
                                                             g->tiles, g->thr, wcnt);
  FS_TRY(launch_check("k_lab_count"));
  k_lab_scan<<<1, 256, 0, st>>>(wcnt, g->n_tiles, goff);
  FS_TRY(launch_check("k_lab_scan"));
  int64_t ngroups = 0;
  FS_HIP(hipMemcpyAsync(&ngroups, goff + g->n_tiles, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  FS_HIP(hipStreamSynchronize(st));
  const int64_t nrec = ngroups * kLabGroup;
  int2* rec = nullptr;
  FS_TRY(g->mem_call.alloc(&rec, (size_t)nrec));
  FS_HIP(hipMemsetAsync(rec, 0, sizeof(int2) * (size_t)nrec, st));
  FS_HIP(hipMemsetAsync(Nn, 0, sizeof(uint32_t) * (size_t)n, st));
  if (surf)
    k_lab_fill<true><<<(unsigned)g->n_tiles, 256, 0, st>>>(g->D, n, Q.n_pad, g->tiled, g->win,
                                                           g->tiles, g->thr, wcnt, goff, rec, Nn);
  else
    k_lab_fill<false><<<(unsigned)g->n_tiles, 256, 0, st>>>(g->D, n, Q.n_pad, g->tiled, g->win,
                                                            g->tiles, g->thr, wcnt, goff, rec, Nn);
  FS_TRY(launch_check("k_lab_fill"));
  *wcnt_out = wcnt, *goff_out = goff, *Nn_out = Nn, *rec_out = rec, *nrec_out = nrec;
  return FS_OK;
}

static int labels_events(Plan* g, size_t count) {
  while (g->ev_labels.size() < count) {
    hipEvent_t e = event_get(g->device, true);
    if (!e) return FS_EHIP;
    g->ev_labels.push_back(e);
  }
  return FS_OK;
}

int plan_score_labels(Plan* g, const int32_t* labels, int64_t B, double* scores) {
  const Prepared& Q = g->P;
  const int64_t n = Q.n;
  FS_HIP(hipSetDevice(g->device));
  // the previous call's buffers (a plan_stir on a caller's stream keeps its own)
  if (!g->mem_call.blocks.empty()) {
    FS_HIP(hipStreamSynchronize(g->stream));
    g->mem_call.release();
  }
  g->labels_chunks = -1;
  if (B <= 0) return FS_OK;
  if (g->n_tiles <= 0 || n >= (1 << 30)) {
    set_error("fs_plan_score_labels: the plan owns no tiles, or n >= 2^30");
    return FS_ENOTSUP;
  }
  int64_t chunk = kLabB;
  if (test_hooks().labels_chunk >= 1) chunk = std::min<int64_t>(kLabB, test_hooks().labels_chunk);
  const int64_t nchunks = (B + chunk - 1) / chunk;
  FS_TRY(labels_events(g, (size_t)(2 + 4 * nchunks)));
  hipStream_t st = g->stream;
  // ---- records, once per call
  uint32_t *wcnt = nullptr, *Nn = nullptr, *H = nullptr;
  int64_t* goff = nullptr;
  int2* rec = nullptr;
  int64_t nrec = 0;
  FS_HIP(hipEventRecord(g->ev_labels[0], st));
  FS_TRY(lab_records(g, false, &wcnt, &goff, &Nn, &rec, &nrec));
  FS_HIP(hipEventRecord(g->ev_labels[1], st));
  // ---- the split of the score kernel: whole tiles per workgroup
  int64_t seg_len = 1, nseg = 1;
  lab_score_split(g, g->n_tiles, &seg_len, &nseg);
  // ---- a chunk's buffers: sized by n, PW and the split, not by B
  int32_t *lab_raw = nullptr, *labT = nullptr;
  double2* U = nullptr;
  float* W = nullptr;
  double* part = nullptr;
  FS_TRY(g->mem_call.alloc(&lab_raw, (size_t)chunk * n));
  FS_TRY(g->mem_call.alloc(&labT, (size_t)kLabB * n));
  FS_TRY(g->mem_call.alloc(&H, (size_t)kLabB * n));
  FS_TRY(g->mem_call.alloc(&U, (size_t)kLabB * n));
  FS_TRY(g->mem_call.alloc(&W, (size_t)nrec * kLabB));
  FS_TRY(g->mem_call.alloc(&part, (size_t)chunk * nseg * Q.PW));
  const unsigned grid_nb = (unsigned)((n * kLabB + 255) / 256);
  for (int64_t c = 0; c < nchunks; c++) {
    const int64_t b0 = c * chunk;
    const int nb = (int)std::min(chunk, B - b0);
    hipEvent_t* ev = g->ev_labels.data() + 2 + 4 * c;
    FS_HIP(hipMemcpyAsync(lab_raw, labels + b0 * n, sizeof(int32_t) * (size_t)nb * n,
                          hipMemcpyHostToDevice, st));
    FS_HIP(hipMemsetAsync(H, 0, sizeof(uint32_t) * (size_t)kLabB * n, st));
    FS_HIP(hipEventRecord(ev[0], st));
    k_lab_transpose<<<grid_nb, 256, 0, st>>>(lab_raw, n, nb, labT);
    FS_TRY(launch_check("k_lab_transpose"));
    if (nrec > 0) {
      k_lab_counts<<<(unsigned)((nrec * kLabB + 255) / 256), 256, 0, st>>>(rec, nrec, labT, nb, H);
      FS_TRY(launch_check("k_lab_counts"));
    }
    k_lab_recip<<<grid_nb, 256, 0, st>>>(H, Nn, n, nb, U);
    FS_TRY(launch_check("k_lab_recip"));
    if (nrec > 0) {
      k_lab_weights<<<(unsigned)((nrec * kLabB + 255) / 256), 256, 0, st>>>(rec, nrec, labT, U, W);
      FS_TRY(launch_check("k_lab_weights"));
    }
    FS_HIP(hipEventRecord(ev[1], st));
    FS_HIP(hipEventRecord(ev[2], st));
    FS_TRY(lab_score_reduce(g, rec, goff, W, g->n_tiles, seg_len, nseg, nb, part,
                            scores + b0 * Q.n_kept, ev[3]));
    g->labels_chunks = (int)(c + 1);
  }
  // the labels are host memory: the call ends when the device has finished
  FS_HIP(hipStreamSynchronize(st));
  g->mem_call.release();
  return FS_OK;
}

// Summed HIP-event time of the last plan_score_labels: which == 0 the record
// kernels, 1 the counts, reciprocal and weights kernels, 2 the score kernel
// (1 and 2 over its chunks), in milliseconds; -1 when unavailable.
double plan_labels_kernel_ms(const Plan* g, int which) {
  if (g->labels_chunks < 0 || which < 0 || which > 2) return -1.0;
  auto span = [&](size_t a, size_t b) -> double {
    float ms = -1.0f;
    if (hipEventSynchronize(g->ev_labels[b]) != hipSuccess ||
        hipEventElapsedTime(&ms, g->ev_labels[a], g->ev_labels[b]) != hipSuccess) {
      (void)hipGetLastError();
      return -1.0;
    }
    return (double)ms;
  };
  if (which == 0) return span(0, 1);
  double total = 0.0;
  for (int c = 0; c < g->labels_chunks; c++) {
    const size_t a = 2 + 4 * (size_t)c + 2 * (size_t)(which - 1);
    const double ms = span(a, a + 1);
    if (ms < 0.0) return -1.0;
    total += ms;
  }
  return total;
}

int multisurf_labels_run(const Prepared& P, const void* x, int device, const int32_t* labels,
                         int64_t B, float* scores_out) {
  if (multisurf_shards(P, device, 1) > 1) {
    set_error("fs_multisurf_score_labels: the distance tiles do not fit the device (a sharded "
              "plan cannot score labellings)");
    return FS_ENOTSUP;
  }
  Plan* g = nullptr;
  Prepared Q = P;
  Q.defer_guard = 1;  // decided beside the first pass 1 (row_guard), as multisurf_run
  FS_TRY(plan_create(&g, Q, x, 0, device, 0, 1, 0));
  double *rs = nullptr, *cnt = nullptr, *sc = nullptr, *out = nullptr;
  int rc, switched = 0;
  double risk = -1.0;
  auto step = [&]() -> int {
    FS_TRY(plan_pass1(g, rs));
    FS_TRY(plan_select(g, rs, cnt));
    return plan_pass2(g, cnt, sc);
  };
  std::vector<double> host((size_t)B * P.n_kept);
  if ((rc = g->mem_plan.alloc(&rs, 3 * P.n)) || (rc = g->mem_plan.alloc(&cnt, 2 * P.n)) ||
      (rc = g->mem_plan.alloc(&sc, P.n_kept)) ||
      (rc = g->mem_plan.alloc(&out, (size_t)B * P.n_kept)) || (rc = step()) ||
      (rc = plan_decision_guard(g, rs, cnt, sc, &risk, &switched)) ||
      (switched && (rc = step())) || (rc = plan_score_labels(g, labels, B, out))) {
    plan_destroy(g);
    return rc;
  }
  if (hipMemcpy(host.data(), out, sizeof(double) * host.size(), hipMemcpyDeviceToHost) !=
      hipSuccess) {
    (void)hipGetLastError();
    plan_destroy(g);
    set_error("fs_multisurf_score_labels: copying the scores to the host failed");
    return FS_EHIP;
  }
  plan_destroy(g);
  for (size_t k = 0; k < host.size(); k++) scores_out[k] = (float)(host[k] / (double)P.n);
  return FS_OK;
}

}  // namespace gpu
}  // namespace fs
