// fs_pairtab.h -- the device side of one pair's contingency table, shared by
// k_mi_scan (fs_mi.hip), k_cfs_row (fs_cfs.hip) and k_mi_row (fs_mrmr.hip).
// All three read the bit-planes of k_mi_pack, planes[(w * P1p + c) * SP + s],
// give a pair NB^2 lanes (NB = SP / 4) and a lane one 4 x 4 block of the pair's
// table in 16 registers, and turn the table into a float64 sum of terms in the
// reference's operation order inside the same kernel.  Here, each once:
//
//   pt_count     the 4 x 4 popcount block of one word (all three kernels).
//   pt_epilogue  (the two row kernels) pxy into LDS [pair][SP][SP], the
//                marginals in index order, every cell's term on the lane that
//                counted it, and the row-major sum on the pair's first lane.
//   pt_row       the scan of one anchor column against a workgroup's columns,
//                then pt_epilogue over the transposed indices when the anchor
//                has the higher index (the column with the lower index
//                supplies the table's rows).
//   pt_block_best  the fixed-tree reduction of (value, index) over 256 lanes.
//
// What differs between the callers is a compile-time parameter: `Terms` gives
// pxy() and term() (MiTerms below; CfsTerms in fs_cfs.hip), kUsed says whether
// the used-state counts are taken (mi_constant needs them; CFS does not pay for
// them).  What a pair's first lane does with the sum stays in each kernel's
// own file.  k_mi_scan keeps its own staging (both sides of its tile come from
// LDS) and, on a measurement, its own copy of the epilogue without the
// transposition: see the note above that kernel.  fs_jmi.hip takes pt_row for
// its relevance, pt_count and pt_block_best for k_jmi_row and its step kernels;
// the three-way table's epilogue is that kernel's own.
#pragma once

#include "fs_gpu_internal.h"
#include "fs_mi.h"

namespace fs {
namespace gpu {

constexpr int kPtThreads = 256;
constexpr int kPtWC = 64;      // words (2048 samples) staged per chunk
constexpr int kPtPx = 4096;    // most cells of a workgroup's tables: pairs * SP^2
constexpr int kPtMarg = 1024;  // most marginals of a workgroup: pairs * SP

struct MiTerms {
  static __device__ __forceinline__ double pxy(int32_t count, double dn) {
    return mi_pxy(count, dn);
  }
  static __device__ __forceinline__ double term(double pxy, double p1, double p2) {
    return mi_term(pxy, p1, p2);
  }
};

// c[r * 4 + k] += popcount(A[r] & B[k]): one word of one 4 x 4 block
__device__ __forceinline__ void pt_count(const uint4 A, const uint4 B, uint32_t (&c)[16]) {
  c[0] += __builtin_popcount(A.x & B.x);
  c[1] += __builtin_popcount(A.x & B.y);
  c[2] += __builtin_popcount(A.x & B.z);
  c[3] += __builtin_popcount(A.x & B.w);
  c[4] += __builtin_popcount(A.y & B.x);
  c[5] += __builtin_popcount(A.y & B.y);
  c[6] += __builtin_popcount(A.y & B.z);
  c[7] += __builtin_popcount(A.y & B.w);
  c[8] += __builtin_popcount(A.z & B.x);
  c[9] += __builtin_popcount(A.z & B.y);
  c[10] += __builtin_popcount(A.z & B.z);
  c[11] += __builtin_popcount(A.z & B.w);
  c[12] += __builtin_popcount(A.w & B.x);
  c[13] += __builtin_popcount(A.w & B.y);
  c[14] += __builtin_popcount(A.w & B.z);
  c[15] += __builtin_popcount(A.w & B.w);
}

// A lane's place in its workgroup: pair q of the workgroup, block (ab, bb) of
// the pair's table.  lane_on: q is a pair of the workgroup at all (its cells
// of s_px are stored, as zeros if need be); pair_on: the pair is wanted.
struct PtLane {
  int q, ab, bb;
  bool lane_on, pair_on;
};

// What the pair's first lane is handed: the columns that supply the table's
// rows (lo) and columns (hi), the row-major sum of the terms over
// kcol[lo] x kcol[hi] and, with kUsed, each side's states with a non-zero
// marginal.
struct PtPair {
  int64_t lo, hi;
  double sum;
  int used1, used2;
};

// cnt[r * 4 + k] counts (state 4 ab + r of the first side, state 4 bb + k of
// the second).  With `swap` the second side supplies the table's rows.  Every
// lane of the workgroup calls this; true on the first lane of a wanted pair,
// with r filled.
template <class Terms, bool kUsed>
__device__ __forceinline__ bool pt_epilogue(const uint32_t (&cnt)[16], const PtLane g, bool swap,
                                            double dn, int SP, int npairs,
                                            const int32_t* __restrict__ kcol, double* s_px,
                                            double* s_p1, double* s_p2, PtPair& r) {
  const int tq = g.q * SP * SP;
  // the lane's block of the table: its first row and column, its first cell,
  // and what a step of a / of b moves in the table
  const int rb = 4 * (swap ? g.bb : g.ab), cb = 4 * (swap ? g.ab : g.bb);
  const int tb = tq + rb * SP + cb;
  const int da = swap ? 1 : SP, db = swap ? SP : 1;
  double px[16];
#pragma unroll
  for (int k = 0; k < 16; k++) px[k] = Terms::pxy((int32_t)cnt[k], dn);
  if (g.lane_on) {
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int b = 0; b < 4; b++) s_px[tb + a * da + b * db] = px[a * 4 + b];
  }
  __syncthreads();
  for (int it = threadIdx.x; it < npairs * SP; it += kPtThreads) {
    const int q2 = it / SP, s = it - q2 * SP;
    const double* t = s_px + q2 * SP * SP;
    double r1 = 0.0, r2 = 0.0;
    for (int b = 0; b < SP; b++) r1 += t[s * SP + b];
    for (int b = 0; b < SP; b++) r2 += t[b * SP + s];
    s_p1[it] = r1;
    s_p2[it] = r2;
  }
  __syncthreads();
  if (g.pair_on) {
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int b = 0; b < 4; b++)
        s_px[tb + a * da + b * db] =
            Terms::term(px[a * 4 + b], s_p1[g.q * SP + rb + (swap ? b : a)],
                        s_p2[g.q * SP + cb + (swap ? a : b)]);
  }
  __syncthreads();
  if (!(g.pair_on && g.ab == 0 && g.bb == 0)) return false;
  // a state count never exceeds SP on packed data; the bound keeps the loop
  // inside the table while a rejected call (a code >= n_states) drains
  const int k1 = kcol[r.lo] < SP ? kcol[r.lo] : SP, k2 = kcol[r.hi] < SP ? kcol[r.hi] : SP;
  const double* t = s_px + tq;
  double sum = 0.0;
  for (int a = 0; a < k1; a++)
    for (int b = 0; b < k2; b++) sum += t[a * SP + b];
  r.sum = sum;
  if (kUsed) {
    int used1 = 0, used2 = 0;
    for (int a = 0; a < k1; a++) used1 += s_p1[g.q * SP + a] > 0.0;
    for (int b = 0; b < k2; b++) used2 += s_p2[g.q * SP + b] > 0.0;
    r.used1 = used1, r.used2 = used2;
  }
  return true;
}

struct PtRowArgs {
  const uint32_t* planes;
  const int32_t* kcol;        // P1 state counts
  int64_t n, p, P1p, W;
  int SP, NB, CPW;            // CPW: columns per workgroup, kPtThreads / NB^2
  int64_t anchor;             // the anchor column (p: the target) ...
  const int64_t* anchor_dev;  // ... or where to read it (negative: nothing to do)
};

// One anchor column against the CPW columns of workgroup blockIdx.x.  The
// anchor's planes are staged in LDS per chunk of kPtWC words; a column's
// planes come straight from HBM, consecutive lanes reading consecutive 16-byte
// vectors of one word.  True on the first lane of a pair (anchor, c), c < p,
// with r filled; lo == hi is the anchor against itself.  The whole workgroup
// returns false when the anchor is negative.
template <class Terms, bool kUsed>
__device__ __forceinline__ bool pt_row(const PtRowArgs& a, int64_t& c, PtPair& r) {
  __shared__ __align__(16) uint32_t s_anc[kPtWC * kMiMaxStatesGpu];
  __shared__ double s_px[kPtPx];  // [pair][SP][SP]: pxy, then the terms
  __shared__ double s_p1[kPtMarg];
  __shared__ double s_p2[kPtMarg];
  const int tid = threadIdx.x;
  const int64_t anc = a.anchor_dev ? *a.anchor_dev : a.anchor;
  if (anc < 0) return false;
  const int SP = a.SP, NB = a.NB, CPW = a.CPW;
  const int L = NB * NB;  // lanes per pair
  PtLane g;
  g.q = tid / L;
  const int blk = tid - g.q * L;
  g.ab = blk / NB, g.bb = blk - g.ab * NB;  // the anchor's / the column's block of 4 states
  g.lane_on = g.q < CPW;
  c = (int64_t)blockIdx.x * CPW + (g.lane_on ? g.q : 0);  // < P1p
  g.pair_on = g.lane_on && c < a.p;

  uint32_t cnt[16];
#pragma unroll
  for (int k = 0; k < 16; k++) cnt[k] = 0;

  const uint4* g4 = reinterpret_cast<const uint4*>(a.planes);
  uint4* s4 = reinterpret_cast<uint4*>(s_anc);
  for (int64_t w0 = 0; w0 < a.W; w0 += kPtWC) {
    const int wn = a.W - w0 < kPtWC ? (int)(a.W - w0) : kPtWC;
    for (int v = tid; v < wn * NB; v += kPtThreads) {
      const int w = v / NB, xb = v - w * NB;
      s4[v] = g4[((size_t)(w0 + w) * a.P1p + anc) * NB + xb];
    }
    __syncthreads();
    if (g.pair_on) {
      const uint4* gc = g4 + ((size_t)w0 * a.P1p + c) * NB + g.bb;
      const size_t gstep = (size_t)a.P1p * NB;
      for (int w = 0; w < wn; w++) pt_count(s4[w * NB + g.ab], gc[(size_t)w * gstep], cnt);
    }
    __syncthreads();
  }

  const bool swap = anc > c;
  r.lo = swap ? c : anc, r.hi = swap ? anc : c;
  return pt_epilogue<Terms, kUsed>(cnt, g, swap, (double)a.n, SP, CPW, a.kcol, s_px, s_p1,
                                         s_p2, r);
}

// The best (value, index) of the workgroup's kPtThreads lanes by `Beats` in a
// fixed tree, to every lane.  sm / si: kPtThreads entries each.
template <bool (*Beats)(double, int64_t, double, int64_t)>
__device__ __forceinline__ void pt_block_best(double& m, int64_t& bi, double* sm, int64_t* si) {
  const int tid = threadIdx.x;
  sm[tid] = m;
  si[tid] = bi;
  __syncthreads();
  for (int s = kPtThreads / 2; s > 0; s >>= 1) {
    if (tid < s && Beats(sm[tid + s], si[tid + s], sm[tid], si[tid])) {
      sm[tid] = sm[tid + s];
      si[tid] = si[tid + s];
    }
    __syncthreads();
  }
  m = sm[0];
  bi = si[0];
}

}  // namespace gpu
}  // namespace fs
