// fs_stir.hip -- the STIR sums on the GPU (definitions: fs_stir.h): per
// feature the sum of diff and of diff^2 over the near-hit pairs and over the
// near-miss pairs of the plan's owned tiles.  One extra pass over what
// fs_plan_select left on the device: the distance tiles, the thresholds, the
// labels and the pass-2 operands xs.  Pass 2's own buffers (Wt, wrow, spart,
// its schedule) are not touched.
// Shared state and helpers: fs_gpu_internal.h.
#include "fs_gpu_internal.h"
#include "fs_stir.h"

namespace fs {
namespace gpu {

// ---------------------------------------------------------------------------
// Pair multiplicities of a chunk of owned tiles
// ---------------------------------------------------------------------------
// For pair (i, j), i < j, of a tile: m = [j in N_i] + [i in N_j], each side
// counted only when its focal sample lies in [r_lo, r_hi) -- the decisions and
// the row range exactly as pair_weight (fs_pass2.hip) takes them: d < thr[i]
// on the stored distance.  The pair is a hit or a miss for both sides, so it
// carries (m, 0) or (0, m) as (hit, miss) multiplicity, 0 / 1 / 2 as integers.
// Layout, the order k_stir_score's waves read it in: W[tile][jj][wave][q][r],
// q = 0 hit / 1 miss, row ii = wave * kStirRows + r: the 2 x 16 weights of one
// wave and one column are 128 contiguous bytes.
constexpr int kStirRows = 16;                     // rows of a tile per wave
constexpr int kStirWaves = kTile / kStirRows;     // 8 waves per workgroup
constexpr int kStirColW = 2 * kTile;              // words of a tile column
constexpr int kStirTileW = kStirColW * kTile;     // words of a tile (128 KB)
constexpr int kStirFold = 8;                      // columns per 32-bit partial

__global__ __launch_bounds__(256) void k_stir_weights(
    const double* __restrict__ D, int64_t n, int64_t n_pad, int tiled, int2 win,
    const int2* __restrict__ tiles, int64_t t0, const double* __restrict__ thr,
    const int32_t* __restrict__ lab, int64_t r_lo, int64_t r_hi, uint32_t* __restrict__ W) {
  const int64_t t = t0 + blockIdx.x;  // owned tile; blockIdx.x: its slot in the chunk
  const int2 tl = tiles[t];
  const int64_t i0 = (int64_t)tl.x * kTile, j0 = (int64_t)tl.y * kTile;
  uint32_t* out = W + (int64_t)blockIdx.x * kStirTileW;
  for (int e = threadIdx.x; e < kTile * kTile; e += 256) {
    const int jj = e / kTile, ii = e % kTile;
    const int64_t i = i0 + ii, j = j0 + jj;
    uint32_t wh = 0, wm = 0;
    if (i < n && j < n && (tl.x < tl.y || ii < jj)) {
      const double d = D[d_rd(tiled, win, n_pad, t, i0, j0, ii, jj)];  // == D[i][j]
      uint32_t m = 0;
      if (d < thr[i] && i >= r_lo && i < r_hi) m++;
      if (d < thr[j] && j >= r_lo && j < r_hi) m++;
      if (lab[i] == lab[j]) wh = m;
      else wm = m;
    }
    uint32_t* o = out + jj * kStirColW + (ii / kStirRows) * (2 * kStirRows) + (ii % kStirRows);
    o[0] = wh;
    o[kStirRows] = wm;
  }
}

// ---------------------------------------------------------------------------
// The four sums per feature over a chunk's tiles
// ---------------------------------------------------------------------------
// The dense walk of k_score (fs_pass2.hip) with two weights per pair and four
// accumulators per feature.  Grid as k_score (XCD-aware: feature blocks of
// 128, segments of seg_len consecutive tiles); 8 waves per workgroup, wave w
// holds rows w * 16 .. w * 16 + 15 of the segment's row block in VGPRs, lane l
// scores the features c0 = blk * 128 + l and c1 = c0 + 64 (each half wholly
// continuous or wholly discrete, PC being a multiple of 64).  Per column the
// wave's 2 x 16 multiplicities are wave-uniform and come by scalar loads, the
// next column's requested while this one's are consumed; the B values run two
// columns ahead.
//
// The sums are exact integer sums of fixed-point terms, not float32 partials.
// fs_plan_set_rows cuts through a pair (one side in the range, the other
// not), so a float32 partial of a row range and that of its complement do not
// add up to the whole range's beyond ~1e-8, where the stage promises 1e-12.
// A term's fixed-point value costs one instruction: for 0 <= d < K, K a
// power of two with an even biased exponent, the float d + K lies in
// [K, 2K), so its low 24 bits are d in units of K 2^-23, rounded to nearest
// (the exponent's lowest bit, bit 23, is zero); v_mad_u32_u24 reads exactly
// those 24 bits.  So per pair-feature, continuous: d = a - b, |d| + K1,
// fma(d, d, K2) (the square, rounded once, on its own grid) and four
// v_mad_u32_u24 (7 VALU); discrete: [a != b] and two (4 VALU; diff^2 == diff,
// so the squares' sums are copies).  A 32-bit partial holds 16 rows x 8
// columns = 128 terms below 2^24 with multiplicities up to 2 (< 2^32), then
// folds into a float64, which adds integers exactly up to 2^53.  Every
// partial sum of the stage is therefore exact, and shards, chunks, ranks and
// row ranges add up bit for bit; the scale K 2^-23 is applied once, to the
// workgroup's sum.  The grid step K 2^-23 (2.4e-7 of a feature's range at
// K = 2) is the rounding of the float32 operands themselves.  No atomics:
// the 8 waves' sums are added through LDS in wave order.
// c + a[23:0] * w for a wave-uniform multiplicity w (an SGPR operand).  As
// inline assembly: left to itself the compiler multiplies (v_mul_u32_u24) and
// adds the products in threes (v_add3_u32), 6 instructions for 4 terms, and
// holds the products of a whole column in VGPRs (241 of them).
__device__ __forceinline__ uint32_t mad_u24(uint32_t a, uint32_t w, uint32_t c) {
  uint32_t d;
  asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "s"(w), "v"(c));
  return d;
}

template <bool DISC>
__device__ __forceinline__ void stir_term(float a, float b, uint32_t wh, uint32_t wm, float k1,
                                          float k2, uint32_t* acc) {
  if (DISC) {
    const uint32_t d = a != b ? 1u : 0u;
    acc[0] = mad_u24(d, wh, acc[0]);
    acc[2] = mad_u24(d, wm, acc[2]);
  } else {
    const float d = a - b;
    const uint32_t f1 = __float_as_uint(__builtin_fabsf(d) + k1);
    const uint32_t f2 = __float_as_uint(__builtin_fmaf(d, d, k2));
    acc[0] = mad_u24(f1, wh, acc[0]);
    acc[1] = mad_u24(f2, wh, acc[1]);
    acc[2] = mad_u24(f1, wm, acc[2]);
    acc[3] = mad_u24(f2, wm, acc[3]);
  }
}

// Order point as in fs_pass2.hip: what computes `v` happens before, and no
// memory access moves across it.
#define FS_STIR_ORDER_AFTER(v) asm volatile("" : "+v"(v)::"memory")

template <bool D0, bool D1, bool TWO>
__device__ __forceinline__ void stir_column(const float (&a0)[kStirRows],
                                            const float (&a1)[kStirRows],
                                            const uint32_t (&w)[2 * kStirRows], float b0,
                                            float b1, float k1, float k2, uint32_t (&acc)[8],
                                            const uint32_t* __restrict__ wnext,
                                            uint32_t (&wn)[2 * kStirRows]) {
  stir_term<D0>(a0[0], b0, w[0], w[kStirRows], k1, k2, acc);
  FS_STIR_ORDER_AFTER(acc[0]);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int r = 0; r < 2 * kStirRows; r++) wn[r] = wnext[r];
  __builtin_amdgcn_sched_barrier(0);  // the scalar loads are issued here
#pragma unroll
  for (int r = 0; r < kStirRows; r++) {
    if (r != 0) stir_term<D0>(a0[r], b0, w[r], w[kStirRows + r], k1, k2, acc);
    if (TWO) stir_term<D1>(a1[r], b1, w[r], w[kStirRows + r], k1, k2, acc + 4);
  }
  __builtin_amdgcn_sched_barrier(0);
}

// Tiles [t_begin, t_end) of the chunk (slots of W); tiles[] is the chunk's
// part of the plan's tile list.
template <bool D0, bool D1, bool TWO>
__device__ __forceinline__ void stir_tiles(const float* __restrict__ xs, int64_t PW, int64_t c0,
                                           int wave, const int2* __restrict__ tiles,
                                           const uint32_t* __restrict__ W, int64_t t_begin,
                                           int64_t t_end, float k1, float k2, double (&s)[8]) {
  float a0[kStirRows], a1[kStirRows];
  int cur_bi = -1;
  // wA holds column 0 of the current tile: the last prefetch of a tile is
  // column 0 of the next slot (W has a spare tile after the chunk's last)
  uint32_t wA[2 * kStirRows], wB[2 * kStirRows];
  {
    const uint32_t* __restrict__ w0 = W + t_begin * kStirTileW + wave * (2 * kStirRows);
#pragma unroll
    for (int r = 0; r < 2 * kStirRows; r++) wA[r] = w0[r];
  }
  for (int64_t t = t_begin; t < t_end; t++) {
    const int2 tl = tiles[t];
    if (tl.x != cur_bi) {
      cur_bi = tl.x;
      const float* __restrict__ xa = xs + ((int64_t)tl.x * kTile + wave * kStirRows) * PW + c0;
#pragma unroll
      for (int r = 0; r < kStirRows; r++) {
        a0[r] = xa[(int64_t)r * PW];
        a1[r] = TWO ? xa[(int64_t)r * PW + 64] : 0.0f;
      }
    }
    const uint32_t* __restrict__ wt = W + t * kStirTileW + wave * (2 * kStirRows);
    const float* __restrict__ xb = xs + (int64_t)tl.y * kTile * PW + c0;
    float bA0 = xb[0], bA1 = TWO ? xb[64] : 0.0f;
    float bB0 = xb[PW], bB1 = TWO ? xb[PW + 64] : 0.0f;
    // the prefetches of the last column pair reach 2 rows past the tile (xs
    // has 2 spare rows) and column 0 of the next slot of W
    const float* __restrict__ xn = xb + 2 * PW;
    const uint32_t* __restrict__ wn = wt + kStirColW;
    for (int jb = 0; jb < kTile; jb += kStirFold) {
      uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int jj = 0; jj < kStirFold; jj += 2) {
        const float cA0 = xn[0], cA1 = TWO ? xn[64] : 0.0f;
        const float cB0 = xn[PW], cB1 = TWO ? xn[PW + 64] : 0.0f;
        stir_column<D0, D1, TWO>(a0, a1, wA, bA0, bA1, k1, k2, acc, wn, wB);
        stir_column<D0, D1, TWO>(a0, a1, wB, bB0, bB1, k1, k2, acc, wn + kStirColW, wA);
        bA0 = cA0; bA1 = cA1; bB0 = cB0; bB1 = cB1;
        xn += 2 * PW;
        wn += 2 * kStirColW;
      }
#pragma unroll
      for (int q = 0; q < 8; q++) s[q] += (double)acc[q];
    }
  }
}

// part[(q * nseg_all + seg0 + seg) * PW + c]: quantity q of segment seg of
// this chunk, permuted column c.
__global__ __launch_bounds__(64 * kStirWaves) void k_stir_score(
    const float* __restrict__ xs, int64_t PW, int64_t PC, const int2* __restrict__ tiles,
    const uint32_t* __restrict__ W, int64_t n_tiles, int64_t seg_len, int64_t nseg, int64_t nfb,
    int64_t seg0, int64_t nseg_all, float k1, float k2, double* __restrict__ part) {
  __shared__ double red[8][kStirWaves][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t w = blockIdx.x;
  const int64_t xcd = w % kXcds, k = w / kXcds;
  const int64_t seg = xcd + kXcds * (k / nfb), fb = k % nfb;
  if (seg >= nseg) return;
  const int64_t f0 = fb * 128;
  const int64_t c0 = f0 + lane;
  const int64_t t_begin = seg * seg_len;
  const int64_t t_end = t_begin + seg_len < n_tiles ? t_begin + seg_len : n_tiles;
  const bool two = f0 + 64 < PW;
  const bool d0 = f0 >= PC, d1 = f0 + 64 >= PC;
  double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (two) {
    if (!d1) stir_tiles<false, false, true>(xs, PW, c0, wave, tiles, W, t_begin, t_end, k1, k2, s);
    else if (d0) stir_tiles<true, true, true>(xs, PW, c0, wave, tiles, W, t_begin, t_end, k1, k2, s);
    else stir_tiles<false, true, true>(xs, PW, c0, wave, tiles, W, t_begin, t_end, k1, k2, s);
  } else {
    if (d0) stir_tiles<true, true, false>(xs, PW, c0, wave, tiles, W, t_begin, t_end, k1, k2, s);
    else stir_tiles<false, false, false>(xs, PW, c0, wave, tiles, W, t_begin, t_end, k1, k2, s);
  }
  // a discrete feature's diff^2 is its diff (plain counts); a continuous
  // feature's integers are in units of K 2^-23 (exact power-of-two scaling)
  const double u1 = (double)k1 * 0x1p-23, u2 = (double)k2 * 0x1p-23;
  if (d0) { s[1] = s[0]; s[3] = s[2]; }
  else { s[0] *= u1; s[1] *= u2; s[2] *= u1; s[3] *= u2; }
  if (d1) { s[5] = s[4]; s[7] = s[6]; }
  else { s[4] *= u1; s[5] *= u2; s[6] *= u1; s[7] *= u2; }
#pragma unroll
  for (int q = 0; q < 8; q++) red[q][wave][lane] = s[q];
  __syncthreads();
  // wave v adds the 8 waves' sums of one (feature half, quantity) in wave order
  const int half = wave >> 2, q = wave & 3;
  if (half == 0 || two) {
    double v = 0.0;
#pragma unroll
    for (int u = 0; u < kStirWaves; u++) v += red[wave][u][lane];
    part[((int64_t)q * nseg_all + seg0 + seg) * PW + c0 + half * 64] = v;
  }
}

// Tiles per chunk of the per-pair buffer (128 KB a tile: 512 MB); the
// stir_chunk test hook sets it.  A chunk is a whole number of segments.
constexpr int64_t kStirChunkTiles = 4096;
// workgroups aimed at over all chunks (as shard_segments' dense target)
constexpr int64_t kStirWorkgroups = 32768;

// The fixed-point offset for values in [0, v]: the smallest power of two with
// an even biased exponent (an odd power of two) above v, with a little room
// for the float32 rounding of the operands.
static float stir_offset(double v) {
  int e = 1;
  (void)std::frexp(std::max(v, 0.0) * 1.001, &e);  // v * 1.001 < 2^e
  if (e % 2 == 0) e++;
  return (float)std::ldexp(1.0, e);
}

static int stir_events(Plan* g, size_t count) {
  while (g->ev_stir.size() < count) {
    hipEvent_t e = event_get(g->device, true);
    if (!e) return FS_EHIP;
    g->ev_stir.push_back(e);
  }
  return FS_OK;
}

int plan_stir(Plan* g, double* sums) {
  const Prepared& Q = g->P;
  FS_HIP(hipSetDevice(g->device));
  // the previous call's buffers (kept when the stream is the caller's)
  if (!g->mem_call.blocks.empty()) {
    FS_HIP(hipStreamSynchronize(g->stream));
    g->mem_call.release();
  }
  g->stir_chunks = 0;
  FS_HIP(hipMemsetAsync(sums, 0, sizeof(double) * 4 * Q.n_kept, g->stream));
  if (g->n_tiles == 0) {
    if (g->own_stream) FS_HIP(hipStreamSynchronize(g->stream));
    return FS_OK;
  }
  const int64_t nfb = (Q.PW + 127) / 128;
  // tiles per segment (one workgroup walks a segment per feature block); the
  // stir_seg_len test hook sets it: small problems compute 1
  int64_t seg_len =
      std::max<int64_t>(1, (g->n_tiles * nfb + kStirWorkgroups - 1) / kStirWorkgroups);
  if (test_hooks().stir_seg_len >= 1) seg_len = test_hooks().stir_seg_len;
  const int64_t nseg_all = (g->n_tiles + seg_len - 1) / seg_len;
  int64_t chunk = test_hooks().stir_chunk >= 1 ? test_hooks().stir_chunk : kStirChunkTiles;
  chunk = std::min(g->n_tiles, (chunk + seg_len - 1) / seg_len * seg_len);
  const int64_t nchunks = (g->n_tiles + chunk - 1) / chunk;
  uint32_t* W = nullptr;
  // continuous diffs lie in [0, Rmax], their squares in [0, Rmax^2]
  const float k1 = stir_offset(Q.Rmax), k2 = stir_offset(Q.Rmax * Q.Rmax);
  double* part = nullptr;
  FS_TRY(g->mem_call.alloc(&W, (size_t)(chunk + 1) * kStirTileW));
  FS_TRY(g->mem_call.alloc(&part, (size_t)4 * nseg_all * Q.PW));
  FS_TRY(stir_events(g, (size_t)4 * nchunks));
  for (int64_t c = 0; c < nchunks; c++) {
    const int64_t t0 = c * chunk, nt = std::min(chunk, g->n_tiles - t0);
    const int64_t nseg = (nt + seg_len - 1) / seg_len;
    const int64_t seg_per_xcd = (nseg + kXcds - 1) / kXcds;
    hipEvent_t* ev = g->ev_stir.data() + 4 * c;
    FS_HIP(hipEventRecord(ev[0], g->stream));
    k_stir_weights<<<(unsigned)nt, 256, 0, g->stream>>>(g->D, Q.n, Q.n_pad, g->tiled, g->win,
                                                        g->tiles, t0, g->thr, g->lab, g->r_lo,
                                                        g->r_hi, W);
    FS_TRY(launch_check("k_stir_weights"));
    FS_HIP(hipEventRecord(ev[1], g->stream));
    FS_HIP(hipEventRecord(ev[2], g->stream));
    k_stir_score<<<(unsigned)(kXcds * seg_per_xcd * nfb), 64 * kStirWaves, 0, g->stream>>>(
        g->xs, Q.PW, Q.PC, g->tiles + t0, W, nt, seg_len, nseg, nfb, t0 / seg_len, nseg_all, k1, k2,
        part);
    FS_TRY(launch_check("k_stir_score"));
    FS_HIP(hipEventRecord(ev[3], g->stream));
    g->stir_chunks = (int)(c + 1);
  }
  for (int q = 0; q < 4; q++)
    FS_TRY(reduce_segments(part + (size_t)q * nseg_all * Q.PW, nseg_all, Q.PW, g->out_pos,
                           sums + (size_t)q * Q.n_kept, g->stream));
  if (g->own_stream) {
    FS_HIP(hipStreamSynchronize(g->stream));
    g->mem_call.release();
  }
  return FS_OK;
}

// Summed HIP-event time of the last plan_stir's weights (which == 0) or score
// (1) kernels over its chunks, in milliseconds; -1 when unavailable.
// which == 2: k_rf_stir of the last plan_score_stir (fs_stir_relieff.hip).
double plan_stir_kernel_ms(const Plan* g, int which) {
  if (which == 2) {
    float ms = -1.0f;
    if (!g->rf_stir_timed || hipEventSynchronize(g->ev_rf_stir[1]) != hipSuccess ||
        hipEventElapsedTime(&ms, g->ev_rf_stir[0], g->ev_rf_stir[1]) != hipSuccess) {
      (void)hipGetLastError();
      return -1.0;
    }
    return (double)ms;
  }
  if (g->stir_chunks <= 0 || which < 0 || which > 1) return -1.0;
  double total = 0.0;
  for (int c = 0; c < g->stir_chunks; c++) {
    float ms = -1.0f;
    hipEvent_t a = g->ev_stir[4 * c + 2 * which], b = g->ev_stir[4 * c + 2 * which + 1];
    if (hipEventSynchronize(b) != hipSuccess || hipEventElapsedTime(&ms, a, b) != hipSuccess) {
      (void)hipGetLastError();
      return -1.0;
    }
    total += (double)ms;
  }
  return total;
}

}  // namespace gpu
}  // namespace fs
