// fs_mrmr.hip -- the GPU backend of fs_mrmr_*: selection-only mRMR.  The
// relevance and one row of mutual information per selected feature, and the
// greedy loop of mRMR.fit (mRMR.py:96-117) on the device: every launch of a
// fit is queued on one stream and the host synchronises once.  Nothing of
// size p x p exists (replaces the calculate_mi_matrices call of mRMR.py:94-96
// for callers who do not need redundancy_matrix_).
//
//   k_mi_pack     (fs_mi.hip) the codes -> word-major state bit-planes
//                 planes[(w * P1p + c) * SP + s]; the columns are padded to a
//                 whole number of k_mi_row workgroups, y is column p.
//   k_mi_row      one anchor column (a feature, or y for the relevance)
//                 against kMrThreads / NB^2 columns per workgroup (NB = SP / 4),
//                 with the scan of k_cfs_row (fs_cfs.hip): the anchor's planes
//                 staged in LDS per chunk of kMrWC words, a column's planes as
//                 16-byte vectors straight from HBM, one 4 x 4 block of a
//                 pair's table in 16 registers per lane.  The epilogue is
//                 k_mi_scan's (fs_mi.hip), over the transposed indices when the
//                 anchor has the higher index: mi_pxy, the marginals in index
//                 order, mi_term on the lane that counted the cell, the pair's
//                 first lane adding row-major over kcol[lo] x kcol[hi], then
//                 mi_constant and mi_finish.  Same expressions in the same
//                 order: a value equals fs_mi_matrices' entry of the same
//                 device bit for bit.  The same lane adds the value to the
//                 running redundancy sum and stores it into the caller's row
//                 when asked.  The anchor may be read from device memory, so
//                 a row is queued behind the pick that chose it.
//   k_mrmr_score  one lane per remaining feature: its score (fs_mrmr.h), then
//                 the workgroup's maximum in a fixed tree.
//   k_mrmr_ties   the global maximum from the workgroups' maxima, the tie set
//                 (mrmr_is_top), then the workgroup's best (mean redundancy,
//                 index) by mrmr_beats.
//   k_mrmr_pick   one workgroup: the best of the workgroups' results;
//                 taken[best] = 1 and sel[i] = best, which is also the anchor
//                 word of the next k_mi_row.
//   k_mrmr_addrow (fs_mrmr_search_matrix) adds the picked feature's row of the
//                 caller's matrix where k_mi_row would have computed it.
// No float atomics: two fits of the same data give identical bits.
#include "fs_gpu_internal.h"
#include "fs_mrmr.h"

namespace fs {
namespace gpu {

namespace {

constexpr int kMrThreads = 256;
constexpr int kMrWC = 64;         // words (2048 samples) of the anchor staged per chunk
constexpr int kMrPx = 4096;       // most cells of a workgroup's tables: CPW * SP^2
constexpr int kMrMarg = 1024;     // most marginals of a workgroup: CPW * SP
constexpr int64_t kMrTimedSteps = 64;  // steps timed one by one (two events each)

thread_local double g_mrmr_ms[5] = {-1.0, -1.0, -1.0, -1.0, -1.0};

struct MiRowArgs {
  const uint32_t* planes;
  const int32_t* kcol;        // P1 state counts
  int64_t n, p, P1p, W;
  int SP, NB, CPW;            // CPW: columns per workgroup
  int unit;
  int64_t anchor;             // the anchor column (p: the target) ...
  const int64_t* anchor_dev;  // ... or where to read it (negative: nothing to do)
  double* out;                // NULL, or p values
  double* rsum;               // NULL, or p sums: rsum[c] += value
};

__global__ __launch_bounds__(kMrThreads) void k_mi_row(const MiRowArgs a) {
  __shared__ __align__(16) uint32_t s_anc[kMrWC * kMiMaxStatesGpu];
  __shared__ double s_px[kMrPx];  // [pair][SP][SP]: pxy, then the terms
  __shared__ double s_p1[kMrMarg];
  __shared__ double s_p2[kMrMarg];
  const int tid = threadIdx.x;
  const int64_t anc = a.anchor_dev ? *a.anchor_dev : a.anchor;
  if (anc < 0) return;
  const int SP = a.SP, NB = a.NB, CPW = a.CPW;
  const int L = NB * NB;  // lanes per pair
  const int q = tid / L, blk = tid - q * L;
  const int ab = blk / NB, bb = blk - ab * NB;  // the anchor's / the column's block of 4 states
  const bool lane_on = q < CPW;
  const int64_t c = (int64_t)blockIdx.x * CPW + (lane_on ? q : 0);  // < P1p
  const bool pair_on = lane_on && c < a.p;

  uint32_t cnt[16];
#pragma unroll
  for (int k = 0; k < 16; k++) cnt[k] = 0;

  const uint4* g4 = reinterpret_cast<const uint4*>(a.planes);
  uint4* s4 = reinterpret_cast<uint4*>(s_anc);
  for (int64_t w0 = 0; w0 < a.W; w0 += kMrWC) {
    const int wn = a.W - w0 < kMrWC ? (int)(a.W - w0) : kMrWC;
    for (int v = tid; v < wn * NB; v += kMrThreads) {
      const int w = v / NB, xb = v - w * NB;
      s4[v] = g4[((size_t)(w0 + w) * a.P1p + anc) * NB + xb];
    }
    __syncthreads();
    if (pair_on) {
      const uint4* gc = g4 + ((size_t)w0 * a.P1p + c) * NB + bb;
      const size_t gstep = (size_t)a.P1p * NB;
      for (int w = 0; w < wn; w++) {
        const uint4 A = s4[w * NB + ab], B = gc[(size_t)w * gstep];
        cnt[0] += __builtin_popcount(A.x & B.x);
        cnt[1] += __builtin_popcount(A.x & B.y);
        cnt[2] += __builtin_popcount(A.x & B.z);
        cnt[3] += __builtin_popcount(A.x & B.w);
        cnt[4] += __builtin_popcount(A.y & B.x);
        cnt[5] += __builtin_popcount(A.y & B.y);
        cnt[6] += __builtin_popcount(A.y & B.z);
        cnt[7] += __builtin_popcount(A.y & B.w);
        cnt[8] += __builtin_popcount(A.z & B.x);
        cnt[9] += __builtin_popcount(A.z & B.y);
        cnt[10] += __builtin_popcount(A.z & B.z);
        cnt[11] += __builtin_popcount(A.z & B.w);
        cnt[12] += __builtin_popcount(A.w & B.x);
        cnt[13] += __builtin_popcount(A.w & B.y);
        cnt[14] += __builtin_popcount(A.w & B.z);
        cnt[15] += __builtin_popcount(A.w & B.w);
      }
    }
    __syncthreads();
  }

  // epilogue (fs_mi.h, as k_mi_scan).  cnt[r * 4 + k] counts (anchor state
  // 4 ab + r, column state 4 bb + k); the column with the lower index supplies
  // the table's rows
  const bool swap = anc > c;
  const double dn = (double)a.n;
  const int tq = q * SP * SP;
  double px[16];
#pragma unroll
  for (int k = 0; k < 16; k++) px[k] = mi_pxy((int32_t)cnt[k], dn);
  if (lane_on) {
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int sa = 4 * ab + r, sc = 4 * bb + k;
        s_px[tq + (swap ? sc * SP + sa : sa * SP + sc)] = px[r * 4 + k];
      }
  }
  __syncthreads();
  for (int it = tid; it < CPW * SP; it += kMrThreads) {
    const int q2 = it / SP, s = it - q2 * SP;
    const double* t = s_px + q2 * SP * SP;
    double r1 = 0.0, r2 = 0.0;
    for (int b = 0; b < SP; b++) r1 += t[s * SP + b];
    for (int b = 0; b < SP; b++) r2 += t[b * SP + s];
    s_p1[it] = r1;
    s_p2[it] = r2;
  }
  __syncthreads();
  if (pair_on) {
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int sa = 4 * ab + r, sc = 4 * bb + k;
        const int row = swap ? sc : sa, col = swap ? sa : sc;
        s_px[tq + row * SP + col] =
            mi_term(px[r * 4 + k], s_p1[q * SP + row], s_p2[q * SP + col]);
      }
  }
  __syncthreads();
  if (pair_on && blk == 0) {
    const int64_t lo = swap ? c : anc, hi = swap ? anc : c;
    // a state count never exceeds SP on packed data; the bound keeps the loop
    // inside the table while a rejected call (a code >= n_states) drains
    const int k1 = a.kcol[lo] < SP ? a.kcol[lo] : SP, k2 = a.kcol[hi] < SP ? a.kcol[hi] : SP;
    const double* t = s_px + tq;
    double mi = 0.0;
    for (int r = 0; r < k1; r++)
      for (int k = 0; k < k2; k++) mi += t[r * SP + k];
    int used1 = 0, used2 = 0;
    for (int r = 0; r < k1; r++) used1 += s_p1[q * SP + r] > 0.0;
    for (int k = 0; k < k2; k++) used2 += s_p2[q * SP + k] > 0.0;
    mi = (c == anc || mi_constant(used1, used2)) ? 0.0 : mi_finish(mi, a.unit);
    if (a.out) a.out[c] = mi;
    if (a.rsum) a.rsum[c] += mi;
  }
}

// ---- one step of the greedy loop -------------------------------------------
struct MrmrStepArgs {
  const double* rel;
  const double* rsum;
  uint8_t* taken;
  int64_t p, nblk, i;  // i: the step (0: the first feature)
  int method;
  double* pm;          // per workgroup: the highest score (-inf: no candidate)
  double* pa;          // per workgroup: the best top candidate's mean redundancy ...
  int64_t* pi;         // ... and its index (-1: none)
  int64_t* sel;
};

__device__ __forceinline__ double mrmr_block_max(double v, double* sm) {
  const int tid = threadIdx.x;
  sm[tid] = v;
  __syncthreads();
  for (int s = kMrThreads / 2; s > 0; s >>= 1) {
    if (tid < s && sm[tid + s] > sm[tid]) sm[tid] = sm[tid + s];
    __syncthreads();
  }
  const double r = sm[0];
  __syncthreads();
  return r;
}

__device__ __forceinline__ void mrmr_block_best(double& av, int64_t& bi, double* sm,
                                                int64_t* si) {
  const int tid = threadIdx.x;
  sm[tid] = av;
  si[tid] = bi;
  __syncthreads();
  for (int s = kMrThreads / 2; s > 0; s >>= 1) {
    if (tid < s && mrmr_beats(sm[tid + s], si[tid + s], sm[tid], si[tid])) {
      sm[tid] = sm[tid + s];
      si[tid] = si[tid + s];
    }
    __syncthreads();
  }
  av = sm[0];
  bi = si[0];
}

__global__ __launch_bounds__(kMrThreads) void k_mrmr_score(const MrmrStepArgs a) {
  __shared__ double sm[kMrThreads];
  const int64_t f = (int64_t)blockIdx.x * kMrThreads + threadIdx.x;
  double v = -HUGE_VAL;
  if (f < a.p && !a.taken[f]) v = mrmr_score(a.method, a.i, a.rel[f], a.rsum[f]);
  v = mrmr_block_max(v, sm);
  if (threadIdx.x == 0) a.pm[blockIdx.x] = v;
}

__global__ __launch_bounds__(kMrThreads) void k_mrmr_ties(const MrmrStepArgs a) {
  __shared__ double sm[kMrThreads];
  __shared__ int64_t si[kMrThreads];
  double mx = -HUGE_VAL;
  for (int64_t b = threadIdx.x; b < a.nblk; b += kMrThreads)
    if (a.pm[b] > mx) mx = a.pm[b];
  mx = mrmr_block_max(mx, sm);
  const int64_t f = (int64_t)blockIdx.x * kMrThreads + threadIdx.x;
  double av = 0.0;
  int64_t bi = -1;
  // the score is recomputed from the same operands: the same bits as in
  // k_mrmr_score
  if (f < a.p && !a.taken[f] &&
      mrmr_is_top(a.i, mrmr_score(a.method, a.i, a.rel[f], a.rsum[f]), mx)) {
    av = mrmr_avg(a.i, a.rsum[f]);
    bi = f;
  }
  mrmr_block_best(av, bi, sm, si);
  if (threadIdx.x == 0) {
    a.pa[blockIdx.x] = av;
    a.pi[blockIdx.x] = bi;
  }
}

__global__ __launch_bounds__(kMrThreads) void k_mrmr_pick(const MrmrStepArgs a) {
  __shared__ double sm[kMrThreads];
  __shared__ int64_t si[kMrThreads];
  double av = 0.0;
  int64_t bi = -1;
  for (int64_t b = threadIdx.x; b < a.nblk; b += kMrThreads)
    if (mrmr_beats(a.pa[b], a.pi[b], av, bi)) av = a.pa[b], bi = a.pi[b];
  mrmr_block_best(av, bi, sm, si);
  if (threadIdx.x == 0 && bi >= 0) {
    a.taken[bi] = 1;
    a.sel[a.i] = bi;
  }
}

// rsum[c] += red[*anchor][c]: the caller's matrix in the place of k_mi_row.
__global__ __launch_bounds__(256) void k_mrmr_addrow(const double* __restrict__ red, int64_t p,
                                                     const int64_t* __restrict__ anchor,
                                                     double* __restrict__ rsum) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t anc = *anchor;
  if (c >= p || anc < 0) return;
  rsum[c] += red[(size_t)anc * p + c];
}

// The buffers and launches of the greedy loop, over computed rows or a
// caller's matrix.
struct MrmrSteps {
  hipStream_t s = nullptr;
  int64_t p = 0, k = 0, nblk = 0;
  int method = 0;
  double *rel = nullptr, *rsum = nullptr, *pm = nullptr, *pa = nullptr;
  int64_t *pi = nullptr, *sel = nullptr;
  uint8_t* taken = nullptr;

  int alloc(DevArena& mem) {
    nblk = (p + kMrThreads - 1) / kMrThreads;
    FS_TRY(mem.alloc(&rel, (size_t)p));
    FS_TRY(mem.alloc(&rsum, (size_t)p));
    FS_TRY(mem.alloc(&taken, (size_t)p));
    FS_TRY(mem.alloc(&sel, (size_t)k));
    FS_TRY(mem.alloc(&pm, (size_t)nblk));
    FS_TRY(mem.alloc(&pa, (size_t)nblk));
    FS_TRY(mem.alloc(&pi, (size_t)nblk));
    return FS_OK;
  }
  int reset() {
    FS_HIP(hipMemsetAsync(rsum, 0, (size_t)p * 8, s));  // +0.0
    FS_HIP(hipMemsetAsync(taken, 0, (size_t)p, s));
    FS_HIP(hipMemsetAsync(sel, 0xff, (size_t)k * 8, s));  // -1: nothing picked yet
    return FS_OK;
  }
  int step(int64_t i) {
    MrmrStepArgs a;
    a.rel = rel, a.rsum = rsum, a.taken = taken, a.p = p, a.nblk = nblk, a.i = i;
    a.method = method, a.pm = pm, a.pa = pa, a.pi = pi, a.sel = sel;
    k_mrmr_score<<<(unsigned)nblk, kMrThreads, 0, s>>>(a);
    FS_TRY(launch_check("k_mrmr_score"));
    k_mrmr_ties<<<(unsigned)nblk, kMrThreads, 0, s>>>(a);
    FS_TRY(launch_check("k_mrmr_ties"));
    k_mrmr_pick<<<1, kMrThreads, 0, s>>>(a);
    return launch_check("k_mrmr_pick");
  }
};

struct StreamLease {
  int device;
  hipStream_t s = nullptr;
  std::vector<hipEvent_t> ev;
  explicit StreamLease(int dev) : device(dev) {}
  ~StreamLease() {  // before the arenas declared ahead of it free their blocks
    if (s) {
      (void)hipStreamSynchronize(s);
      stream_put(device, s);
    }
    for (hipEvent_t e : ev)
      if (e) event_put(device, e, true);
    (void)hipGetLastError();
  }
};

int no_device() {
  set_error("backend='gpu' requested but no HIP device is visible");
  return FS_ENODEV;
}

}  // namespace

void mrmr_last_timing(double* ms5) {
  for (int k = 0; k < 5; k++) ms5[k] = g_mrmr_ms[k];
}

int mrmr_select(int device, const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p,
                int n_states, int unit, int method, int64_t k, double* relevance,
                int64_t* selected, double* rows) {
  if (device_count() <= 0) return no_device();
  for (double& v : g_mrmr_ms) v = -1.0;
  const int S = n_states;
  const int NB = (S + 3) / 4, SP = NB * 4, CPW = kMrThreads / (NB * NB);
  const int64_t P1 = p + 1;
  const int64_t P1p = (P1 + CPW - 1) / CPW * CPW;
  const int64_t W = (n + 31) / 32;
  // sizes in floating point first: a request beyond any device is an
  // out-of-memory answer, not an overflowed size
  const double kMaxBytes = 1e15;
  if ((double)W * (double)P1p * SP * 4.0 > kMaxBytes || (double)n * (double)p > kMaxBytes ||
      (rows && (double)k * (double)p * 8.0 > kMaxBytes)) {
    set_error("fs_mrmr_select: the bit-planes and rows do not fit the device memory");
    return FS_EOOM;
  }
  FS_HIP(hipSetDevice(device));
  DevArena mem(device);
  StreamLease lease(device);  // destroyed (and the stream synchronised) before `mem`
  lease.s = stream_get(device);
  // timing: upload, pack, relevance, then (row, step) pairs; above
  // kMrTimedSteps steps the loop is timed as a whole
  const bool per_step = k - 1 <= kMrTimedSteps;
  const size_t nev = 4 + (per_step ? 2 * (size_t)(k - 1) + 1 : 1);
  if (!lease.s) return FS_EHIP;
  for (size_t e = 0; e < nev; e++) {
    lease.ev.push_back(event_get(device, true));
    if (!lease.ev.back()) return FS_EHIP;
  }
  hipStream_t s = lease.s;
  std::vector<hipEvent_t>& ev = lease.ev;

  MrmrSteps st;
  st.s = s, st.p = p, st.k = k, st.method = method;
  uint8_t *dx = nullptr, *dy = nullptr;
  uint32_t* planes = nullptr;
  int32_t* kcol = nullptr;
  double* drows = nullptr;
  int* dbad = nullptr;
  // every block is allocated before any array is read
  FS_TRY(mem.alloc(&dx, (size_t)n * p));
  FS_TRY(mem.alloc(&dy, (size_t)n));
  FS_TRY(mem.alloc(&planes, (size_t)W * P1p * SP));
  FS_TRY(mem.alloc(&kcol, (size_t)P1));
  FS_TRY(mem.alloc(&dbad, 1));
  FS_TRY(st.alloc(mem));
  if (rows) FS_TRY(mem.alloc(&drows, (size_t)k * p));

  FS_HIP(hipEventRecord(ev[0], s));
  FS_HIP(hipMemcpyAsync(dx, codes, (size_t)n * p, hipMemcpyHostToDevice, s));
  FS_HIP(hipMemcpyAsync(dy, ycodes, (size_t)n, hipMemcpyHostToDevice, s));
  FS_HIP(hipMemsetAsync(dbad, 0, 4, s));
  FS_HIP(hipMemsetAsync(kcol, 0, (size_t)P1 * 4, s));
  FS_TRY(st.reset());
  FS_HIP(hipEventRecord(ev[1], s));
  FS_HIP(mi_pack(dx, dy, n, p, P1p, S, SP, planes, kcol, dbad, s));
  FS_HIP(hipEventRecord(ev[2], s));

  MiRowArgs a;
  a.planes = planes, a.kcol = kcol, a.n = n, a.p = p, a.P1p = P1p, a.W = W;
  a.SP = SP, a.NB = NB, a.CPW = CPW, a.unit = unit;
  auto launch_row = [&](int64_t anchor, const int64_t* anchor_dev, double* out, double* rsum) {
    a.anchor = anchor, a.anchor_dev = anchor_dev, a.out = out, a.rsum = rsum;
    k_mi_row<<<(unsigned)(P1p / CPW), kMrThreads, 0, s>>>(a);
    return launch_check("k_mi_row");
  };
  FS_TRY(launch_row(p, nullptr, st.rel, nullptr));  // the target is column p
  FS_TRY(st.step(0));
  FS_HIP(hipEventRecord(ev[3], s));
  // k - 1 x (the last pick's row into the sum, the next pick), back to back
  for (int64_t i = 1; i < k; i++) {
    FS_TRY(launch_row(-1, st.sel + (i - 1), rows ? drows + (size_t)(i - 1) * p : nullptr, st.rsum));
    if (per_step) FS_HIP(hipEventRecord(ev[2 + 2 * i], s));
    FS_TRY(st.step(i));
    if (per_step) FS_HIP(hipEventRecord(ev[3 + 2 * i], s));
  }
  // the last pick's row feeds no step: only a caller's rows need it
  if (rows) FS_TRY(launch_row(-1, st.sel + (k - 1), drows + (size_t)(k - 1) * p, nullptr));
  FS_HIP(hipEventRecord(ev[nev - 1], s));

  int bad = 0;
  FS_HIP(hipMemcpyAsync(&bad, dbad, 4, hipMemcpyDeviceToHost, s));
  FS_HIP(hipMemcpyAsync(selected, st.sel, (size_t)k * 8, hipMemcpyDeviceToHost, s));
  FS_HIP(hipMemcpyAsync(relevance, st.rel, (size_t)p * 8, hipMemcpyDeviceToHost, s));
  if (rows)
    FS_HIP(hipMemcpyAsync(rows, drows, (size_t)k * p * 8, hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  if (bad) {
    set_error("fs_mrmr_select: a code is >= n_states");
    return FS_EINVAL;
  }
  auto span = [&](size_t e0, size_t e1) {
    float ms = -1.0f;
    return hipEventElapsedTime(&ms, ev[e0], ev[e1]) == hipSuccess ? (double)ms : -1.0;
  };
  for (int t = 0; t < 3; t++) g_mrmr_ms[t] = span(t, t + 1);
  if (per_step) {
    // ev[3 + 2 (i - 1)] .. ev[2 + 2 i]: row i - 1; .. ev[3 + 2 i]: step i;
    // the last row of a caller's rows ends at ev[nev - 1]
    double r = 0.0, t = 0.0;
    bool ok = true;
    for (int64_t i = 1; i < k; i++) {
      const double a0 = span(1 + 2 * i, 2 + 2 * i), a1 = span(2 + 2 * i, 3 + 2 * i);
      ok = ok && a0 >= 0.0 && a1 >= 0.0;
      r += a0, t += a1;
    }
    const double last = span(nev - 2, nev - 1);
    ok = ok && last >= 0.0;
    g_mrmr_ms[3] = ok ? r + last : -1.0;
    g_mrmr_ms[4] = ok ? t : -1.0;
  } else {
    g_mrmr_ms[3] = span(3, 4);  // rows and steps together; steps stays -1
  }
  (void)hipGetLastError();
  return FS_OK;
}

int mrmr_search_matrix(int device, const double* relevance, const double* redundancy, int64_t p,
                       int method, int64_t k, int64_t* selected) {
  if (device_count() <= 0) return no_device();
  if ((double)p * (double)p * 8.0 > 1e15) {
    set_error("fs_mrmr_search_matrix: the matrix does not fit the device memory");
    return FS_EOOM;
  }
  FS_HIP(hipSetDevice(device));
  DevArena mem(device);
  StreamLease lease(device);
  lease.s = stream_get(device);
  if (!lease.s) return FS_EHIP;
  hipStream_t s = lease.s;
  MrmrSteps st;
  st.s = s, st.p = p, st.k = k, st.method = method;
  double* dred = nullptr;
  FS_TRY(st.alloc(mem));
  FS_TRY(mem.alloc(&dred, (size_t)p * p));
  FS_HIP(hipMemcpyAsync(st.rel, relevance, (size_t)p * 8, hipMemcpyHostToDevice, s));
  FS_HIP(hipMemcpyAsync(dred, redundancy, (size_t)p * p * 8, hipMemcpyHostToDevice, s));
  FS_TRY(st.reset());
  FS_TRY(st.step(0));
  for (int64_t i = 1; i < k; i++) {
    k_mrmr_addrow<<<(unsigned)((p + 255) / 256), 256, 0, s>>>(dred, p, st.sel + (i - 1), st.rsum);
    FS_TRY(launch_check("k_mrmr_addrow"));
    FS_TRY(st.step(i));
  }
  FS_HIP(hipMemcpyAsync(selected, st.sel, (size_t)k * 8, hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  return FS_OK;
}

}  // namespace gpu
}  // namespace fs
