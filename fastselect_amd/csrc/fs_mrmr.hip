// fs_mrmr.hip -- the GPU backend of fs_mrmr_*: selection-only mRMR.  The
// relevance and one row of mutual information per selected feature, and the
// greedy loop of mRMR.fit (mRMR.py:96-117) on the device: every launch of a
// fit is queued on one stream and the host synchronises once.  Nothing of
// size p x p exists (replaces the calculate_mi_matrices call of mRMR.py:94-96
// for callers who do not need redundancy_matrix_).
//
//   k_mi_pack     (fs_mi.hip, through MiPlanes) the codes -> word-major state
//                 bit-planes planes[(w * P1p + c) * SP + s]; the columns are
//                 padded to a whole number of k_mi_row workgroups, y is
//                 column p.
//   k_mi_row      one anchor column (a feature, or y for the relevance)
//                 against kPtThreads / NB^2 columns per workgroup (NB = SP / 4).
//                 The scan and the epilogue are pt_row's (fs_pairtab.h): the
//                 anchor's planes staged in LDS per chunk of kPtWC words, a
//                 column's planes as 16-byte vectors straight from HBM, one
//                 4 x 4 block of a pair's table in 16 registers per lane; then
//                 pt_epilogue with MiTerms, the steps k_mi_scan runs in its
//                 own copy (fs_mi.hip says why), over the transposed indices
//                 when the anchor has the higher index:
//                 mi_pxy, the marginals in index order, mi_term on the lane
//                 that counted the cell, the pair's first lane adding row-major
//                 over kcol[lo] x kcol[hi]; here that lane applies mi_constant
//                 and mi_finish as k_mi_scan does.  Same expressions in the
//                 same order: a value equals fs_mi_matrices' entry of the same
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
#include "fs_pairtab.h"

namespace fs {
namespace gpu {

namespace {

constexpr int64_t kMrTimedSteps = 64;  // steps timed one by one (two events each)

thread_local double g_mrmr_ms[5] = {-1.0, -1.0, -1.0, -1.0, -1.0};

struct MiRowArgs {
  PtRowArgs row;
  int unit;
  double* out;   // NULL, or p values
  double* rsum;  // NULL, or p sums: rsum[c] += value
};

// The scan and the epilogue are pt_row's (fs_pairtab.h) with k_mi_scan's
// parameters; the pair's first lane finishes the value as k_mi_scan does.
__global__ __launch_bounds__(kPtThreads) void k_mi_row(const MiRowArgs a) {
  int64_t c;
  PtPair r;
  if (!pt_row<MiTerms, true>(a.row, c, r)) return;
  const double mi =
      (r.lo == r.hi || mi_constant(r.used1, r.used2)) ? 0.0 : mi_finish(r.sum, a.unit);
  if (a.out) a.out[c] = mi;
  if (a.rsum) a.rsum[c] += mi;
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
  for (int s = kPtThreads / 2; s > 0; s >>= 1) {
    if (tid < s && sm[tid + s] > sm[tid]) sm[tid] = sm[tid + s];
    __syncthreads();
  }
  const double r = sm[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kPtThreads) void k_mrmr_score(const MrmrStepArgs a) {
  __shared__ double sm[kPtThreads];
  const int64_t f = (int64_t)blockIdx.x * kPtThreads + threadIdx.x;
  double v = -HUGE_VAL;
  if (f < a.p && !a.taken[f]) v = mrmr_score(a.method, a.i, a.rel[f], a.rsum[f]);
  v = mrmr_block_max(v, sm);
  if (threadIdx.x == 0) a.pm[blockIdx.x] = v;
}

__global__ __launch_bounds__(kPtThreads) void k_mrmr_ties(const MrmrStepArgs a) {
  __shared__ double sm[kPtThreads];
  __shared__ int64_t si[kPtThreads];
  double mx = -HUGE_VAL;
  for (int64_t b = threadIdx.x; b < a.nblk; b += kPtThreads)
    if (a.pm[b] > mx) mx = a.pm[b];
  mx = mrmr_block_max(mx, sm);
  const int64_t f = (int64_t)blockIdx.x * kPtThreads + threadIdx.x;
  double av = 0.0;
  int64_t bi = -1;
  // the score is recomputed from the same operands: the same bits as in
  // k_mrmr_score
  if (f < a.p && !a.taken[f] &&
      mrmr_is_top(a.i, mrmr_score(a.method, a.i, a.rel[f], a.rsum[f]), mx)) {
    av = mrmr_avg(a.i, a.rsum[f]);
    bi = f;
  }
  pt_block_best<mrmr_beats>(av, bi, sm, si);
  if (threadIdx.x == 0) {
    a.pa[blockIdx.x] = av;
    a.pi[blockIdx.x] = bi;
  }
}

__global__ __launch_bounds__(kPtThreads) void k_mrmr_pick(const MrmrStepArgs a) {
  __shared__ double sm[kPtThreads];
  __shared__ int64_t si[kPtThreads];
  double av = 0.0;
  int64_t bi = -1;
  for (int64_t b = threadIdx.x; b < a.nblk; b += kPtThreads)
    if (mrmr_beats(a.pa[b], a.pi[b], av, bi)) av = a.pa[b], bi = a.pi[b];
  pt_block_best<mrmr_beats>(av, bi, sm, si);
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
    nblk = (p + kPtThreads - 1) / kPtThreads;
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
    k_mrmr_score<<<(unsigned)nblk, kPtThreads, 0, s>>>(a);
    FS_TRY(launch_check("k_mrmr_score"));
    k_mrmr_ties<<<(unsigned)nblk, kPtThreads, 0, s>>>(a);
    FS_TRY(launch_check("k_mrmr_ties"));
    k_mrmr_pick<<<1, kPtThreads, 0, s>>>(a);
    return launch_check("k_mrmr_pick");
  }
};

}  // namespace

void mrmr_last_timing(double* ms5) {
  for (int k = 0; k < 5; k++) ms5[k] = g_mrmr_ms[k];
}

int mrmr_select(int device, const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p,
                int n_states, int unit, int method, int64_t k, double* relevance,
                int64_t* selected, double* rows) {
  if (device_count() <= 0) return no_device();
  for (double& v : g_mrmr_ms) v = -1.0;
  MiPlanes pl;
  const int CPW = kPtThreads / (((n_states + 3) / 4) * ((n_states + 3) / 4));
  FS_TRY(pl.shape("fs_mrmr_select", n, p, n_states, CPW));
  if (rows && (double)k * (double)p * 8.0 > kMiMaxBytes) {
    set_error("fs_mrmr_select: the rows do not fit the device memory");
    return FS_EOOM;
  }
  FS_HIP(hipSetDevice(device));
  DevArena mem(device);
  StreamLease lease(device);  // destroyed (and the stream synchronised) before `mem`
  // timing: upload, pack, relevance, then (row, step) pairs; above
  // kMrTimedSteps steps the loop is timed as a whole
  const bool per_step = k - 1 <= kMrTimedSteps;
  const size_t nev = 4 + (per_step ? 2 * (size_t)(k - 1) + 1 : 1);
  FS_TRY(lease.open(nev));
  hipStream_t s = lease.s;
  std::vector<hipEvent_t>& ev = lease.ev;

  MrmrSteps st;
  st.s = s, st.p = p, st.k = k, st.method = method;
  double* drows = nullptr;
  // every block is allocated before any array is read
  FS_TRY(pl.alloc(mem, mem));
  FS_TRY(st.alloc(mem));
  if (rows) FS_TRY(mem.alloc(&drows, (size_t)k * p));

  FS_HIP(hipEventRecord(ev[0], s));
  FS_TRY(pl.upload(codes, ycodes, s));
  FS_TRY(st.reset());
  FS_HIP(hipEventRecord(ev[1], s));
  FS_TRY(pl.pack(s));
  FS_HIP(hipEventRecord(ev[2], s));

  MiRowArgs a;
  a.row.planes = pl.planes, a.row.kcol = pl.kcol, a.row.n = n, a.row.p = p, a.row.P1p = pl.P1p;
  a.row.W = pl.W, a.row.SP = pl.SP, a.row.NB = pl.NB, a.row.CPW = CPW, a.unit = unit;
  auto launch_row = [&](int64_t anchor, const int64_t* anchor_dev, double* out, double* rsum) {
    a.row.anchor = anchor, a.row.anchor_dev = anchor_dev, a.out = out, a.rsum = rsum;
    k_mi_row<<<(unsigned)(pl.P1p / CPW), kPtThreads, 0, s>>>(a);
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

  FS_TRY(pl.fetch_bad(s));
  FS_HIP(hipMemcpyAsync(selected, st.sel, (size_t)k * 8, hipMemcpyDeviceToHost, s));
  FS_HIP(hipMemcpyAsync(relevance, st.rel, (size_t)p * 8, hipMemcpyDeviceToHost, s));
  if (rows)
    FS_HIP(hipMemcpyAsync(rows, drows, (size_t)k * p * 8, hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  FS_TRY(pl.check());
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
  if ((double)p * (double)p * 8.0 > kMiMaxBytes) {
    set_error("fs_mrmr_search_matrix: the matrix does not fit the device memory");
    return FS_EOOM;
  }
  FS_HIP(hipSetDevice(device));
  DevArena mem(device);
  StreamLease lease(device);  // destroyed (and the stream synchronised) before `mem`
  FS_TRY(lease.open(0));
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
