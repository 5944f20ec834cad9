// fs_cfs.hip -- the GPU backend of fs_cfs_*: correlation-based feature
// selection with rows of symmetrical uncertainty computed when the best-first
// search selects their feature (replaces _cu_entropy,
// _cu_symmetrical_uncertainty and _precompute_correlations_gpu_kernel,
// CFS.py:165-243, and runs _best_first_search, CFS.py:115-162, on the device).
//
//   k_mi_pack      (fs_mi.hip) the codes -> word-major state bit-planes
//                  planes[(w * P1p + c) * SP + s]; the columns are padded to a
//                  whole number of k_cfs_row workgroups, y is column p.
//   k_cfs_entropy  one lane per column: its marginal counts by popcount and
//                  its entropy (fs_cfs.h cfs_entropy), once per handle.
//   k_cfs_row      one anchor column (a feature, or y for r_cf) against
//                  kCfsThreads / NB^2 columns per workgroup (NB = SP / 4):
//                  256 columns up to 4 states, 64 up to 8, 28 up to 12, ...,
//                  4 at 32.  Each group of NB^2 lanes owns one pair and each
//                  lane one 4 x 4 block of its table in 16 registers, as in
//                  k_mi_scan.  The anchor's planes are staged in LDS per chunk
//                  of kCfsWC words; a column's planes come straight from HBM,
//                  consecutive lanes reading consecutive 16-byte vectors of
//                  one word.  The epilogue runs in the same kernel in
//                  fs_cfs.h's order, over the transposed indices when the
//                  anchor has the higher index (the column with the lower
//                  index supplies the rows), and writes one float32 per pair.
//                  No table reaches HBM.  The anchor may be read from device
//                  memory, so that the row of a step's winner is queued behind
//                  the step without a round trip to the host.
//   k_cfs_step     one lane per candidate: its merit from k coalesced reads
//                  down the selected features' rows (fs_cfs.h
//                  cfs_candidate_merit), then the workgroup's best (merit,
//                  index) by cfs_beats in a fixed tree.
//   k_cfs_pick     one workgroup: the best of the workgroups' results, the
//                  verdict against the current merit, and the bookkeeping of
//                  an accepted feature (taken, selected, rowof) on the device.
//   k_cfs_entries  the new row's entries at the selected positions, behind
//                  the verdict in one buffer: one download and one
//                  synchronisation per step.
// No float atomics: two fits of the same data give identical bits.
#include "fs_gpu_internal.h"
#include "fs_cfs.h"

#include <memory>
#include <unordered_map>

namespace fs {
namespace gpu {

namespace {

constexpr int kCfsThreads = 256;
constexpr int kCfsWC = 64;        // words (2048 samples) of the anchor staged per chunk
constexpr int kCfsPx = 4096;      // most cells of a workgroup's tables: CPW * SP^2
constexpr int kCfsMarg = 1024;    // most marginals of a workgroup: CPW * SP
constexpr int64_t kCfsRowsCap = 16;  // rows the cache holds at first

thread_local double g_cfs_ms[5] = {-1.0, -1.0, -1.0, -1.0, -1.0};

// One lane per column (y included): entropy from the marginal counts.
__global__ __launch_bounds__(256) void k_cfs_entropy(const uint32_t* __restrict__ planes,
                                                     int64_t n, int64_t P1, int64_t P1p, int64_t W,
                                                     int SP, double* __restrict__ hcol) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= P1) return;
  const double dn = (double)n;
  double h = 0.0;
  for (int blk = 0; blk < SP / 4; blk++) {
    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int64_t w = 0; w < W; w++) {
      const uint4 v =
          *reinterpret_cast<const uint4*>(planes + ((size_t)w * P1p + c) * SP + 4 * blk);
      c0 += __builtin_popcount(v.x);
      c1 += __builtin_popcount(v.y);
      c2 += __builtin_popcount(v.z);
      c3 += __builtin_popcount(v.w);
    }
    h -= cfs_h_term(cfs_pxy((int32_t)c0, dn));
    h -= cfs_h_term(cfs_pxy((int32_t)c1, dn));
    h -= cfs_h_term(cfs_pxy((int32_t)c2, dn));
    h -= cfs_h_term(cfs_pxy((int32_t)c3, dn));
  }
  hcol[c] = h;
}

struct CfsRowArgs {
  const uint32_t* planes;
  const int32_t* kcol;        // P1 state counts
  const double* hcol;         // P1 entropies
  int64_t n, p, P1p, W;
  int SP, NB, CPW;            // CPW: columns per workgroup
  int64_t anchor;             // the anchor column (p: the target) ...
  const int64_t* anchor_dev;  // ... or where to read it (negative: nothing to do)
  float* out;                 // p values
};

__global__ __launch_bounds__(kCfsThreads) void k_cfs_row(const CfsRowArgs a) {
  __shared__ __align__(16) uint32_t s_anc[kCfsWC * kMiMaxStatesGpu];
  __shared__ double s_px[kCfsPx];  // [pair][SP][SP]: pxy, then the terms
  __shared__ double s_p1[kCfsMarg];
  __shared__ double s_p2[kCfsMarg];
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
  for (int64_t w0 = 0; w0 < a.W; w0 += kCfsWC) {
    const int wn = a.W - w0 < kCfsWC ? (int)(a.W - w0) : kCfsWC;
    for (int v = tid; v < wn * NB; v += kCfsThreads) {
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

  // epilogue (fs_cfs.h).  cnt[r * 4 + k] counts (anchor state 4 ab + r, column
  // state 4 bb + k); the column with the lower index supplies the table's rows
  const bool swap = anc > c;
  const double dn = (double)a.n;
  const int tq = q * SP * SP;
  double px[16];
#pragma unroll
  for (int k = 0; k < 16; k++) px[k] = cfs_pxy((int32_t)cnt[k], dn);
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
  for (int it = tid; it < CPW * SP; it += kCfsThreads) {
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
            cfs_mi_term(px[r * 4 + k], s_p1[q * SP + row], s_p2[q * SP + col]);
      }
  }
  __syncthreads();
  if (pair_on && blk == 0) {
    const int64_t lo = swap ? c : anc, hi = swap ? anc : c;
    const int k1 = a.kcol[lo], k2 = a.kcol[hi];
    const double* t = s_px + tq;
    double mi = 0.0;
    for (int r = 0; r < k1; r++)
      for (int k = 0; k < k2; k++) mi += t[r * SP + k];
    a.out[c] = c == anc ? 0.0f : cfs_su(mi, a.hcol[lo], a.hcol[hi]);
  }
}

// The verdict of a step, followed in the same buffer by the float32 entries
// of the accepted feature's row at the selected positions.
struct CfsRes {
  int64_t best_i;  // -1: no candidate improves the merit
  double merit;
};

struct CfsStepArgs {
  const float* r_cf;
  const float* rows;
  const int64_t* rowof;
  const uint8_t* taken;
  int64_t p, stride, k;
  double base_cf, base_ff, min_r_cf, current;
  double* pm;    // per workgroup: the best merit ...
  int64_t* pi;   // ... and its index (-1: none above current)
};

__device__ __forceinline__ void cfs_block_best(double& m, int64_t& bi, double* sm, int64_t* si) {
  const int tid = threadIdx.x;
  sm[tid] = m;
  si[tid] = bi;
  __syncthreads();
  for (int s = kCfsThreads / 2; s > 0; s >>= 1) {
    if (tid < s && cfs_beats(sm[tid + s], si[tid + s], sm[tid], si[tid])) {
      sm[tid] = sm[tid + s];
      si[tid] = si[tid + s];
    }
    __syncthreads();
  }
  m = sm[0];
  bi = si[0];
}

__global__ __launch_bounds__(kCfsThreads) void k_cfs_step(const CfsStepArgs a) {
  __shared__ double sm[kCfsThreads];
  __shared__ int64_t si[kCfsThreads];
  const int64_t i = (int64_t)blockIdx.x * kCfsThreads + threadIdx.x;
  double m = a.current;
  int64_t bi = -1;
  if (i < a.p && cfs_is_candidate(a.taken, a.r_cf, a.min_r_cf, i)) {
    const double v =
        cfs_candidate_merit(a.base_cf, a.base_ff, a.r_cf, a.rows, a.rowof, a.stride, a.k, i);
    if (cfs_beats(v, i, m, bi)) m = v, bi = i;
  }
  cfs_block_best(m, bi, sm, si);
  if (threadIdx.x == 0) {
    a.pm[blockIdx.x] = m;
    a.pi[blockIdx.x] = bi;
  }
}

__global__ __launch_bounds__(kCfsThreads) void k_cfs_pick(const double* __restrict__ pm,
                                                          const int64_t* __restrict__ pi,
                                                          int64_t nblk, double current, int64_t k,
                                                          int matrix, uint8_t* taken, int64_t* sel,
                                                          int64_t* rowof, CfsRes* res) {
  __shared__ double sm[kCfsThreads];
  __shared__ int64_t si[kCfsThreads];
  double m = current;
  int64_t bi = -1;
  for (int64_t b = threadIdx.x; b < nblk; b += kCfsThreads)
    if (cfs_beats(pm[b], pi[b], m, bi)) m = pm[b], bi = pi[b];
  cfs_block_best(m, bi, sm, si);
  if (threadIdx.x == 0) {
    res->best_i = bi;
    res->merit = m;
    if (bi >= 0) {
      taken[bi] = 1;
      sel[k] = bi;
      rowof[k] = matrix ? bi : k;  // a caller's matrix: the feature's own row
    }
  }
}

__global__ __launch_bounds__(256) void k_cfs_entries(const CfsRes* __restrict__ res,
                                                     const float* __restrict__ rows,
                                                     const int64_t* __restrict__ rowof,
                                                     const int64_t* __restrict__ sel,
                                                     int64_t stride, int64_t k,
                                                     float* __restrict__ ent) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= k || res->best_i < 0) return;
  ent[s] = rows[rowof[k] * stride + sel[s]];
}

__global__ void k_cfs_begin(uint8_t* taken, int64_t* sel, int64_t* rowof, int64_t first,
                            int64_t row0) {
  taken[first] = 1;
  sel[0] = first;
  rowof[0] = row0;
}

// The device side of one search, over the handle's row cache or a caller's
// matrix.
struct CfsGpu;
struct GpuStepper : CfsStepper {
  int device = 0;
  hipStream_t s = nullptr;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  int64_t p = 0, stride = 0, nblk = 0;
  double min_r_cf = 0.0;
  int matrix = 0;
  const float* r_cf = nullptr;
  const float* rows = nullptr;   // the matrix; with an owner: its cache
  uint8_t* taken = nullptr;
  int64_t *sel = nullptr, *rowof = nullptr, *pi = nullptr;
  double* pm = nullptr;
  char* res = nullptr;           // CfsRes, then p floats
  CfsGpu* owner = nullptr;
  std::vector<char> hres;
  int begin(int64_t first) override;
  int step(int64_t k, double base_cf, double base_ff, double current, int64_t* best_i,
           double* best_merit, float* entries) override;
};

struct CfsGpu : fs_cfs {
  explicit CfsGpu(int dev) : device(dev) {}
  const int device;
  int S = 0, SP = 0, NB = 0, CPW = 0;
  int64_t P1p = 0, W = 0, nblk = 0;
  hipStream_t s = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  // device buffers (mem: as long as the handle; mem_up: until the pack is done)
  uint32_t* planes = nullptr;
  int32_t* kcol = nullptr;
  double* hcol = nullptr;
  float *d_rcf = nullptr, *scratch = nullptr;
  uint8_t* taken = nullptr;
  int64_t *sel = nullptr, *rowof = nullptr, *pi = nullptr;
  double* pm = nullptr;
  char* res = nullptr;
  int* dbad = nullptr;
  DevArena mem{device}, mem_up{device};
  DevBuf<float> rows{device};  // the row cache [cap][p], in selection order
  int64_t rows_cap = 0;
  std::vector<float> r_cf;
  std::unordered_map<int64_t, int64_t> slot;  // feature -> row of the cache

  ~CfsGpu() override {
    (void)hipSetDevice(device);
    if (s) {
      (void)hipStreamSynchronize(s);
      stream_put(device, s);
    }
    for (hipEvent_t e : ev)
      if (e) event_put(device, e, true);
    (void)hipGetLastError();
  }

  int launch_row(int64_t anchor, const int64_t* anchor_dev, float* out) {
    CfsRowArgs a;
    a.planes = planes, a.kcol = kcol, a.hcol = hcol, a.n = n, a.p = p, a.P1p = P1p, a.W = W;
    a.SP = SP, a.NB = NB, a.CPW = CPW, a.anchor = anchor, a.anchor_dev = anchor_dev, a.out = out;
    k_cfs_row<<<(unsigned)(P1p / CPW), kCfsThreads, 0, s>>>(a);
    return launch_check("k_cfs_row");
  }
  // room for row k of the cache; the rows below it are kept
  int ensure_row(int64_t k) {
    if (k < rows_cap) return FS_OK;
    const int64_t cap = std::min<int64_t>(p, std::max<int64_t>(2 * rows_cap, k + 1));
    DevBuf<float> grown(device);
    FS_TRY(grown.reserve((size_t)cap * p, 0, nullptr, 0));
    FS_HIP(hipMemcpyAsync(grown.p, rows.p, (size_t)k * p * sizeof(float),
                          hipMemcpyDeviceToDevice, s));
    FS_HIP(hipStreamSynchronize(s));
    std::swap(grown.p, rows.p);
    std::swap(grown.cap, rows.cap);
    rows_cap = cap;
    return FS_OK;  // `grown` frees the old block
  }
  void add_ms(int which, hipEvent_t e0, hipEvent_t e1) {
    float ms = 0.0f;
    if (g_cfs_ms[which] >= 0.0 && hipEventElapsedTime(&ms, e0, e1) == hipSuccess)
      g_cfs_ms[which] += ms;
  }

  int init(const uint8_t* codes, const uint8_t* ycodes);
  int relevance(float* out) override {
    std::memcpy(out, r_cf.data(), (size_t)p * sizeof(float));
    return FS_OK;
  }
  int row(int64_t feature, float* out) override {
    FS_HIP(hipSetDevice(device));
    auto it = slot.find(feature);
    const float* src = scratch;
    if (it != slot.end()) {
      src = rows.p + (size_t)it->second * p;
    } else {
      FS_HIP(hipEventRecord(ev[0], s));
      FS_TRY(launch_row(feature, nullptr, scratch));
      FS_HIP(hipEventRecord(ev[1], s));
    }
    FS_HIP(hipMemcpyAsync(out, src, (size_t)p * sizeof(float), hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    if (it == slot.end()) add_ms(3, ev[0], ev[1]);
    return FS_OK;
  }
  int search(double min_r_cf, int64_t* selected, int64_t* n_selected, double* merits) override {
    FS_HIP(hipSetDevice(device));
    slot.clear();
    FS_HIP(hipMemsetAsync(taken, 0, (size_t)p, s));
    GpuStepper st;
    st.device = device, st.s = s, st.p = p, st.stride = p, st.nblk = nblk;
    st.ev[0] = ev[0], st.ev[1] = ev[1], st.ev[2] = ev[2];
    st.min_r_cf = min_r_cf, st.matrix = 0, st.r_cf = d_rcf, st.taken = taken, st.sel = sel;
    st.rowof = rowof, st.pi = pi, st.pm = pm, st.res = res, st.owner = this;
    const int rc = cfs_search_drive(st, r_cf.data(), p, min_r_cf, selected, n_selected, merits);
    if (rc != FS_OK) {
      (void)hipStreamSynchronize(s);
      (void)hipGetLastError();
      return rc;
    }
    for (int64_t k = 0; k < *n_selected; k++) slot[selected[k]] = k;
    return FS_OK;
  }
};

int GpuStepper::begin(int64_t first) {
  k_cfs_begin<<<1, 1, 0, s>>>(taken, sel, rowof, first, matrix ? first : 0);
  FS_TRY(launch_check("k_cfs_begin"));
  if (!owner) return FS_OK;
  FS_TRY(owner->ensure_row(0));
  FS_HIP(hipEventRecord(ev[0], s));
  FS_TRY(owner->launch_row(first, nullptr, owner->rows.p));
  FS_HIP(hipEventRecord(ev[1], s));
  FS_HIP(hipStreamSynchronize(s));
  owner->add_ms(3, ev[0], ev[1]);
  return FS_OK;
}

int GpuStepper::step(int64_t k, double base_cf, double base_ff, double current, int64_t* best_i,
                     double* best_merit, float* entries) {
  if (owner) {
    FS_TRY(owner->ensure_row(k));
    rows = owner->rows.p;
  }
  CfsRes* dres = reinterpret_cast<CfsRes*>(res);
  float* dent = reinterpret_cast<float*>(res + sizeof(CfsRes));
  CfsStepArgs a;
  a.r_cf = r_cf, a.rows = rows, a.rowof = rowof, a.taken = taken, a.p = p, a.stride = stride;
  a.k = k, a.base_cf = base_cf, a.base_ff = base_ff, a.min_r_cf = min_r_cf, a.current = current;
  a.pm = pm, a.pi = pi;
  FS_HIP(hipEventRecord(ev[0], s));
  k_cfs_step<<<(unsigned)nblk, kCfsThreads, 0, s>>>(a);
  FS_TRY(launch_check("k_cfs_step"));
  k_cfs_pick<<<1, kCfsThreads, 0, s>>>(pm, pi, nblk, current, k, matrix, taken, sel, rowof, dres);
  FS_TRY(launch_check("k_cfs_pick"));
  FS_HIP(hipEventRecord(ev[1], s));
  // the winner's row, queued behind the verdict (a negative winner: no work)
  if (owner) FS_TRY(owner->launch_row(-1, &dres->best_i, owner->rows.p + (size_t)k * p));
  k_cfs_entries<<<(unsigned)((k + 255) / 256), 256, 0, s>>>(dres, rows, rowof, sel, stride, k,
                                                            dent);
  FS_TRY(launch_check("k_cfs_entries"));
  FS_HIP(hipEventRecord(ev[2], s));
  const size_t bytes = sizeof(CfsRes) + (size_t)k * sizeof(float);
  hres.resize(bytes);
  FS_HIP(hipMemcpyAsync(hres.data(), res, bytes, hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  if (owner) {
    owner->add_ms(4, ev[0], ev[1]);
    owner->add_ms(3, ev[1], ev[2]);
  }
  CfsRes r;
  std::memcpy(&r, hres.data(), sizeof(CfsRes));
  *best_i = r.best_i;
  *best_merit = r.merit;
  if (r.best_i >= 0) std::memcpy(entries, hres.data() + sizeof(CfsRes), (size_t)k * sizeof(float));
  return FS_OK;
}

int CfsGpu::init(const uint8_t* codes, const uint8_t* ycodes) {
  const int64_t P1 = p + 1;
  NB = (S + 3) / 4, SP = NB * 4, CPW = kCfsThreads / (NB * NB);
  P1p = (P1 + CPW - 1) / CPW * CPW;
  W = (n + 31) / 32;
  nblk = (p + kCfsThreads - 1) / kCfsThreads;
  // sizes in floating point first: a request beyond any device is an
  // out-of-memory answer, not an overflowed size
  const double kMaxBytes = 1e15;
  if ((double)W * (double)P1p * SP * 4.0 > kMaxBytes || (double)n * (double)p > kMaxBytes) {
    set_error("fs_cfs_create: the bit-planes do not fit the device memory");
    return FS_EOOM;
  }
  rows_cap = test_hooks().cfs_rows_cap > 0 ? test_hooks().cfs_rows_cap : kCfsRowsCap;
  rows_cap = std::min<int64_t>(rows_cap, p);
  try {
    r_cf.resize((size_t)p);
  } catch (const std::bad_alloc&) {
    set_error("fs_cfs_create: out of host memory");
    return FS_EOOM;
  }
  FS_HIP(hipSetDevice(device));
  s = stream_get(device);
  for (hipEvent_t& e : ev) e = event_get(device, true);
  uint8_t *dx = nullptr, *dy = nullptr;
  // every block is allocated before any array is read
  FS_TRY(mem_up.alloc(&dx, (size_t)n * p));
  FS_TRY(mem_up.alloc(&dy, (size_t)n));
  FS_TRY(mem.alloc(&planes, (size_t)W * P1p * SP));
  FS_TRY(mem.alloc(&kcol, (size_t)P1));
  FS_TRY(mem.alloc(&hcol, (size_t)P1));
  FS_TRY(mem.alloc(&d_rcf, (size_t)p));
  FS_TRY(mem.alloc(&scratch, (size_t)p));
  FS_TRY(mem.alloc(&taken, (size_t)p));
  FS_TRY(mem.alloc(&sel, (size_t)p));
  FS_TRY(mem.alloc(&rowof, (size_t)p));
  FS_TRY(mem.alloc(&pm, (size_t)nblk));
  FS_TRY(mem.alloc(&pi, (size_t)nblk));
  FS_TRY(mem.alloc(&res, sizeof(CfsRes) + (size_t)p * sizeof(float)));
  FS_TRY(mem.alloc(&dbad, 1));
  FS_TRY(rows.reserve((size_t)rows_cap * p, 0, nullptr, 0));

  FS_HIP(hipEventRecord(ev[0], s));
  FS_HIP(hipMemcpyAsync(dx, codes, (size_t)n * p, hipMemcpyHostToDevice, s));
  FS_HIP(hipMemcpyAsync(dy, ycodes, (size_t)n, hipMemcpyHostToDevice, s));
  FS_HIP(hipMemsetAsync(dbad, 0, 4, s));
  FS_HIP(hipMemsetAsync(kcol, 0, (size_t)P1 * 4, s));
  FS_HIP(hipEventRecord(ev[1], s));
  FS_HIP(mi_pack(dx, dy, n, p, P1p, S, SP, planes, kcol, dbad, s));
  k_cfs_entropy<<<(unsigned)((P1 + 255) / 256), 256, 0, s>>>(planes, n, P1, P1p, W, SP, hcol);
  FS_TRY(launch_check("k_cfs_entropy"));
  FS_HIP(hipEventRecord(ev[2], s));
  int bad = 0;
  FS_HIP(hipMemcpyAsync(&bad, dbad, 4, hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  mem_up.release();
  if (bad) {
    set_error("fs_cfs_create: a code is >= n_states");
    return FS_EINVAL;
  }
  FS_TRY(launch_row(p, nullptr, d_rcf));  // the target is column p
  FS_HIP(hipEventRecord(ev[3], s));
  FS_HIP(hipMemcpyAsync(r_cf.data(), d_rcf, (size_t)p * sizeof(float), hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  for (int k = 0; k < 3; k++) {
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess) g_cfs_ms[k] = ms;
  }
  g_cfs_ms[3] = g_cfs_ms[4] = 0.0;
  return FS_OK;
}

}  // namespace

void cfs_last_timing(double* ms5) {
  for (int k = 0; k < 5; k++) ms5[k] = g_cfs_ms[k];
}

int cfs_create(fs_cfs** out, int device, const uint8_t* codes, const uint8_t* ycodes, int64_t n,
               int64_t p, int n_states) {
  if (device_count() <= 0) {
    set_error("backend='gpu' requested but no HIP device is visible");
    return FS_ENODEV;
  }
  for (double& v : g_cfs_ms) v = -1.0;
  std::unique_ptr<CfsGpu> h(new (std::nothrow) CfsGpu(device));
  if (!h) {
    set_error("fs_cfs_create: out of host memory");
    return FS_EOOM;
  }
  h->n = n, h->p = p, h->S = n_states;
  const int rc = h->init(codes, ycodes);
  if (rc != FS_OK) return rc;  // ~CfsGpu synchronises the stream, then the blocks go
  *out = h.release();
  return FS_OK;
}

int cfs_search_matrix(int device, const float* r_cf, const float* r_ff, int64_t p,
                      double min_r_cf, int64_t* selected, int64_t* n_selected, double* merits) {
  if (device_count() <= 0) {
    set_error("backend='gpu' requested but no HIP device is visible");
    return FS_ENODEV;
  }
  if ((double)p * (double)p * 4.0 > 1e15) {
    set_error("fs_cfs_search_matrix: the matrix does not fit the device memory");
    return FS_EOOM;
  }
  FS_HIP(hipSetDevice(device));
  GpuStepper st;
  st.device = device, st.p = p, st.stride = p, st.matrix = 1, st.min_r_cf = min_r_cf;
  st.nblk = (p + kCfsThreads - 1) / kCfsThreads;
  st.s = stream_get(device);
  for (hipEvent_t& e : st.ev) e = event_get(device, true);
  DevArena mem(device);
  float *d_rcf = nullptr, *d_rff = nullptr;
  int rc = FS_OK;
  auto run = [&]() -> int {
    FS_TRY(mem.alloc(&d_rcf, (size_t)p));
    FS_TRY(mem.alloc(&d_rff, (size_t)p * p));
    FS_TRY(mem.alloc(&st.taken, (size_t)p));
    FS_TRY(mem.alloc(&st.sel, (size_t)p));
    FS_TRY(mem.alloc(&st.rowof, (size_t)p));
    FS_TRY(mem.alloc(&st.pm, (size_t)st.nblk));
    FS_TRY(mem.alloc(&st.pi, (size_t)st.nblk));
    FS_TRY(mem.alloc(&st.res, sizeof(CfsRes) + (size_t)p * sizeof(float)));
    st.r_cf = d_rcf, st.rows = d_rff;
    FS_HIP(hipMemcpyAsync(d_rcf, r_cf, (size_t)p * 4, hipMemcpyHostToDevice, st.s));
    FS_HIP(hipMemcpyAsync(d_rff, r_ff, (size_t)p * p * 4, hipMemcpyHostToDevice, st.s));
    FS_HIP(hipMemsetAsync(st.taken, 0, (size_t)p, st.s));
    return cfs_search_drive(st, r_cf, p, min_r_cf, selected, n_selected, merits);
  };
  rc = run();
  (void)hipStreamSynchronize(st.s);  // before `mem` frees its blocks
  (void)hipGetLastError();
  for (hipEvent_t e : st.ev) event_put(device, e, true);
  stream_put(device, st.s);
  return rc;
}

}  // namespace gpu
}  // namespace fs
