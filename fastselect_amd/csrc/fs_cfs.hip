// fs_cfs.hip -- the GPU backend of fs_cfs_*: correlation-based feature
// selection with rows of symmetrical uncertainty computed when the best-first
// search selects their feature (replaces _cu_entropy,
// _cu_symmetrical_uncertainty and _precompute_correlations_gpu_kernel,
// CFS.py:165-243, and runs _best_first_search, CFS.py:115-162, on the device).
//
//   k_mi_pack      (fs_mi.hip, through MiPlanes) the codes -> word-major state
//                  bit-planes planes[(w * P1p + c) * SP + s]; the columns are
//                  padded to a whole number of k_cfs_row workgroups, y is
//                  column p.
//   k_cfs_entropy  one lane per column: its marginal counts by popcount and
//                  its entropy (fs_cfs.h cfs_entropy), once per handle.
//   k_cfs_row      one anchor column (a feature, or y for r_cf) against
//                  kPtThreads / NB^2 columns per workgroup (NB = SP / 4):
//                  256 columns up to 4 states, 64 up to 8, 28 up to 12, ...,
//                  4 at 32.  Each group of NB^2 lanes owns one pair and each
//                  lane one 4 x 4 block of its table in 16 registers.  The
//                  scan and the epilogue are pt_row's (fs_pairtab.h, shared
//                  with k_mi_row): the
//                  anchor's planes are staged in LDS per chunk of kPtWC words;
//                  a column's planes come straight from HBM, consecutive lanes
//                  reading consecutive 16-byte vectors of one word.  The
//                  epilogue runs in the same kernel in fs_cfs.h's order
//                  (CfsTerms), over the transposed indices when the anchor has
//                  the higher index (the column with the lower index supplies
//                  the rows); the pair's first lane writes one float32 here.
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
#include "fs_pairtab.h"

#include <memory>
#include <unordered_map>

namespace fs {
namespace gpu {

namespace {

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

struct CfsTerms {
  static __device__ __forceinline__ double pxy(int32_t count, double dn) {
    return cfs_pxy(count, dn);
  }
  static __device__ __forceinline__ double term(double pxy, double px, double py) {
    return cfs_mi_term(pxy, px, py);
  }
};

struct CfsRowArgs {
  PtRowArgs row;
  const double* hcol;  // P1 entropies
  float* out;          // p values
};

// The scan and the epilogue are pt_row's (fs_pairtab.h); the pair's first lane
// turns the sum into the float32 SU here.
__global__ __launch_bounds__(kPtThreads) void k_cfs_row(const CfsRowArgs a) {
  int64_t c;
  PtPair r;
  if (!pt_row<CfsTerms, false>(a.row, c, r)) return;
  a.out[c] = r.lo == r.hi ? 0.0f : cfs_su(r.sum, a.hcol[r.lo], a.hcol[r.hi]);
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

__global__ __launch_bounds__(kPtThreads) void k_cfs_step(const CfsStepArgs a) {
  __shared__ double sm[kPtThreads];
  __shared__ int64_t si[kPtThreads];
  const int64_t i = (int64_t)blockIdx.x * kPtThreads + threadIdx.x;
  double m = a.current;
  int64_t bi = -1;
  if (i < a.p && cfs_is_candidate(a.taken, a.r_cf, a.min_r_cf, i)) {
    const double v =
        cfs_candidate_merit(a.base_cf, a.base_ff, a.r_cf, a.rows, a.rowof, a.stride, a.k, i);
    if (cfs_beats(v, i, m, bi)) m = v, bi = i;
  }
  pt_block_best<cfs_beats>(m, bi, sm, si);
  if (threadIdx.x == 0) {
    a.pm[blockIdx.x] = m;
    a.pi[blockIdx.x] = bi;
  }
}

__global__ __launch_bounds__(kPtThreads) void k_cfs_pick(const double* __restrict__ pm,
                                                          const int64_t* __restrict__ pi,
                                                          int64_t nblk, double current, int64_t k,
                                                          int matrix, uint8_t* taken, int64_t* sel,
                                                          int64_t* rowof, CfsRes* res) {
  __shared__ double sm[kPtThreads];
  __shared__ int64_t si[kPtThreads];
  double m = current;
  int64_t bi = -1;
  for (int64_t b = threadIdx.x; b < nblk; b += kPtThreads)
    if (cfs_beats(pm[b], pi[b], m, bi)) m = pm[b], bi = pi[b];
  pt_block_best<cfs_beats>(m, bi, sm, si);
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
  int S = 0;
  int64_t nblk = 0;
  MiPlanes pl;                // the packed planes and their geometry
  CfsRowArgs row_args{};      // k_cfs_row's, but for the anchor and `out`
  hipStream_t s = nullptr;    // lease.s
  // device buffers (mem: as long as the handle; mem_up: until the pack is done)
  double* hcol = nullptr;
  float *d_rcf = nullptr, *scratch = nullptr;
  uint8_t* taken = nullptr;
  int64_t *sel = nullptr, *rowof = nullptr, *pi = nullptr;
  double* pm = nullptr;
  char* res = nullptr;
  DevArena mem{device}, mem_up{device};
  DevBuf<float> rows{device};  // the row cache [cap][p], in selection order
  int64_t rows_cap = 0;
  std::vector<float> r_cf;
  std::unordered_map<int64_t, int64_t> slot;  // feature -> row of the cache
  // declared after the arenas and the cache: destroyed first, so the stream
  // is synchronised before any block is freed
  StreamLease lease{device};

  ~CfsGpu() override { (void)hipSetDevice(device); }  // then the members, `lease` first

  int launch_row(int64_t anchor, const int64_t* anchor_dev, float* out) {
    CfsRowArgs a = row_args;
    a.row.anchor = anchor, a.row.anchor_dev = anchor_dev, a.out = out;
    k_cfs_row<<<(unsigned)(pl.P1p / a.row.CPW), kPtThreads, 0, s>>>(a);
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
      FS_HIP(hipEventRecord(lease.ev[0], s));
      FS_TRY(launch_row(feature, nullptr, scratch));
      FS_HIP(hipEventRecord(lease.ev[1], s));
    }
    FS_HIP(hipMemcpyAsync(out, src, (size_t)p * sizeof(float), hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    if (it == slot.end()) add_ms(3, lease.ev[0], lease.ev[1]);
    return FS_OK;
  }
  int search(double min_r_cf, int64_t* selected, int64_t* n_selected, double* merits) override {
    FS_HIP(hipSetDevice(device));
    slot.clear();
    FS_HIP(hipMemsetAsync(taken, 0, (size_t)p, s));
    GpuStepper st;
    st.device = device, st.s = s, st.p = p, st.stride = p, st.nblk = nblk;
    st.ev[0] = lease.ev[0], st.ev[1] = lease.ev[1], st.ev[2] = lease.ev[2];
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
  k_cfs_step<<<(unsigned)nblk, kPtThreads, 0, s>>>(a);
  FS_TRY(launch_check("k_cfs_step"));
  k_cfs_pick<<<1, kPtThreads, 0, s>>>(pm, pi, nblk, current, k, matrix, taken, sel, rowof, dres);
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
  const int CPW = kPtThreads / (((S + 3) / 4) * ((S + 3) / 4));
  FS_TRY(pl.shape("fs_cfs_create", n, p, S, CPW));
  nblk = (p + kPtThreads - 1) / kPtThreads;
  rows_cap = test_hooks().cfs_rows_cap > 0 ? test_hooks().cfs_rows_cap : kCfsRowsCap;
  rows_cap = std::min<int64_t>(rows_cap, p);
  try {
    r_cf.resize((size_t)p);
  } catch (const std::bad_alloc&) {
    set_error("fs_cfs_create: out of host memory");
    return FS_EOOM;
  }
  FS_HIP(hipSetDevice(device));
  FS_TRY(lease.open(4));
  s = lease.s;
  std::vector<hipEvent_t>& ev = lease.ev;
  const int64_t P1 = pl.P1;
  // every block is allocated before any array is read
  FS_TRY(pl.alloc(mem, mem_up));
  FS_TRY(mem.alloc(&hcol, (size_t)P1));
  FS_TRY(mem.alloc(&d_rcf, (size_t)p));
  FS_TRY(mem.alloc(&scratch, (size_t)p));
  FS_TRY(mem.alloc(&taken, (size_t)p));
  FS_TRY(mem.alloc(&sel, (size_t)p));
  FS_TRY(mem.alloc(&rowof, (size_t)p));
  FS_TRY(mem.alloc(&pm, (size_t)nblk));
  FS_TRY(mem.alloc(&pi, (size_t)nblk));
  FS_TRY(mem.alloc(&res, sizeof(CfsRes) + (size_t)p * sizeof(float)));
  FS_TRY(rows.reserve((size_t)rows_cap * p, 0, nullptr, 0));
  PtRowArgs& ra = row_args.row;
  ra.planes = pl.planes, ra.kcol = pl.kcol, ra.n = n, ra.p = p, ra.P1p = pl.P1p, ra.W = pl.W;
  ra.SP = pl.SP, ra.NB = pl.NB, ra.CPW = CPW;
  row_args.hcol = hcol;

  FS_HIP(hipEventRecord(ev[0], s));
  FS_TRY(pl.upload(codes, ycodes, s));
  FS_HIP(hipEventRecord(ev[1], s));
  FS_TRY(pl.pack(s));
  k_cfs_entropy<<<(unsigned)((P1 + 255) / 256), 256, 0, s>>>(pl.planes, n, P1, pl.P1p, pl.W,
                                                            pl.SP, hcol);
  FS_TRY(launch_check("k_cfs_entropy"));
  FS_HIP(hipEventRecord(ev[2], s));
  FS_TRY(pl.fetch_bad(s));
  FS_HIP(hipStreamSynchronize(s));
  mem_up.release();
  FS_TRY(pl.check());
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
  if (device_count() <= 0) return no_device();
  for (double& v : g_cfs_ms) v = -1.0;
  std::unique_ptr<CfsGpu> h(new (std::nothrow) CfsGpu(device));
  if (!h) {
    set_error("fs_cfs_create: out of host memory");
    return FS_EOOM;
  }
  h->n = n, h->p = p, h->S = n_states;
  const int rc = h->init(codes, ycodes);
  if (rc != FS_OK) return rc;  // the handle's lease synchronises the stream, then the blocks go
  *out = h.release();
  return FS_OK;
}

int cfs_search_matrix(int device, const float* r_cf, const float* r_ff, int64_t p,
                      double min_r_cf, int64_t* selected, int64_t* n_selected, double* merits) {
  if (device_count() <= 0) return no_device();
  if ((double)p * (double)p * 4.0 > kMiMaxBytes) {
    set_error("fs_cfs_search_matrix: the matrix does not fit the device memory");
    return FS_EOOM;
  }
  FS_HIP(hipSetDevice(device));
  DevArena mem(device);
  StreamLease lease(device);  // destroyed (and the stream synchronised) before `mem`
  FS_TRY(lease.open(3));
  GpuStepper st;
  st.device = device, st.p = p, st.stride = p, st.matrix = 1, st.min_r_cf = min_r_cf;
  st.nblk = (p + kPtThreads - 1) / kPtThreads;
  st.s = lease.s;
  for (int k = 0; k < 3; k++) st.ev[k] = lease.ev[k];
  float *d_rcf = nullptr, *d_rff = nullptr;
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
}

}  // namespace gpu
}  // namespace fs
