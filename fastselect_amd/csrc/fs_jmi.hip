// fs_jmi.hip -- the GPU backend of fs_jmi_*: JMI and CMIM selection on lazy
// rows of joint relevance J(f, s) = I(X_f, X_s; y) (fs_jmi.h).  The structure is
// fs_mrmr.hip's: the relevance, one row per selected feature, the greedy loop on
// the device, every launch of a fit on one stream and one synchronisation.
//
//   k_mi_pack    (fs_mi.hip, through MiPlanes) unchanged: word-major state
//                bit-planes planes[(w * P1p + c) * SP + s], y is column p.
//   k_jmi_rel    the relevance I(X_f; y): pt_row<MiTerms, true> with y as the
//                anchor and k_mi_scan's finish, the instantiation k_mi_row
//                (fs_mrmr.hip) makes; same expressions in the same order, so the
//                same bits as fs_mi_matrices and fs_mrmr_select.  A kernel of
//                this file's own so that fs_mrmr.hip is not touched.
//   k_jmi_row<C> one anchor column against kPtThreads / NB^2 columns per
//                workgroup (NB = SP / 4), C = kcol[y] in 2..4.  Per chunk of
//                kPtWC words the workgroup stages the anchor's planes ANDed with
//                each class plane of y: C masked copies in LDS.  A lane loads its
//                column's 16-byte vector once per word from HBM and counts it
//                against each copy with pt_count into cnt[C][16]: the column
//                planes are read once per row, not once per class.  The
//                epilogue runs mi_from_table's steps (fs_mi.h) on the table
//                T[(a, b)][c], (a, b) = (state of the lower-indexed column, of
//                the higher), in its order:
//                  p1[(a, b)]  the lane's own sum over c, in index order;
//                  p2[c]       the pair's first lane adds pxy row-major over
//                              (a, b), one table row a at a time through LDS;
//                  the terms   mi_term on the lane that counted the cell, the
//                              pair's first lane adding them row-major over
//                              ((a, b), c), again one table row at a time.
//                One table row of every pair of the workgroup is CPW * SP * C
//                doubles, at most 1024 C, and lies over the dead staging area
//                (8 KB per class either way), so the kernel holds 10 KB of LDS
//                per class whatever SP is and CPW does not shrink with C; the
//                whole three-way table (4096 C doubles) would not fit 64 KB.
//                The price is 4 SP barriers.  When the anchor has the higher
//                index the lanes write the transposed cells, as pt_epilogue
//                does.  The pair's first lane finishes the value (mi_constant,
//                mi_finish), stores it into the caller's row and applies
//                jmi_update to acc[c].  The anchor may be read from device
//                memory, so a row is queued behind the pick that chose it.
//   k_jmi_row_zero  a one-class y: every J is exactly 0.0 (mi_constant), no scan.
//   k_jmi_best   one lane per remaining feature: its score (fs_jmi.h), then the
//                workgroup's best (score, index) by jmi_beats in pt_block_best.
//   k_jmi_pick   one workgroup: the best of the workgroups' results;
//                taken[best] = 1 and sel[i] = best, the anchor word of the next
//                k_jmi_row.  Two kernels a step where mRMR has three: there is
//                no tie set around the maximum to resolve by a second key.
//   k_jmi_addrow (fs_jmi_search_matrix) applies the picked feature's row of the
//                caller's matrix where k_jmi_row would have computed it.
// No float atomics: two fits of the same data give identical bits.
#include <algorithm>

#include "fs_gpu_internal.h"
#include "fs_jmi.h"
#include "fs_pairtab.h"

namespace fs {
namespace gpu {

namespace {

constexpr int64_t kJmiTimedSteps = 64;  // steps timed one by one (two events each)
// Bytes per class of k_jmi_row's staging area, kPtWC words of kMiMaxStatesGpu
// planes, which is also CPW * SP doubles for every SP.
constexpr int kJmiClassBytes = kPtWC * kMiMaxStatesGpu * 4;
static_assert(kJmiClassBytes >= (kPtThreads * 4) * 8, "a table row of every pair must fit");

thread_local double g_jmi_ms[5] = {-1.0, -1.0, -1.0, -1.0, -1.0};

struct JmiRelArgs {
  PtRowArgs row;
  int unit;
  double* out;
};

__global__ __launch_bounds__(kPtThreads) void k_jmi_rel(const JmiRelArgs a) {
  int64_t c;
  PtPair r;
  if (!pt_row<MiTerms, true>(a.row, c, r)) return;
  a.out[c] = (r.lo == r.hi || mi_constant(r.used1, r.used2)) ? 0.0 : mi_finish(r.sum, a.unit);
}

struct JmiRowArgs {
  PtRowArgs row;
  int unit, method;
  const double* rel;  // p: rel[anchor] enters the CMIM update
  double* out;        // NULL, or p values
  double* acc;        // NULL, or p accumulators: acc[c] = jmi_update(...)
};

template <int C>
__global__ __launch_bounds__(kPtThreads) void k_jmi_row(const JmiRowArgs a) {
  // staging: [class][word][SP]; after the scan: one table row, [pair][SP][C]
  __shared__ __align__(16) unsigned char s_raw[C * kJmiClassBytes];
  __shared__ double s_p2[kPtThreads * C];  // [pair][C]
  const int tid = threadIdx.x;
  const int64_t anc = a.row.anchor_dev ? *a.row.anchor_dev : a.row.anchor;
  if (anc < 0) return;
  const int SP = a.row.SP, NB = a.row.NB, CPW = a.row.CPW;
  const int L = NB * NB;  // lanes per pair
  const int q = tid / L;
  const int blk = tid - q * L;
  const int ab = blk / NB, bb = blk - ab * NB;  // the anchor's / the column's block of 4 states
  const bool lane_on = q < CPW;
  const int64_t c = (int64_t)blockIdx.x * CPW + (lane_on ? q : 0);  // < P1p
  const bool pair_on = lane_on && c < a.row.p;
  const int64_t P1p = a.row.P1p;

  uint32_t cnt[C][16];
#pragma unroll
  for (int cls = 0; cls < C; cls++)
#pragma unroll
    for (int k = 0; k < 16; k++) cnt[cls][k] = 0;

  const uint4* g4 = reinterpret_cast<const uint4*>(a.row.planes);
  uint4* s4 = reinterpret_cast<uint4*>(s_raw);
  for (int64_t w0 = 0; w0 < a.row.W; w0 += kPtWC) {
    const int wn = a.row.W - w0 < kPtWC ? (int)(a.row.W - w0) : kPtWC;
    const int per = wn * NB;
    for (int v = tid; v < C * per; v += kPtThreads) {
      const int cls = v / per, rest = v - cls * per;
      const int w = rest / NB, xb = rest - w * NB;
      uint4 A = g4[((size_t)(w0 + w) * P1p + anc) * NB + xb];
      // y is column p: the plane of its class cls (C <= SP)
      const uint32_t m = a.row.planes[((size_t)(w0 + w) * P1p + a.row.p) * SP + cls];
      A.x &= m, A.y &= m, A.z &= m, A.w &= m;
      s4[(cls * kPtWC + w) * NB + xb] = A;
    }
    __syncthreads();
    if (pair_on) {
      const uint4* gc = g4 + ((size_t)w0 * P1p + c) * NB + bb;
      const size_t gstep = (size_t)P1p * NB;
      for (int w = 0; w < wn; w++) {
        const uint4 B = gc[(size_t)w * gstep];
#pragma unroll
        for (int cls = 0; cls < C; cls++) pt_count(s4[(cls * kPtWC + w) * NB + ab], B, cnt[cls]);
      }
    }
    __syncthreads();
  }

  // cnt[cls][r * 4 + k] counts (anchor state 4 ab + r, column state 4 bb + k,
  // class cls).  The column with the lower index supplies the high digit of
  // the joint state: with `swap` the column does.
  const bool swap = anc > c;
  const int64_t lo = swap ? c : anc, hi = swap ? anc : c;
  const int rblk = swap ? bb : ab, cblk = swap ? ab : bb;  // the lane's rows / columns of (a, b)
  const double dn = (double)a.row.n;
  double* s_row = reinterpret_cast<double*>(s_raw);
  const int sq = q * SP + 4 * cblk;  // the lane's first cell of a table row
  const bool first = pair_on && blk == 0;
  // a state count never exceeds SP on packed data; the bound keeps the loops
  // inside the row while a rejected call (a code >= n_states) drains
  int k_lo = 0, k_hi = 0;
  if (first) {
    k_lo = a.row.kcol[lo] < SP ? a.row.kcol[lo] : SP;
    k_hi = a.row.kcol[hi] < SP ? a.row.kcol[hi] : SP;
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
      if (lane_on && rblk == rb) {
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
          for (int cls = 0; cls < C; cls++)
            s_row[(sq + k) * C + cls] =
                mi_pxy((int32_t)(swap ? cnt[cls][k * 4 + r] : cnt[cls][r * 4 + k]), dn);
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
    // the counts as new values in every round: the compiler would otherwise
    // hoist every cell's pxy (and term) out of this loop into registers
#pragma unroll
    for (int cls = 0; cls < C; cls++)
#pragma unroll
      for (int k = 0; k < 16; k++) asm volatile("" : "+v"(cnt[cls][k]));
#pragma unroll
    for (int r = 0; r < 4; r++) {
      if (pair_on && rblk == rb) {
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
          for (int cls = 0; cls < C; cls++) {
            const uint32_t n3 = swap ? cnt[cls][k * 4 + r] : cnt[cls][r * 4 + k];
            const double pz = swap ? p1[k * 4 + r] : p1[r * 4 + k];
            s_row[(sq + k) * C + cls] = mi_term(mi_pxy((int32_t)n3, dn), pz, s_p2[q * C + cls]);
          }
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
  if (!first) return;
  const double j = (lo == hi || mi_constant(used1, used2)) ? 0.0 : mi_finish(sum, a.unit);
  if (a.out) a.out[c] = j;
  if (a.acc) a.acc[c] = jmi_update(a.method, a.acc[c], j, a.rel[anc]);
}

// A one-class y: J is exactly 0.0 everywhere.
__global__ __launch_bounds__(256) void k_jmi_row_zero(const JmiRowArgs a) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t anc = a.row.anchor_dev ? *a.row.anchor_dev : a.row.anchor;
  if (c >= a.row.p || anc < 0) return;
  if (a.out) a.out[c] = 0.0;
  if (a.acc) a.acc[c] = jmi_update(a.method, a.acc[c], 0.0, a.rel[anc]);
}

__global__ __launch_bounds__(256) void k_jmi_fill(double* __restrict__ v, int64_t p, double x) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c < p) v[c] = x;
}

// ---- one step of the greedy loop -------------------------------------------
struct JmiStepArgs {
  const double* rel;
  const double* acc;
  uint8_t* taken;
  int64_t p, nblk, i;  // i: the step (0: the first feature)
  double* ps;          // per workgroup: the best candidate's score ...
  int64_t* pi;         // ... and its index (-1: none)
  int64_t* sel;
};

__global__ __launch_bounds__(kPtThreads) void k_jmi_best(const JmiStepArgs a) {
  __shared__ double sm[kPtThreads];
  __shared__ int64_t si[kPtThreads];
  const int64_t f = (int64_t)blockIdx.x * kPtThreads + threadIdx.x;
  double s = 0.0;
  int64_t bi = -1;
  if (f < a.p && !a.taken[f]) {
    s = jmi_score(a.i, a.rel[f], a.acc[f]);
    bi = f;
  }
  pt_block_best<jmi_beats>(s, bi, sm, si);
  if (threadIdx.x == 0) {
    a.ps[blockIdx.x] = s;
    a.pi[blockIdx.x] = bi;
  }
}

__global__ __launch_bounds__(kPtThreads) void k_jmi_pick(const JmiStepArgs a) {
  __shared__ double sm[kPtThreads];
  __shared__ int64_t si[kPtThreads];
  double s = 0.0;
  int64_t bi = -1;
  for (int64_t b = threadIdx.x; b < a.nblk; b += kPtThreads)
    if (jmi_beats(a.ps[b], a.pi[b], s, bi)) s = a.ps[b], bi = a.pi[b];
  pt_block_best<jmi_beats>(s, bi, sm, si);
  if (threadIdx.x == 0 && bi >= 0) {
    a.taken[bi] = 1;
    a.sel[a.i] = bi;
  }
}

// acc[c] = jmi_update(acc[c], joint[*anchor][c], rel[*anchor]): the caller's
// matrix in the place of k_jmi_row.
__global__ __launch_bounds__(256) void k_jmi_addrow(const double* __restrict__ joint, int64_t p,
                                                    const int64_t* __restrict__ anchor,
                                                    const double* __restrict__ rel, int method,
                                                    double* __restrict__ acc) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t anc = *anchor;
  if (c >= p || anc < 0) return;
  acc[c] = jmi_update(method, acc[c], joint[(size_t)anc * p + c], rel[anc]);
}

// The buffers and launches of the greedy loop, over computed rows or a
// caller's matrix.
struct JmiSteps {
  hipStream_t s = nullptr;
  int64_t p = 0, k = 0, nblk = 0;
  int method = 0;
  double *rel = nullptr, *acc = nullptr, *ps = nullptr;
  int64_t *pi = nullptr, *sel = nullptr;
  uint8_t* taken = nullptr;

  int alloc(DevArena& mem) {
    nblk = (p + kPtThreads - 1) / kPtThreads;
    FS_TRY(mem.alloc(&rel, (size_t)p));
    FS_TRY(mem.alloc(&acc, (size_t)p));
    FS_TRY(mem.alloc(&taken, (size_t)p));
    FS_TRY(mem.alloc(&sel, (size_t)k));
    FS_TRY(mem.alloc(&ps, (size_t)nblk));
    FS_TRY(mem.alloc(&pi, (size_t)nblk));
    return FS_OK;
  }
  int reset() {
    k_jmi_fill<<<(unsigned)((p + 255) / 256), 256, 0, s>>>(acc, p, jmi_start(method));
    FS_TRY(launch_check("k_jmi_fill"));
    FS_HIP(hipMemsetAsync(taken, 0, (size_t)p, s));
    FS_HIP(hipMemsetAsync(sel, 0xff, (size_t)k * 8, s));  // -1: nothing picked yet
    return FS_OK;
  }
  int step(int64_t i) {
    JmiStepArgs a;
    a.rel = rel, a.acc = acc, a.taken = taken, a.p = p, a.nblk = nblk, a.i = i;
    a.ps = ps, a.pi = pi, a.sel = sel;
    k_jmi_best<<<(unsigned)nblk, kPtThreads, 0, s>>>(a);
    FS_TRY(launch_check("k_jmi_best"));
    k_jmi_pick<<<1, kPtThreads, 0, s>>>(a);
    return launch_check("k_jmi_pick");
  }
};

// The classes of y (max code + 1) from the host's copy: k_jmi_row's template
// parameter.  FS_EINVAL for a code >= n_states (what the pack would report)
// and beyond kJmiMaxClassesGpu.
int y_classes(const char* who, const uint8_t* ycodes, int64_t n, int n_states, int& C) {
  int mx = 0;
  for (int64_t i = 0; i < n; i++) mx = ycodes[i] > mx ? ycodes[i] : mx;
  if (mx >= n_states) {
    set_error(std::string(who) + ": a code is >= n_states");
    return FS_EINVAL;
  }
  if (mx + 1 > kJmiMaxClassesGpu) {
    set_error(std::string(who) + ": the GPU backend supports at most 4 classes of y");
    return FS_EINVAL;
  }
  C = mx + 1;
  return FS_OK;
}

// The row launches of one call: the planes' geometry and y's classes.
struct JmiRows {
  JmiRowArgs a;
  unsigned grid = 0;
  int64_t p = 0;
  int C = 0;
  hipStream_t s = nullptr;

  void init(const MiPlanes& pl, int CPW, int C_, int unit, int method, const double* rel,
            hipStream_t s_) {
    a.row.planes = pl.planes, a.row.kcol = pl.kcol, a.row.n = pl.n, a.row.p = pl.p;
    a.row.P1p = pl.P1p, a.row.W = pl.W, a.row.SP = pl.SP, a.row.NB = pl.NB, a.row.CPW = CPW;
    a.unit = unit, a.method = method, a.rel = rel;
    grid = (unsigned)(pl.P1p / CPW), p = pl.p, C = C_, s = s_;
  }
  int launch(int64_t anchor, const int64_t* anchor_dev, double* out, double* acc) {
    a.row.anchor = anchor, a.row.anchor_dev = anchor_dev, a.out = out, a.acc = acc;
    switch (C) {
      case 1: k_jmi_row_zero<<<(unsigned)((p + 255) / 256), 256, 0, s>>>(a); break;
      case 2: k_jmi_row<2><<<grid, kPtThreads, 0, s>>>(a); break;
      case 3: k_jmi_row<3><<<grid, kPtThreads, 0, s>>>(a); break;
      default: k_jmi_row<4><<<grid, kPtThreads, 0, s>>>(a); break;
    }
    return launch_check("k_jmi_row");
  }
};

int launch_rel(const MiPlanes& pl, int CPW, int unit, double* out, hipStream_t s) {
  JmiRelArgs a;
  a.row.planes = pl.planes, a.row.kcol = pl.kcol, a.row.n = pl.n, a.row.p = pl.p;
  a.row.P1p = pl.P1p, a.row.W = pl.W, a.row.SP = pl.SP, a.row.NB = pl.NB, a.row.CPW = CPW;
  a.row.anchor = pl.p, a.row.anchor_dev = nullptr;  // the target is column p
  a.unit = unit, a.out = out;
  k_jmi_rel<<<(unsigned)(pl.P1p / CPW), kPtThreads, 0, s>>>(a);
  return launch_check("k_jmi_rel");
}

}  // namespace

void jmi_last_timing(double* ms5) {
  for (int k = 0; k < 5; k++) ms5[k] = g_jmi_ms[k];
}

int jmi_select(int device, const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p,
               int n_states, int unit, int method, int64_t k, double* relevance,
               int64_t* selected, double* rows) {
  if (device_count() <= 0) return no_device();
  for (double& v : g_jmi_ms) v = -1.0;
  MiPlanes pl;
  const int CPW = kPtThreads / (((n_states + 3) / 4) * ((n_states + 3) / 4));
  FS_TRY(pl.shape("fs_jmi_select", n, p, n_states, CPW));
  if (rows && (double)k * (double)p * 8.0 > kMiMaxBytes) {
    set_error("fs_jmi_select: the rows do not fit the device memory");
    return FS_EOOM;
  }
  int C = 0;
  FS_TRY(y_classes("fs_jmi_select", ycodes, n, n_states, C));
  FS_HIP(hipSetDevice(device));
  DevArena mem(device);
  StreamLease lease(device);  // destroyed (and the stream synchronised) before `mem`
  // timing: upload, pack, relevance, then (row, step) pairs; above
  // kJmiTimedSteps steps the loop is timed as a whole
  const bool per_step = k - 1 <= kJmiTimedSteps;
  const size_t nev = 4 + (per_step ? 2 * (size_t)(k - 1) + 1 : 1);
  FS_TRY(lease.open(nev));
  hipStream_t s = lease.s;
  std::vector<hipEvent_t>& ev = lease.ev;

  JmiSteps st;
  st.s = s, st.p = p, st.k = k, st.method = method;
  double* drows = nullptr;
  // every block is allocated before any array is uploaded
  FS_TRY(pl.alloc(mem, mem));
  FS_TRY(st.alloc(mem));
  if (rows) FS_TRY(mem.alloc(&drows, (size_t)k * p));

  FS_HIP(hipEventRecord(ev[0], s));
  FS_TRY(pl.upload(codes, ycodes, s));
  FS_TRY(st.reset());
  FS_HIP(hipEventRecord(ev[1], s));
  FS_TRY(pl.pack(s));
  FS_HIP(hipEventRecord(ev[2], s));

  JmiRows jr;
  jr.init(pl, CPW, C, unit, method, st.rel, s);
  FS_TRY(launch_rel(pl, CPW, unit, st.rel, s));
  FS_TRY(st.step(0));
  FS_HIP(hipEventRecord(ev[3], s));
  // k - 1 x (the last pick's row into the accumulators, the next pick), back to back
  for (int64_t i = 1; i < k; i++) {
    FS_TRY(jr.launch(-1, st.sel + (i - 1), rows ? drows + (size_t)(i - 1) * p : nullptr, st.acc));
    if (per_step) FS_HIP(hipEventRecord(ev[2 + 2 * i], s));
    FS_TRY(st.step(i));
    if (per_step) FS_HIP(hipEventRecord(ev[3 + 2 * i], s));
  }
  // the last pick's row feeds no step: only a caller's rows need it
  if (rows) FS_TRY(jr.launch(-1, st.sel + (k - 1), drows + (size_t)(k - 1) * p, nullptr));
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
  for (int t = 0; t < 3; t++) g_jmi_ms[t] = span(t, t + 1);
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
    g_jmi_ms[3] = ok ? r + last : -1.0;
    g_jmi_ms[4] = ok ? t : -1.0;
  } else {
    g_jmi_ms[3] = span(3, 4);  // rows and steps together; steps stays -1
  }
  (void)hipGetLastError();
  return FS_OK;
}

int jmi_rows(int device, const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p,
             int n_states, int unit, const int64_t* anchors, int64_t m, double* rows) {
  if (device_count() <= 0) return no_device();
  MiPlanes pl;
  const int CPW = kPtThreads / (((n_states + 3) / 4) * ((n_states + 3) / 4));
  FS_TRY(pl.shape("fs_jmi_rows", n, p, n_states, CPW));
  if ((double)m * (double)p * 8.0 > kMiMaxBytes) {
    set_error("fs_jmi_rows: the rows do not fit the device memory");
    return FS_EOOM;
  }
  int C = 0;
  FS_TRY(y_classes("fs_jmi_rows", ycodes, n, n_states, C));
  FS_HIP(hipSetDevice(device));
  DevArena mem(device);
  StreamLease lease(device);  // destroyed (and the stream synchronised) before `mem`
  FS_TRY(lease.open(0));
  hipStream_t s = lease.s;
  double* drows = nullptr;
  FS_TRY(pl.alloc(mem, mem));
  FS_TRY(mem.alloc(&drows, (size_t)m * p));
  FS_TRY(pl.upload(codes, ycodes, s));
  FS_TRY(pl.pack(s));
  JmiRows jr;
  jr.init(pl, CPW, C, unit, kJmiJmi, nullptr, s);
  for (int64_t t = 0; t < m; t++) FS_TRY(jr.launch(anchors[t], nullptr, drows + (size_t)t * p, nullptr));
  FS_TRY(pl.fetch_bad(s));
  FS_HIP(hipMemcpyAsync(rows, drows, (size_t)m * p * 8, hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  FS_TRY(pl.check());
  return FS_OK;
}

int jmi_search_matrix(int device, const double* relevance, const double* joint, int64_t p,
                      int method, int64_t k, int64_t* selected) {
  if (device_count() <= 0) return no_device();
  if ((double)p * (double)p * 8.0 > kMiMaxBytes) {
    set_error("fs_jmi_search_matrix: the matrix does not fit the device memory");
    return FS_EOOM;
  }
  FS_HIP(hipSetDevice(device));
  DevArena mem(device);
  StreamLease lease(device);  // destroyed (and the stream synchronised) before `mem`
  FS_TRY(lease.open(0));
  hipStream_t s = lease.s;
  JmiSteps st;
  st.s = s, st.p = p, st.k = k, st.method = method;
  double* djoint = nullptr;
  FS_TRY(st.alloc(mem));
  FS_TRY(mem.alloc(&djoint, (size_t)p * p));
  FS_HIP(hipMemcpyAsync(st.rel, relevance, (size_t)p * 8, hipMemcpyHostToDevice, s));
  FS_HIP(hipMemcpyAsync(djoint, joint, (size_t)p * p * 8, hipMemcpyHostToDevice, s));
  FS_TRY(st.reset());
  FS_TRY(st.step(0));
  for (int64_t i = 1; i < k; i++) {
    k_jmi_addrow<<<(unsigned)((p + 255) / 256), 256, 0, s>>>(djoint, p, st.sel + (i - 1), st.rel,
                                                            method, st.acc);
    FS_TRY(launch_check("k_jmi_addrow"));
    FS_TRY(st.step(i));
  }
  FS_HIP(hipMemcpyAsync(selected, st.sel, (size_t)k * 8, hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  return FS_OK;
}

}  // namespace gpu
}  // namespace fs
