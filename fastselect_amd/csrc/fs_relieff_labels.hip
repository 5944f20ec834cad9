// fs_relieff_labels.hip -- the ReliefF permutation test on the GPU: the score
// sums of B labellings of the plan's samples on one pass 1.
//
// ReliefF's neighbour sets read the labels (the k nearest of every class), so
// MultiSURF's shortcut of re-weighing label-independent near sets
// (fs_labels.hip) does not carry over.  Two things do not read the labels:
// the distance pass, and the order in which the reference walks a row -- one
// argsort of the row's float32 keys (ReliefF.py:157-175).  For any labelling
// the k nearest of a class are the first k of that class met on that walk,
// and with class shares that are not tiny the walk ends within a few dozen
// entries.  Two routes:
//
//  general (always correct, the baseline): per labelling the class codes go
//     in place of the plan's lab / lab8, its counts and priors in place of
//     the plan's (relieff_set_labelling), and relieff_select_update
//     (fs_relieff.hip) runs the kernels and the order of a plain plan_score
//     on the resident keys: row b carries the bits of a plan created with
//     labelling b as y.
//  fast, per chunk of at most 32 labellings:
//   1. candidate prefix, once per call: k_rfl_prefix takes the L smallest
//      exact keys of every row (relieff_exact_rows: k_rf_select's exact-key
//      arithmetic for whole rows; an all-discrete layout's keys are exact
//      already) by a radix select on the key bits, sorts them by (key, index)
//      in LDS and cuts the usable length lok before a run of equal keys that
//      goes on past L (lok = n - 1 when the prefix holds the whole row).
//      Rows whose prefix holds equal adjacent keys get those runs in numba's
//      quicksort order (relieff_prefix_ties: k_rf_ref_ties' focus replay over
//      the row's exact keys).  k_rfl_records lists (i, cand) as the records
//      k_lab_score walks, L per row, groups of 256 records as its "tiles".
//   2. walk and weights: k_rfl_walk, one wave per row, lanes over the
//      candidates; per labelling and present class one ballot of "candidate
//      is of class c" per 64 candidates and a prefix popcount give the rank
//      within the class; rank < k is chosen, weight -1 / h for a hit and
//      (P_c / (1 - P_y)) / k for a miss, in float64 as k_rf_update forms
//      them, rounded once into W[record][32].  A class short of k within a
//      prefix that is not the whole row raises the labelling's overflow flag.
//   3. score: k_lab_score and k_lab_reduce of fs_labels.hip, unchanged
//      (lab_score_reduce).
//     A labelling that overflowed is scored again on the general route.
//
// Which route (plan_relieff_score_labels): general for a labelling with a
// present class of at most k members, with more than 8 classes, or whose
// depth need min(ceil(3 k / smallest class share), n - 1) exceeds 256 (or with
// n above kRflMaxRows, the exact-key kernel's grid); and for
// all of them when fewer than kRflMinFast are left, when the prefix (whole
// rows of exact keys, paid once per call) would cost more than two thirds of
// what the general route costs for them (the estimate is beside the rule), or
// when the rf_labels_route hook says so.  L is the smallest of 64,
// 128, 256 that covers the largest need (rf_labels_depth forces it).  The
// factor 3 is a guess; correctness does not rest on it, since every overflow
// is caught and rerun.
#include "fs_gpu_internal.h"

namespace fs {
namespace gpu {

namespace {

constexpr int kRflB = 32;        // labellings per chunk (k_lab_score's)
constexpr int kRflGroup = 256;   // records per group (k_lab_score's fold)
constexpr int kRflMaxL = 256;
constexpr int64_t kRflMinFast = 8;  // fast-route labellings below which the prefix is not worth it
// relieff_exact_rows' grid has ceil(n / 4) blocks in y (at most 65535)
constexpr int64_t kRflMaxRows = 4 * 65535 - 3;
constexpr double kRflKeySec = 1.3e-12, kRflGenSec = 1.5e-4, kRflSelSec = 3.6e-12, kRflUpdSec = 2.3e-12;

// The L smallest keys of row i = row0 + blockIdx.x (keys + blockIdx.x *
// stride: n floats, the entry at i ignored), ascending by (key, index):
// cand[i * L + s], ckeys[i * L + s] for s < lok[i]; beyond that cand = i (a
// zero diff, never weighted) and ckeys = +inf.  dup[i] = 1 when two adjacent
// keys of the prefix are equal.  Keys are >= +0, so their bit patterns order
// as they do.
__global__ __launch_bounds__(256) void k_rfl_prefix(const float* __restrict__ keys,
                                                    int64_t stride, int64_t row0, int n, int L,
                                                    int32_t* __restrict__ cand,
                                                    float* __restrict__ ckeys,
                                                    int32_t* __restrict__ lok,
                                                    int32_t* __restrict__ dup) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_prefix, s_need, s_less, s_eq, s_cnt, s_dup;
  __shared__ uint32_t ck[kRflMaxL];
  __shared__ int32_t cj[kRflMaxL];
  const int tid = threadIdx.x;
  const int i = (int)(row0 + blockIdx.x);
  const uint32_t* __restrict__ row = (const uint32_t*)(keys + (int64_t)blockIdx.x * stride);
  const int m = n - 1;
  const bool whole = m <= L;
  if (tid == 0) s_prefix = 0u, s_need = (uint32_t)L, s_less = 0u, s_eq = 0u, s_cnt = 0u, s_dup = 0u;
  __syncthreads();
  if (!whole) {
    // the L-th smallest key T, the keys below it and those equal to it
    for (int pass = 0; pass < 4; pass++) {
      const int lo = 24 - 8 * pass;
      hist[tid] = 0u;
      __syncthreads();
      const uint32_t pre = s_prefix;
      for (int j = tid; j < n; j += 256) {
        if (j == i) continue;
        const uint32_t kv = row[j];
        if (pass == 0 || (kv >> (lo + 8)) == (pre >> (lo + 8))) atomicAdd(&hist[(kv >> lo) & 255u], 1u);
      }
      __syncthreads();
      if (tid == 0) {
        uint32_t cum = 0u, need = s_need;
        int b = 0;
        while (b < 255 && cum + hist[b] < need) cum += hist[b++];
        s_prefix = pre | ((uint32_t)b << lo);
        s_need = need - cum;
        s_less += cum;
        s_eq = hist[b];
      }
      __syncthreads();
    }
  }
  const uint32_t T = s_prefix, less = s_less, eq = s_eq;
  const bool take_eq = whole || less + eq <= (uint32_t)L;
  const int Lok = whole ? m : (int)(take_eq ? less + eq : less);
  for (int j = tid; j < n; j += 256) {
    if (j == i) continue;
    const uint32_t kv = row[j];
    if (whole || kv < T || (take_eq && kv == T)) {
      const uint32_t s = atomicAdd(&s_cnt, 1u);
      if (s < (uint32_t)kRflMaxL) ck[s] = kv, cj[s] = j;
    }
  }
  __syncthreads();
  // rank of every collected entry by (key, index): its place in the prefix
  int32_t* __restrict__ oc = cand + (int64_t)i * L;
  float* __restrict__ ok = ckeys + (int64_t)i * L;
  uint32_t myk = 0u;
  int32_t myj = 0, rank = -1;
  if (tid < Lok) {
    myk = ck[tid], myj = cj[tid], rank = 0;
    for (int f = 0; f < Lok; f++) {
      const uint32_t kf = ck[f];
      rank += (kf < myk || (kf == myk && cj[f] < myj)) ? 1 : 0;
    }
  }
  __syncthreads();
  if (rank >= 0) ck[rank] = myk, cj[rank] = myj;
  __syncthreads();
  if (tid < L) {
    const bool in = tid < Lok;
    oc[tid] = in ? cj[tid] : i;
    ok[tid] = in ? __uint_as_float(ck[tid]) : __builtin_inff();
    if (in && tid > 0 && ck[tid] == ck[tid - 1]) s_dup = 1u;
  }
  __syncthreads();
  if (tid == 0) lok[i] = Lok, dup[i] = (int32_t)s_dup;
}

// rec[i * L + s] = (i, cand | 1 << 30); the padding of the last group stays
// (0, 0, no flag) from the caller's memset.  goff[t] = t: a group is a tile.
__global__ __launch_bounds__(256) void k_rfl_records(const int32_t* __restrict__ cand,
                                                     int64_t nrec_rows, int L, int64_t ngroups,
                                                     int2* __restrict__ rec,
                                                     int64_t* __restrict__ goff) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g <= ngroups) goff[g] = g;
  if (g >= nrec_rows) return;
  rec[g] = make_int2((int32_t)(g / L), (int32_t)((uint32_t)cand[g] | (1u << 30)));
}

// One wave per row i.  labT[j * 32 + b]: the class of sample j under
// labelling b of the chunk; cmask[b]: the present classes (codes < 64);
// prior[b * 64 + c].  W[(i * L + s) * 32 + b] for every s < L and b < 32.
__global__ __launch_bounds__(64) void k_rfl_walk(const int32_t* __restrict__ cand,
                                                 const int32_t* __restrict__ lok, int L, int cap,
                                                 int n, int k, const int32_t* __restrict__ labT,
                                                 int nb, const uint64_t* __restrict__ cmask,
                                                 const double* __restrict__ prior,
                                                 float* __restrict__ W,
                                                 int32_t* __restrict__ overflow) {
  const int lane = threadIdx.x;
  const int64_t i = blockIdx.x;
  const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  int leff = lok[i];
  if (cap > 0 && cap < leff) leff = cap;
  const bool whole = leff == n - 1;
  const int ns = L >> 6;  // 1, 2 or 4 runs of 64 candidates
  int64_t cj[4];
  bool valid[4];
#pragma unroll
  for (int s = 0; s < 4; s++) {
    const int e = lane + 64 * s;
    valid[s] = s < ns && e < leff;
    cj[s] = s < ns ? cand[i * L + e] : i;
  }
  for (int b = 0; b < kRflB; b++) {
    float w[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (b < nb) {
      const int li = labT[i * kRflB + b];
      int myc[4];
#pragma unroll
      for (int s = 0; s < 4; s++) myc[s] = valid[s] ? labT[cj[s] * kRflB + b] : -1;
      double denom = 1.0 - prior[b * 64 + li];
      if (denom == 0.0) denom = 1.0;
      uint64_t cm = cmask[b];
      while (cm) {
        const int c = (int)__builtin_ctzll(cm);
        cm &= cm - 1;
        int total = 0, rank[4];
#pragma unroll
        for (int s = 0; s < 4; s++) {
          const uint64_t mm = __ballot(myc[s] == c);
          rank[s] = total + __popcll(mm & below);
          total += __popcll(mm);
        }
        if (total < k && !whole) {
          if (lane == 0) overflow[b] = 1;
          continue;
        }
        // the self-hit of a class with fewer than k other members (k_rf_update)
        const int found = total < k ? total : k;
        const int64_t h_found = found < k ? (int64_t)found + 1 : (int64_t)k;
        const double wgt =
            (c == li) ? -1.0 / (double)h_found : (prior[b * 64 + c] / denom) / (double)k;
#pragma unroll
        for (int s = 0; s < 4; s++)
          if (myc[s] == c && rank[s] < k) w[s] = (float)wgt;
      }
    }
#pragma unroll
    for (int s = 0; s < 4; s++)
      if (s < ns) W[((i * L + lane + 64 * s) * kRflB) + b] = w[s];
  }
}

struct Labelling {
  int64_t cc[kRfLabelCodes];
  std::vector<double> prior;  // 64 entries
  int n_classes = 0;
  uint64_t cmask = 0;
  int64_t need = 0;           // depth need; > kRflMaxL: general route
};

// The general route for the labellings idx, one after the other, on the
// resident keys.  The caller restores the plan's labels.
int general_loop(Plan* g, const int32_t* labels, const std::vector<int64_t>& idx, int c_max,
                 double* scores) {
  if (idx.empty()) return FS_OK;
  const int64_t n = g->P.n, k = g->P.k_neighbors, n_kept = g->P.n_kept;
  const int64_t nrb = std::max<int64_t>(1, (n + kRfRows - 1) / kRfRows);
  DevArena& M = g->mem_call;
  double *dprior = nullptr, *part = nullptr;
  int64_t* dcc = nullptr;
  int32_t *nbr = nullptr, *nfound = nullptr;
  FS_TRY(M.alloc(&dprior, (size_t)kRfLabelCodes));
  FS_TRY(M.alloc(&dcc, (size_t)kRfLabelCodes));
  FS_TRY(M.alloc(&part, (size_t)nrb * g->P.PW));
  FS_TRY(M.alloc(&nbr, (size_t)n * c_max * std::max<int64_t>(k, 1)));
  FS_TRY(M.alloc(&nfound, (size_t)n * c_max));
  const size_t mark = M.blocks.size();
  std::vector<uint8_t> lab8((size_t)n);
  int64_t cc[kRfLabelCodes];
  std::vector<double> prior((size_t)kRfLabelCodes);
  for (int64_t b : idx) {
    const int32_t* lab = labels + b * n;
    relieff_set_labelling(g->P, lab, cc);  // checked by the caller
    std::fill(prior.begin(), prior.end(), 0.0);
    std::copy(g->P.class_prior.begin(), g->P.class_prior.end(), prior.begin());
    for (int64_t i = 0; i < n; i++) lab8[i] = (uint8_t)lab[i];
    FS_TRY(h2d(g, g->lab, lab, (size_t)n));
    FS_TRY(h2d(g, g->lab8, lab8.data(), (size_t)n));
    FS_TRY(h2d(g, dcc, cc, (size_t)kRfLabelCodes));
    FS_TRY(h2d(g, dprior, prior.data(), (size_t)kRfLabelCodes));
    FS_HIP(hipEventRecord(g->ev_rf_labels[0], g->stream));
    FS_TRY(relieff_select_update(g, dcc, dprior, nbr, nfound, part, scores + b * n_kept));
    FS_HIP(hipEventRecord(g->ev_rf_labels[1], g->stream));
    // the host arrays above and the selection's temporaries serve the next
    // labelling: this one has to be through with them
    FS_HIP(hipStreamSynchronize(g->stream));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, g->ev_rf_labels[0], g->ev_rf_labels[1]) == hipSuccess)
      g->rf_labels_ms[3] += (double)ms;
    else
      (void)hipGetLastError();
    while (M.blocks.size() > mark) {
      dev_free(M.blocks.back());
      M.blocks.pop_back();
    }
  }
  return FS_OK;
}

double span_ms(hipEvent_t a, hipEvent_t b) {
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, a, b) != hipSuccess) {
    (void)hipGetLastError();
    return 0.0;
  }
  return (double)ms;
}

// The fast route for the labellings idx at depth L; the ones that overflowed
// are appended to `again`.
int fast_loop(Plan* g, const int32_t* labels, const std::vector<Labelling>& info,
              const std::vector<int64_t>& idx, int L, double* scores,
              std::vector<int64_t>& again) {
  const Prepared& Q = g->P;
  const int64_t n = Q.n, n_kept = Q.n_kept;
  const int k = (int)Q.k_neighbors;
  hipStream_t st = g->stream;
  hipEvent_t* ev = g->ev_rf_fast;
  DevArena& M = g->mem_call;
  const int64_t nrows_rec = n * L;
  const int64_t ngroups = (nrows_rec + kRflGroup - 1) / kRflGroup;
  const int64_t nrec = ngroups * kRflGroup;
  int32_t *cand = nullptr, *lok = nullptr, *dup = nullptr;
  float* ckeys = nullptr;
  int2* rec = nullptr;
  int64_t* goff = nullptr;
  FS_TRY(M.alloc(&cand, (size_t)nrows_rec));
  FS_TRY(M.alloc(&ckeys, (size_t)nrows_rec));
  FS_TRY(M.alloc(&lok, (size_t)n));
  FS_TRY(M.alloc(&dup, (size_t)n));
  FS_TRY(M.alloc(&rec, (size_t)nrec));
  FS_TRY(M.alloc(&goff, (size_t)ngroups + 1));
  // ---- 1. candidate prefix, once per call
  FS_HIP(hipEventRecord(ev[0], st));
  if (Q.pc == 0) {  // the plan's keys are exact
    k_rfl_prefix<<<(unsigned)n, 256, 0, st>>>(g->Dk, Q.n_pad, 0, (int)n, L, cand, ckeys, lok, dup);
    FS_TRY(launch_check("k_rfl_prefix"));
  } else {
    const int64_t batch = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)(1ll << 30) / (4 * n)));
    float* keys = nullptr;
    int32_t* drows = nullptr;
    FS_TRY(M.alloc(&keys, (size_t)(batch * n)));
    FS_TRY(M.alloc(&drows, (size_t)n));
    std::vector<int32_t> all((size_t)n);
    for (int64_t i = 0; i < n; i++) all[i] = (int32_t)i;
    FS_TRY(h2d(g, drows, all.data(), (size_t)n));
    for (int64_t r0 = 0; r0 < n; r0 += batch) {
      const int64_t nr = std::min<int64_t>(batch, n - r0);
      FS_TRY(relieff_exact_rows(g, drows + r0, nr, keys));
      k_rfl_prefix<<<(unsigned)nr, 256, 0, st>>>(keys, n, r0, (int)n, L, cand, ckeys, lok, dup);
      FS_TRY(launch_check("k_rfl_prefix"));
    }
    FS_HIP(hipStreamSynchronize(st));  // `all` is read by the upload
  }
  std::vector<int32_t> hdup((size_t)n), tie_rows;
  FS_HIP(hipMemcpyAsync(hdup.data(), dup, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
  FS_HIP(hipStreamSynchronize(st));
  for (int64_t i = 0; i < n; i++)
    if (hdup[i]) tie_rows.push_back((int32_t)i);
  FS_TRY(relieff_prefix_ties(g, tie_rows, L, cand, lok, ckeys));
  FS_HIP(hipMemsetAsync(rec, 0, sizeof(int2) * (size_t)nrec, st));
  k_rfl_records<<<(unsigned)((std::max(nrows_rec, ngroups + 1) + 255) / 256), 256, 0, st>>>(
      cand, nrows_rec, L, ngroups, rec, goff);
  FS_TRY(launch_check("k_rfl_records"));
  FS_HIP(hipEventRecord(ev[1], st));
  // ---- per chunk
  int64_t chunk = kRflB;
  if (test_hooks().labels_chunk >= 1) chunk = std::min<int64_t>(kRflB, test_hooks().labels_chunk);
  int64_t seg_len = 1, nseg = 1;
  lab_score_split(g, ngroups, &seg_len, &nseg);
  int32_t *lab_raw = nullptr, *labT = nullptr, *ovf = nullptr;
  uint64_t* dmask = nullptr;
  double *dprior = nullptr, *part = nullptr, *out = nullptr;
  float* W = nullptr;
  FS_TRY(M.alloc(&lab_raw, (size_t)chunk * n));
  FS_TRY(M.alloc(&labT, (size_t)kRflB * n));
  FS_TRY(M.alloc(&ovf, (size_t)kRflB));
  FS_TRY(M.alloc(&dmask, (size_t)kRflB));
  FS_TRY(M.alloc(&dprior, (size_t)kRflB * 64));
  FS_TRY(M.alloc(&W, (size_t)nrec * kRflB));
  FS_TRY(M.alloc(&part, (size_t)chunk * nseg * Q.PW));
  FS_TRY(M.alloc(&out, (size_t)chunk * n_kept));
  // the padding records of the last group: never written by the walk
  FS_HIP(hipMemsetAsync(W + nrows_rec * kRflB, 0, sizeof(float) * (size_t)(nrec - nrows_rec) * kRflB,
                        st));
  const int cap = (int)std::max<int64_t>(0, test_hooks().rf_labels_depth_cap);
  std::vector<uint64_t> hmask((size_t)kRflB);
  std::vector<double> hprior((size_t)kRflB * 64);
  int32_t hovf[kRflB];
  for (size_t c0 = 0; c0 < idx.size(); c0 += (size_t)chunk) {
    const int nb = (int)std::min<size_t>((size_t)chunk, idx.size() - c0);
    std::fill(hmask.begin(), hmask.end(), 0ull);
    std::fill(hprior.begin(), hprior.end(), 0.0);
    for (int q = 0; q < nb; q++) {
      const int64_t b = idx[c0 + q];
      FS_HIP(hipMemcpyAsync(lab_raw + (int64_t)q * n, labels + b * n, sizeof(int32_t) * (size_t)n,
                            hipMemcpyHostToDevice, st));
      hmask[q] = info[b].cmask;
      std::copy(info[b].prior.begin(), info[b].prior.end(), hprior.begin() + (size_t)q * 64);
    }
    FS_TRY(h2d(g, dmask, hmask.data(), hmask.size()));
    FS_TRY(h2d(g, dprior, hprior.data(), hprior.size()));
    FS_HIP(hipMemsetAsync(ovf, 0, sizeof(int32_t) * kRflB, st));
    FS_HIP(hipEventRecord(ev[2], st));
    FS_TRY(lab_transpose(g, lab_raw, nb, labT));
    k_rfl_walk<<<(unsigned)n, 64, 0, st>>>(cand, lok, L, cap, (int)n, k, labT, nb, dmask, dprior, W,
                                           ovf);
    FS_TRY(launch_check("k_rfl_walk"));
    FS_HIP(hipEventRecord(ev[3], st));
    FS_HIP(hipEventRecord(ev[4], st));
    FS_TRY(lab_score_reduce(g, rec, goff, W, ngroups, seg_len, nseg, nb, part, out));
    FS_HIP(hipEventRecord(ev[5], st));
    for (int q = 0; q < nb; q++)
      FS_HIP(hipMemcpyAsync(scores + idx[c0 + q] * n_kept, out + (int64_t)q * n_kept,
                            sizeof(double) * (size_t)n_kept, hipMemcpyDeviceToDevice, st));
    FS_HIP(hipMemcpyAsync(hovf, ovf, sizeof(int32_t) * kRflB, hipMemcpyDeviceToHost, st));
    FS_HIP(hipStreamSynchronize(st));
    g->rf_labels_ms[1] += span_ms(ev[2], ev[3]);
    g->rf_labels_ms[2] += span_ms(ev[4], ev[5]);
    for (int q = 0; q < nb; q++)
      if (hovf[q]) again.push_back(idx[c0 + q]);
  }
  g->rf_labels_ms[0] = span_ms(ev[0], ev[1]);
  return FS_OK;
}

}  // namespace

int plan_relieff_score_labels(Plan* g, const int32_t* labels, int64_t B, double* scores) {
  const int64_t n = g->P.n, k = g->P.k_neighbors;
  FS_HIP(hipSetDevice(g->device));
  if (!g->mem_call.blocks.empty()) {  // a call on a caller's stream keeps its buffers
    FS_HIP(hipStreamSynchronize(g->stream));
    g->mem_call.release();
  }
  if (B <= 0) return FS_OK;
  // every labelling is checked before the plan is touched; its route
  int c_max = 0;
  std::vector<Labelling> info((size_t)B);
  std::vector<int64_t> fast, general;
  int64_t need_max = 0;
  {
    Prepared T;
    T.n = n;
    for (int64_t b = 0; b < B; b++) {
      Labelling& lb = info[b];
      if (const int bad = relieff_set_labelling(T, labels + b * n, lb.cc)) {
        set_error("fs_plan_relieff_score_labels: labelling " + std::to_string(b) +
                  (bad == 1 ? " holds a class code outside [0, 64)"
                            : " has fewer than 2 classes"));
        return FS_EINVAL;
      }
      lb.n_classes = T.n_classes;
      lb.prior.assign((size_t)kRfLabelCodes, 0.0);
      std::copy(T.class_prior.begin(), T.class_prior.end(), lb.prior.begin());
      c_max = std::max<int>(c_max, T.n_classes);
      int present = 0;
      int64_t smallest = n;
      for (int c = 0; c < kRfLabelCodes; c++)
        if (lb.cc[c] > 0) {
          present++;
          lb.cmask |= 1ull << c;
          smallest = std::min(smallest, lb.cc[c]);
        }
      // ceil(3 k / share), a prefix that holds the whole row at the most
      lb.need = std::min<int64_t>((3 * k * n + smallest - 1) / smallest, n - 1);
      const bool slow = test_hooks().rf_labels_route == 1 || smallest <= k || present > 8 ||
                        lb.need > kRflMaxL || k < 1 || n > kRflMaxRows;
      (slow ? general : fast).push_back(b);
      if (!slow) need_max = std::max(need_max, lb.need);
    }
  }
  // The prefix is paid once per call and the general route once per
  // labelling: whole rows of exact keys cost about kRflKeySec per pair and
  // continuous feature (an all-discrete layout's keys are the plan's), a
  // general-route labelling about kRflGenSec + kRflSelSec n^2 + kRflUpdSec
  // n k C PW (fits to the three shapes of tools/bench_relieff_perm.py on an
  // MI355X).  The fast route is taken when it saves half again its prefix.
  // The constants are absolute seconds of that one device and clock: on
  // another part the rule can pick the slower route (never a wrong result);
  // the margin of 1.5 has not been swept.
  const double prefix_s = kRflKeySec * (double)n * (double)n * (double)g->P.pc;
  const double general_s = kRflGenSec + kRflSelSec * (double)n * (double)n +
                           kRflUpdSec * (double)n * (double)k * (double)c_max * (double)g->P.PW;
  const bool pays = (double)fast.size() * general_s >= 1.5 * prefix_s;
  if (((int64_t)fast.size() < kRflMinFast || !pays) && !(test_hooks().rf_labels_depth > 0)) {
    general.insert(general.end(), fast.begin(), fast.end());
    std::sort(general.begin(), general.end());
    fast.clear();
  }
  int L = need_max <= 64 ? 64 : need_max <= 128 ? 128 : 256;
  if (const int64_t d = test_hooks().rf_labels_depth; d == 64 || d == 128 || d == 256) L = (int)d;
  for (auto& e : g->ev_rf_labels)
    if (!e && !(e = event_get(g->device, true))) return FS_EHIP;
  for (auto& e : g->ev_rf_fast)
    if (!e && !(e = event_get(g->device, true))) return FS_EHIP;
  for (int q = 0; q < 4; q++) g->rf_labels_info[q] = 0, g->rf_labels_ms[q] = 0.0;
  g->rf_labels_info[0] = -1;
  const std::vector<int32_t> own_labels = g->P.labels;
  const std::vector<double> own_prior = g->P.class_prior;
  const int32_t own_classes = g->P.n_classes;
  std::vector<int64_t> again;
  int rc = run_quantize_dist(g);
  if (rc == FS_OK && !fast.empty()) rc = fast_loop(g, labels, info, fast, L, scores, again);
  if (rc == FS_OK) rc = general_loop(g, labels, general, c_max, scores);
  if (rc == FS_OK) rc = general_loop(g, labels, again, c_max, scores);
  // the plan's own state, whatever happened
  g->P.labels = own_labels;
  g->P.class_prior = own_prior;
  g->P.n_classes = own_classes;
  std::vector<uint8_t> lab8((size_t)n);
  for (int64_t i = 0; i < n; i++) lab8[i] = (uint8_t)own_labels[i];
  int rc2 = h2d(g, g->lab, own_labels.data(), (size_t)n);
  if (rc2 == FS_OK) rc2 = h2d(g, g->lab8, lab8.data(), (size_t)n);
  if (hipStreamSynchronize(g->stream) != hipSuccess && rc2 == FS_OK) {
    (void)hipGetLastError();
    set_error("fs_plan_relieff_score_labels: the stream failed while the plan's labels went back");
    rc2 = FS_EHIP;
  }
  g->mem_call.release();
  if (rc != FS_OK || rc2 != FS_OK) return rc != FS_OK ? rc : rc2;
  g->rf_labels_info[0] = (int64_t)fast.size();
  g->rf_labels_info[1] = (int64_t)general.size();
  g->rf_labels_info[2] = (int64_t)again.size();
  g->rf_labels_info[3] = fast.empty() ? 0 : L;
  return FS_OK;
}

int plan_relieff_labels_info(const Plan* g, int64_t* out4) {
  if (g->rf_labels_info[0] < 0) {
    set_error("fs_plan_relieff_labels_info: no completed fs_plan_relieff_score_labels call");
    return FS_EINVAL;
  }
  for (int q = 0; q < 4; q++) out4[q] = g->rf_labels_info[q];
  return FS_OK;
}

double plan_relieff_labels_kernel_ms(const Plan* g, int which) {
  if (g->rf_labels_info[0] < 0 || which < 0 || which > 3) return -1.0;
  return g->rf_labels_ms[which];
}

int relieff_labels_run(const Prepared& P, const void* x, int device, const int32_t* labels,
                       int64_t B, float* scores_out) {
  Plan* g = nullptr;
  FS_TRY(plan_create(&g, P, x, 0, device, 0, 1, 0, 0, P.n));
  double* out = nullptr;
  std::vector<double> host((size_t)B * P.n_kept);
  int rc = g->mem_plan.alloc(&out, host.size());
  if (rc == FS_OK) rc = plan_relieff_score_labels(g, labels, B, out);
  if (rc == FS_OK &&
      hipMemcpy(host.data(), out, sizeof(double) * host.size(), hipMemcpyDeviceToHost) !=
          hipSuccess) {
    (void)hipGetLastError();
    set_error("fs_relieff_score_labels: copying the scores to the host failed");
    rc = FS_EHIP;
  }
  plan_destroy(g);
  if (rc != FS_OK) return rc;
  for (size_t q = 0; q < host.size(); q++) scores_out[q] = (float)(host[q] / (double)P.n);
  return FS_OK;
}

}  // namespace gpu
}  // namespace fs
