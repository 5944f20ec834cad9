// fs_rrelieff.hip -- the RReliefF sums of a one-class ReliefF plan on the GPU
// (definitions: fs_rrelieff.h): per feature the sum of diff over the
// (focal row, neighbour) pairs (S_A) and, per target, the sum of dy * diff
// (S_CA); per target the sum of dy (S_C).  The neighbours do not read the
// target, so pass 1 and relieff_select run once per call; a chunk of up to 8
// targets then costs its pairs' weights (k_rrf_dy), their sums (k_rrf_sc) and
// one gather over the lists nbr / nfound and the pass-2 operands xs
// (k_rrf_update, modelled on k_rf_stir).
// Shared state and helpers: fs_gpu_internal.h.
#include "fs_gpu_internal.h"
#include "fs_rrelieff.h"

namespace fs {
namespace gpu {

// Targets per launch of k_rrf_update: 8 (one float64 FMA accumulator each),
// or 1 for a single target (a fit, the ragged end of 8 q + 1 targets).  A
// ragged chunk of 2..7 runs at 8 on zero targets whose rows are not read.
constexpr int kRrfChunk = 8;
// Neighbours gathered per step of the list walk (as kRfStirUnroll): their
// indices are wave-uniform, so the row gathers of a step are in flight
// together.
constexpr int kRrfUnroll = 4;

// dy of every (focal row, list position) pair for the chunk's targets:
// dy[((i - r_lo) * k + pos) * cw + t] = |u_i - u_j| in float64, 0 beyond the
// row's list.  One thread per pair.  u is laid out [n][cw].  Computed once
// per chunk: k_rrf_update's feature blocks and lanes would each repeat it.
__global__ __launch_bounds__(256) void k_rrf_dy(const int32_t* __restrict__ nbr,
                                                const int32_t* __restrict__ nfound, int64_t k,
                                                int64_t r_lo, int64_t r_hi,
                                                const double* __restrict__ u, int cw,
                                                double* __restrict__ dy) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (r_hi - r_lo) * k) return;
  const int64_t i = r_lo + e / k, pos = e % k;
  const bool in = pos < nfound[i];
  const int64_t j = in ? nbr[i * k + pos] : i;
  for (int t = 0; t < cw; t++)
    dy[e * cw + t] = in ? __builtin_fabs(u[i * cw + t] - u[j * cw + t]) : 0.0;
}

// N neighbours lst[0..N) of a focal row: N indices, N row gathers, then per
// gathered value the diff once, into sa and with the wave-uniform weight dy
// of each target into sca[t] by one float64 FMA.  w = the dy of lst[0]: a
// neighbour's CW weights are one contiguous scalar load.  The order is the
// list's for every CW: a target's bits do not depend on the chunk it is
// scored in.
template <bool DISC, int CW, int N>
__device__ __forceinline__ void rrf_step(const float* __restrict__ xc, int64_t PW, float a,
                                         const int32_t* __restrict__ lst,
                                         const double* __restrict__ w, double& sa,
                                         double (&sca)[CW]) {
  int32_t j[N];
  float b[N];
#pragma unroll
  for (int q = 0; q < N; q++) j[q] = __builtin_amdgcn_readfirstlane(lst[q]);
#pragma unroll
  for (int q = 0; q < N; q++) b[q] = xc[(int64_t)j[q] * PW];
#pragma unroll
  for (int q = 0; q < N; q++) {
    const double d = DISC ? ((a != b[q]) ? 1.0 : 0.0) : (double)__builtin_fabsf(a - b[q]);
    sa += d;
#pragma unroll
    for (int t = 0; t < CW; t++) sca[t] = __builtin_fma(w[q * CW + t], d, sca[t]);
  }
}

// The focal rows b0 + wave, b0 + wave + 4, ... of one row block for one
// lane's feature: whole steps of kRrfUnroll, then the ragged rest on a
// wave-uniform switch.
template <bool DISC, int CW>
__device__ __forceinline__ void rrf_rows(const float* __restrict__ xc, int64_t PW, int64_t r_lo,
                                         int64_t b0, int64_t r_hi, int wave, int64_t k,
                                         const int32_t* __restrict__ nbr,
                                         const int32_t* __restrict__ nfound,
                                         const double* __restrict__ dy, double& sa,
                                         double (&sca)[CW]) {
  static_assert(kRrfUnroll == 4, "the switch below lists the rests of steps of 4");
  for (int64_t i = b0 + wave; i < r_hi && i < b0 + kRfRows; i += 4) {
    const int32_t found = __builtin_amdgcn_readfirstlane(nfound[i]);
    const float a = xc[i * PW];
    const int32_t* __restrict__ lst = nbr + i * k;
    const double* __restrict__ w = dy + (i - r_lo) * k * CW;
    int32_t t = 0;
    for (; t + kRrfUnroll <= found; t += kRrfUnroll)
      rrf_step<DISC, CW, kRrfUnroll>(xc, PW, a, lst + t, w + t * CW, sa, sca);
    switch (found - t) {
      case 1: rrf_step<DISC, CW, 1>(xc, PW, a, lst + t, w + t * CW, sa, sca); break;
      case 2: rrf_step<DISC, CW, 2>(xc, PW, a, lst + t, w + t * CW, sa, sca); break;
      case 3: rrf_step<DISC, CW, 3>(xc, PW, a, lst + t, w + t * CW, sa, sca); break;
      default: break;
    }
  }
}

// Grid as k_rf_stir: (PW / 64 feature blocks, row blocks of kRfRows focal
// rows), 4 waves per workgroup, lane = feature; a feature block is wholly
// continuous or wholly discrete (PC is a multiple of 64).  Per focal row one
// load of a, per neighbour one coalesced 256-byte gather of its row of xs and
// one scalar load of its CW weights (k_rrf_dy's).  1 + CW float64
// accumulators per lane; the four waves' are added through LDS in wave order
// (wave w folds the quantities w, w + 4, ...) into
// part[(q * nrb + row block) * PW + c], q = 0 for S_A (written when want_sa:
// the first chunk of a call) and 1 + t for target t of the chunk.  No
// atomics.  One class: nbr / nfound have one list per row.
template <int CW>
__global__ __launch_bounds__(256) void k_rrf_update(const float* __restrict__ xs, int64_t r_lo,
                                                    int64_t r_hi, int64_t PW, int64_t PC,
                                                    int64_t k, const int32_t* __restrict__ nbr,
                                                    const int32_t* __restrict__ nfound,
                                                    const double* __restrict__ dy, int want_sa,
                                                    int64_t nrb, double* __restrict__ part) {
  __shared__ double red[1 + CW][4][64];  // [quantity][wave][lane]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t c = (int64_t)blockIdx.x * 64 + lane;
  const bool disc = (int64_t)blockIdx.x * 64 >= PC;
  const int64_t b0 = r_lo + (int64_t)blockIdx.y * kRfRows;
  double sa = 0.0, sca[CW];
#pragma unroll
  for (int t = 0; t < CW; t++) sca[t] = 0.0;
  if (disc) rrf_rows<true, CW>(xs + c, PW, r_lo, b0, r_hi, wave, k, nbr, nfound, dy, sa, sca);
  else rrf_rows<false, CW>(xs + c, PW, r_lo, b0, r_hi, wave, k, nbr, nfound, dy, sa, sca);
  red[0][wave][lane] = sa;
#pragma unroll
  for (int t = 0; t < CW; t++) red[1 + t][wave][lane] = sca[t];
  __syncthreads();
  for (int q = wave; q < 1 + CW; q += 4) {
    if (q == 0 && !want_sa) continue;
    double v = 0.0;
#pragma unroll
    for (int w = 0; w < 4; w++) v += red[q][w][lane];
    part[((int64_t)q * nrb + blockIdx.y) * PW + c] = v;
  }
}

// S_C of the chunk's targets: workgroup t sums target t's dy over the pairs
// of the focal rows.  Pair e goes to thread (e mod 1024) whatever the chunk
// width, the thread partials are folded by a fixed LDS tree: a target's bits
// do not depend on its chunk.
__global__ __launch_bounds__(1024) void k_rrf_sc(const double* __restrict__ dy, int64_t np,
                                                 int cw, double* __restrict__ s_c) {
  __shared__ double red[1024];
  const int t = blockIdx.x;
  double s = 0.0;
  for (int64_t e = threadIdx.x; e < np; e += 1024) s += dy[e * cw + t];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = 512; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) s_c[t] = red[0];
}

int plan_score_targets(Plan* g, const double* u, int64_t B, double* s_a_dev, double* s_ca_dev,
                       double* s_c_dev) {
  FS_HIP(hipSetDevice(g->device));
  const Prepared& Q = g->P;
  const int64_t n = Q.n, k = Q.k_neighbors, nk = Q.n_kept;
  if (Q.algo != ALGO_RELIEFF || Q.n_classes != 1 || Q.ref_accum || k < 1 || k > n - 1 || B < 1) {
    set_error("fs_plan_score_targets: a one-class ReliefF plan in fast accumulation with "
              "1 <= k <= n - 1, and B >= 1");
    return FS_EINVAL;
  }
  if (!g->mem_call.blocks.empty()) {  // a call on a caller's stream keeps its buffers
    FS_HIP(hipStreamSynchronize(g->stream));
    g->mem_call.release();
  }
  g->rrf_chunks = -1;
  // chunks of kRrfChunk targets; a single last target runs at width 1
  struct Chunk {
    int64_t b0;
    int nb, cw;
  };
  std::vector<Chunk> chunks;
  for (int64_t b0 = 0; b0 < B; b0 += kRrfChunk) {
    const int nb = (int)std::min<int64_t>(kRrfChunk, B - b0);
    chunks.push_back({b0, nb, nb == 1 ? 1 : kRrfChunk});
  }
  const int nch = (int)chunks.size();
  for (hipEvent_t& e : g->ev_rrf_sel)
    if (!e && !(e = event_get(g->device, true))) return FS_EHIP;
  while ((int)g->ev_rrf.size() < 2 * nch) {
    hipEvent_t e = event_get(g->device, true);
    if (!e) return FS_EHIP;
    g->ev_rrf.push_back(e);
  }
  // every chunk's u as [n][cw] (zero beyond the chunk's targets), one upload
  std::vector<double> hu((size_t)nch * n * kRrfChunk, 0.0);
  for (int c = 0; c < nch; c++) {
    double* dst = hu.data() + (size_t)c * n * kRrfChunk;
    for (int t = 0; t < chunks[c].nb; t++) {
      const double* src = u + (chunks[c].b0 + t) * n;
      for (int64_t i = 0; i < n; i++) dst[i * chunks[c].cw + t] = src[i];
    }
  }
  const int64_t nrb = std::max<int64_t>(1, (g->r_hi - g->r_lo + kRfRows - 1) / kRfRows);
  const int64_t cc = n;  // the one class holds every sample
  DevArena& M = g->mem_call;
  const int64_t np = std::max<int64_t>(g->r_hi - g->r_lo, 0) * k;  // pairs of the focal rows
  double *du = nullptr, *part = nullptr, *dy = nullptr;
  int64_t* dcc = nullptr;
  int32_t *nbr = nullptr, *nfound = nullptr;
  int rc;
  if ((rc = M.alloc(&du, hu.size())) || (rc = M.alloc(&part, (size_t)(1 + kRrfChunk) * nrb * Q.PW)) ||
      (rc = M.alloc(&dy, (size_t)std::max<int64_t>(np, 1) * kRrfChunk)) ||
      (rc = M.alloc(&dcc, 1)) || (rc = M.alloc(&nbr, (size_t)n * k)) ||
      (rc = M.alloc(&nfound, (size_t)n)) || (rc = h2d(g, dcc, &cc, 1)) ||
      (rc = h2d(g, du, hu.data(), hu.size())) || (rc = run_quantize_dist(g))) {
    (void)hipStreamSynchronize(g->stream);  // hu and cc leave scope
    M.release();
    return rc;
  }
  auto body = [&]() -> int {
    FS_HIP(hipEventRecord(g->ev_rrf_sel[0], g->stream));
    FS_TRY(relieff_select(g, dcc, nbr, nfound));
    FS_HIP(hipEventRecord(g->ev_rrf_sel[1], g->stream));
    FS_HIP(hipMemsetAsync(s_a_dev, 0, sizeof(double) * nk, g->stream));
    FS_HIP(hipMemsetAsync(s_ca_dev, 0, sizeof(double) * B * nk, g->stream));
    const dim3 grid((unsigned)(Q.PW / 64), (unsigned)nrb);
    for (int c = 0; c < nch; c++) {
      const Chunk& ch = chunks[c];
      const double* uc = du + (size_t)c * n * kRrfChunk;
      if (np > 0) {
        k_rrf_dy<<<(unsigned)((np + 255) / 256), 256, 0, g->stream>>>(nbr, nfound, k, g->r_lo,
                                                                      g->r_hi, uc, ch.cw, dy);
        FS_TRY(launch_check("k_rrf_dy"));
      }
      k_rrf_sc<<<ch.nb, 1024, 0, g->stream>>>(dy, np, ch.cw, s_c_dev + ch.b0);
      FS_TRY(launch_check("k_rrf_sc"));
      FS_HIP(hipEventRecord(g->ev_rrf[2 * c], g->stream));
      if (ch.cw == 1)
        k_rrf_update<1><<<grid, 256, 0, g->stream>>>(g->xs, g->r_lo, g->r_hi, Q.PW, Q.PC, k, nbr,
                                                     nfound, dy, c == 0, nrb, part);
      else
        k_rrf_update<kRrfChunk><<<grid, 256, 0, g->stream>>>(g->xs, g->r_lo, g->r_hi, Q.PW, Q.PC,
                                                             k, nbr, nfound, dy, c == 0, nrb,
                                                             part);
      FS_TRY(launch_check("k_rrf_update"));
      FS_HIP(hipEventRecord(g->ev_rrf[2 * c + 1], g->stream));
      if (c == 0) FS_TRY(reduce_segments(part, nrb, Q.PW, g->out_pos, s_a_dev, g->stream));
      for (int t = 0; t < ch.nb; t++)
        FS_TRY(reduce_segments(part + (size_t)(1 + t) * nrb * Q.PW, nrb, Q.PW, g->out_pos,
                               s_ca_dev + (size_t)(ch.b0 + t) * nk, g->stream));
    }
    return FS_OK;
  };
  rc = body();
  if (hipStreamSynchronize(g->stream) != hipSuccess && rc == FS_OK) {
    set_error(std::string("fs_plan_score_targets: ") + hipGetErrorString(hipGetLastError()));
    rc = FS_EHIP;
  }
  M.release();
  if (rc == FS_OK) g->rrf_chunks = nch;
  return rc;
}

double plan_targets_kernel_ms(const Plan* g, int which) {
  if (g->rrf_chunks < 0 || which < 0 || which > 1) return -1.0;
  float ms = -1.0f;
  if (which == 0) {
    if (hipEventSynchronize(g->ev_rrf_sel[1]) != hipSuccess ||
        hipEventElapsedTime(&ms, g->ev_rrf_sel[0], g->ev_rrf_sel[1]) != hipSuccess) {
      (void)hipGetLastError();
      return -1.0;
    }
    return (double)ms;
  }
  double total = 0.0;
  for (int c = 0; c < g->rrf_chunks; c++) {
    if (hipEventSynchronize(g->ev_rrf[2 * c + 1]) != hipSuccess ||
        hipEventElapsedTime(&ms, g->ev_rrf[2 * c], g->ev_rrf[2 * c + 1]) != hipSuccess) {
      (void)hipGetLastError();
      return -1.0;
    }
    total += (double)ms;
  }
  return total;
}

int rrelieff_run(const Prepared& P, const void* x, int device, const double* u, int64_t B,
                 float* scores_out) {
  Plan* g = nullptr;
  FS_TRY(plan_create(&g, P, x, 0, device, 0, 1, 0, 0, P.n));
  const int64_t nk = P.n_kept;
  std::vector<double> host((size_t)(nk + B * nk + B));
  double* out = nullptr;
  int rc = g->mem_plan.alloc(&out, host.size());
  if (rc == FS_OK) rc = plan_score_targets(g, u, B, out, out + nk, out + nk + B * nk);
  if (rc == FS_OK &&
      hipMemcpy(host.data(), out, sizeof(double) * host.size(), hipMemcpyDeviceToHost) !=
          hipSuccess) {
    (void)hipGetLastError();
    set_error("fs_rrelieff_score: copying the sums to the host failed");
    rc = FS_EHIP;
  }
  plan_destroy(g);
  if (rc != FS_OK) return rc;
  const double n_pairs = (double)P.n * (double)P.k_neighbors;
  for (int64_t b = 0; b < B; b++)
    rrelieff::scores(host.data(), host.data() + nk + b * nk, host[(size_t)(nk + B * nk + b)],
                     n_pairs, nk, scores_out + b * nk);
  return FS_OK;
}

}  // namespace gpu
}  // namespace fs
