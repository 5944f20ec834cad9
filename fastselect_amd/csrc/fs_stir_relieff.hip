// fs_stir_relieff.hip -- the STIR sums of a ReliefF plan on the GPU
// (definitions: fs_stir.h, "STIR for ReliefF"): per feature the sum of diff
// and of diff^2 over the nearest-hit pairs and over the nearest-miss pairs of
// the plan's focal rows.  One extra gather over what relieff_select left in
// the call arena (the neighbour lists nbr / nfound) and the pass-2 operands
// xs; k_rf_update and the reference-order path are not touched.
// Shared state and helpers: fs_gpu_internal.h.
#include "fs_gpu_internal.h"
#include "fs_stir.h"

namespace fs {
namespace gpu {

// Neighbours gathered per step of the list walk: their indices are
// wave-uniform (scalar loads), so the kRfStirUnroll row gathers of a step are
// all in flight before the first is used.
constexpr int kRfStirUnroll = 4;

// N neighbours lst[0..N) of a focal row into (s1, s2), the sum of the diffs
// and of their squares, in list order: N indices, then N row gathers, then
// the terms -- nothing conditional in between, so the gathers stay together.
// Discrete features count mismatches into s1 only.
template <bool DISC, int N>
__device__ __forceinline__ void rf_stir_step(const float* __restrict__ xc, int64_t PW, float a,
                                             const int32_t* __restrict__ lst, double& s1,
                                             double& s2) {
  int32_t j[N];
  float b[N];
#pragma unroll
  for (int u = 0; u < N; u++) j[u] = __builtin_amdgcn_readfirstlane(lst[u]);
#pragma unroll
  for (int u = 0; u < N; u++) b[u] = xc[(int64_t)j[u] * PW];
#pragma unroll
  for (int u = 0; u < N; u++) {
    if (DISC) {
      s1 += (a != b[u]) ? 1.0 : 0.0;
    } else {
      const double d = (double)__builtin_fabsf(a - b[u]);
      s1 += d;
      s2 = __builtin_fma(d, d, s2);
    }
  }
}

// One neighbour list of focal row i: whole steps of kRfStirUnroll, then the
// ragged rest (1 .. kRfStirUnroll - 1 neighbours) on a wave-uniform switch.
template <bool DISC>
__device__ __forceinline__ void rf_stir_list(const float* __restrict__ xc, int64_t PW, float a,
                                             const int32_t* __restrict__ lst, int32_t found,
                                             double& s1, double& s2) {
  static_assert(kRfStirUnroll == 4, "the switch below lists the rests of steps of 4");
  int32_t t = 0;
  for (; t + kRfStirUnroll <= found; t += kRfStirUnroll)
    rf_stir_step<DISC, kRfStirUnroll>(xc, PW, a, lst + t, s1, s2);
  switch (found - t) {
    case 1: rf_stir_step<DISC, 1>(xc, PW, a, lst + t, s1, s2); break;
    case 2: rf_stir_step<DISC, 2>(xc, PW, a, lst + t, s1, s2); break;
    case 3: rf_stir_step<DISC, 3>(xc, PW, a, lst + t, s1, s2); break;
    default: break;
  }
}

// The focal rows b0 + wave, b0 + wave + 4, ... of one row block for one lane's
// feature: acc[0..1] over the hit lists, acc[2..3] over the miss lists.  A
// class's list is wholly one or the other, so the choice is one wave-uniform
// branch per list.
template <bool DISC>
__device__ __forceinline__ void rf_stir_rows(const float* __restrict__ xc, int64_t PW, int64_t b0,
                                             int64_t r_hi, int wave,
                                             const int32_t* __restrict__ lab, int n_classes,
                                             int64_t k, const int32_t* __restrict__ nbr,
                                             const int32_t* __restrict__ nfound,
                                             double (&acc)[4]) {
  for (int64_t i = b0 + wave; i < r_hi && i < b0 + kRfRows; i += 4) {
    const int32_t li = __builtin_amdgcn_readfirstlane(lab[i]);
    const float a = xc[i * PW];
    for (int cl = 0; cl < n_classes; cl++) {
      const int32_t found = __builtin_amdgcn_readfirstlane(nfound[i * n_classes + cl]);
      if (found <= 0) continue;
      const int32_t* __restrict__ lst = nbr + (i * n_classes + cl) * k;
      double s1 = 0.0, s2 = 0.0;
      rf_stir_list<DISC>(xc, PW, a, lst, found, s1, s2);
      if (cl == li) {
        acc[0] += s1;
        acc[1] += s2;
      } else {
        acc[2] += s1;
        acc[3] += s2;
      }
    }
  }
}

// Grid as k_rf_update (fs_relieff.hip): (PW / 64 feature blocks, row blocks
// of kRfRows focal rows), 4 waves per workgroup, lane = feature; a feature
// block is wholly continuous or wholly discrete (PC is a multiple of 64).
// Per focal row one load of a, per neighbour one coalesced 256-byte gather of
// its row of xs.  Four float64 accumulators per lane; the four waves' are
// added through LDS in wave order (wave q folds quantity q) into
// part[(q * nrb + row block) * PW + c].  No atomics: a call is reproducible
// bit for bit.  A discrete block's sums of squares are copies of its sums
// (diff^2 == diff).
__global__ __launch_bounds__(256) void k_rf_stir(const float* __restrict__ xs, int64_t r_lo,
                                                 int64_t r_hi, int64_t PW, int64_t PC,
                                                 const int32_t* __restrict__ lab, int n_classes,
                                                 int64_t k, const int32_t* __restrict__ nbr,
                                                 const int32_t* __restrict__ nfound,
                                                 int64_t nrb, double* __restrict__ part) {
  __shared__ double red[4][4][64];  // [quantity][wave][lane]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t c = (int64_t)blockIdx.x * 64 + lane;
  const bool disc = (int64_t)blockIdx.x * 64 >= PC;
  const int64_t b0 = r_lo + (int64_t)blockIdx.y * kRfRows;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (disc) {
    rf_stir_rows<true>(xs + c, PW, b0, r_hi, wave, lab, n_classes, k, nbr, nfound, acc);
    acc[1] = acc[0];
    acc[3] = acc[2];
  } else {
    rf_stir_rows<false>(xs + c, PW, b0, r_hi, wave, lab, n_classes, k, nbr, nfound, acc);
  }
#pragma unroll
  for (int q = 0; q < 4; q++) red[q][wave][lane] = acc[q];
  __syncthreads();
  double v = 0.0;
#pragma unroll
  for (int u = 0; u < 4; u++) v += red[wave][u][lane];
  part[((int64_t)wave * nrb + blockIdx.y) * PW + c] = v;
}

// |H| and |M| of the focal rows: the lengths of each row's own-class list and
// of its other lists.  One workgroup; integer sums (exact in any order),
// thread partials folded by a fixed LDS tree, written as doubles.
__global__ __launch_bounds__(256) void k_rf_stir_counts(const int32_t* __restrict__ lab,
                                                        const int32_t* __restrict__ nfound,
                                                        int n_classes, int64_t r_lo, int64_t r_hi,
                                                        double* __restrict__ counts) {
  __shared__ unsigned long long red[2][256];
  unsigned long long nh = 0ull, nm = 0ull;
  for (int64_t i = r_lo + threadIdx.x; i < r_hi; i += 256) {
    const int32_t li = lab[i];
    for (int cl = 0; cl < n_classes; cl++) {
      const int32_t f = nfound[i * n_classes + cl];
      if (f <= 0) continue;
      if (cl == li) nh += (unsigned long long)f;
      else nm += (unsigned long long)f;
    }
  }
  red[0][threadIdx.x] = nh;
  red[1][threadIdx.x] = nm;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    counts[0] = (double)red[0][0];
    counts[1] = (double)red[1][0];
  }
}

int relieff_stir_sums(Plan* g, const int32_t* nbr, const int32_t* nfound, double* stir_dev,
                      double* counts_dev) {
  const Prepared& Q = g->P;
  const int C = Q.n_classes;
  const int64_t k = std::max<int64_t>(Q.k_neighbors, 1);  // nbr's pitch
  const int64_t nrb = std::max<int64_t>(1, (g->r_hi - g->r_lo + kRfRows - 1) / kRfRows);
  for (hipEvent_t& e : g->ev_rf_stir)
    if (!e && !(e = event_get(g->device, true))) return FS_EHIP;
  double* part = nullptr;
  FS_TRY(g->mem_call.alloc(&part, (size_t)4 * nrb * Q.PW));
  k_rf_stir_counts<<<1, 256, 0, g->stream>>>(g->lab, nfound, C, g->r_lo, g->r_hi, counts_dev);
  FS_TRY(launch_check("k_rf_stir_counts"));
  FS_HIP(hipEventRecord(g->ev_rf_stir[0], g->stream));
  k_rf_stir<<<dim3((unsigned)(Q.PW / 64), (unsigned)nrb), 256, 0, g->stream>>>(
      g->xs, g->r_lo, g->r_hi, Q.PW, Q.PC, g->lab, C, k, nbr, nfound, nrb, part);
  FS_TRY(launch_check("k_rf_stir"));
  FS_HIP(hipEventRecord(g->ev_rf_stir[1], g->stream));
  g->rf_stir_timed = true;
  FS_HIP(hipMemsetAsync(stir_dev, 0, sizeof(double) * 4 * Q.n_kept, g->stream));
  for (int q = 0; q < 4; q++)
    FS_TRY(reduce_segments(part + (size_t)q * nrb * Q.PW, nrb, Q.PW, g->out_pos,
                           stir_dev + (size_t)q * Q.n_kept, g->stream));
  return FS_OK;
}

}  // namespace gpu
}  // namespace fs
