// fs_surf_labels.hip -- the SURF / SURF* permutation test on the GPU: the
// score sums of B labellings of a SURF plan's samples on one distance stage.
//
// SURF's near sets N_i = { j != i : (double)(float)D_ij < avg_i } never read
// the labels, and a near side weighs -1 for a hit and +1 for a miss: no
// per-sample counts at all.  With s_b(i, j) = +1 where labelling b labels i
// and j differently, -1 where equally, and c_ij = near_i(j) + near_j(i),
//
//   S_surf[f, b] = sum over i < j of s_b(i, j) c_ij d_f(i, j)
//   S_star[f, b] = 2 S_surf[f, b] - 2 (T_f - 2 Hs[f, b])
//   T_f = sum over i < j of d_f(i, j)                       (no labels)
//   Hs[f, b] = the same over the pairs of one class under b (fs_starterm.hip)
//
// the split in the header of fs_starterm.hip (alpha = 1, gamma = 2) written
// per labelling.  Once per call: the plan's own distance stage
// (surf_distances: run_quantize_dist, then surf_resolve or k_surf_avg), the
// record stage of fs_labels.hip with SURF's decisions (lab_records) and, for
// SURF*, one sort of every scored column (star_lab_sort).  Per chunk of at
// most 32 labellings: k_lab_transpose, k_surf_lab_weights (W = s c: +-1 or
// +-2, 0 for padding), k_lab_score / k_lab_reduce as they stand, and for SURF*
// the walk over the sorted columns and its epilogue.  All buffers come from
// mem_call; one host synchronisation for the record count and one at the end.
// No float atomics: the same call gives the same bits twice.
#include "fs_gpu_internal.h"

namespace fs {
namespace gpu {

namespace {

constexpr int kSfB = 32;  // labellings per chunk (fs_labels.hip's kLabB)

// W[r * 32 + b] = (float)(s_b c) of record r = (i, j | flags << 30): c the
// near sides of the pair, s_b = -1 for a hit under labelling b of the chunk,
// +1 for a miss; 0 for padding records and padding labellings (b >= nb).
__global__ __launch_bounds__(256) void k_surf_lab_weights(const int2* __restrict__ rec,
                                                          int64_t nrec,
                                                          const int32_t* __restrict__ labT, int nb,
                                                          float* __restrict__ W) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r = g / kSfB;
  const int b = (int)(g % kSfB);
  if (r >= nrec) return;
  const int2 rc = rec[r];
  const uint32_t fl = (uint32_t)rc.y >> 30;
  float w = 0.0f;
  if (fl != 0u && b < nb) {
    const int64_t i = rc.x, j = rc.y & 0x3fffffff;
    const float c = (float)((fl & 1u) + (fl >> 1));
    w = labT[i * kSfB + b] == labT[j * kSfB + b] ? -c : c;
  }
  W[g] = w;
}

// xsT[c][i] = xs[i][c]: the feature-major pass-2 values of a plan in the
// dense star form (which keeps none), 32 x 32 tiles through LDS.
__global__ __launch_bounds__(256) void k_surf_lab_xsT(const float* __restrict__ xs, int64_t n_pad,
                                                      int64_t PW, float* __restrict__ xsT) {
  __shared__ float t[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t i0 = (int64_t)blockIdx.y * 32, c0 = (int64_t)blockIdx.x * 32;
  for (int k = ty; k < 32; k += 8) t[k][tx] = xs[(i0 + k) * PW + c0 + tx];
  __syncthreads();
  for (int k = ty; k < 32; k += 8) xsT[(c0 + k) * n_pad + i0 + tx] = t[tx][k];
}

// info[0] += the weighted pairs (wcnt), info[1] += the near sides (Nn);
// integer atomics: exact in any order.
__global__ __launch_bounds__(256) void k_surf_lab_info(const uint32_t* __restrict__ wcnt,
                                                       int64_t nw, const uint32_t* __restrict__ Nn,
                                                       int64_t n, unsigned long long* __restrict__ info) {
  __shared__ double red[256];
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  // counts below 2^53: exact as doubles in block_sum_256
  const double a = block_sum_256(g < nw ? (double)wcnt[g] : 0.0, red);
  const double b = block_sum_256(g < n ? (double)Nn[g] : 0.0, red);
  if (threadIdx.x == 0) {
    atomicAdd(&info[0], (unsigned long long)a);
    atomicAdd(&info[1], (unsigned long long)b);
  }
}

int surf_labels_events(Plan* g, size_t count) {
  while (g->ev_surf_labels.size() < count) {
    hipEvent_t e = event_get(g->device, true);
    if (!e) return FS_EHIP;
    g->ev_surf_labels.push_back(e);
  }
  return FS_OK;
}

}  // namespace

int plan_surf_score_labels(Plan* g, const int32_t* labels, int64_t B, double* scores) {
  const Prepared& Q = g->P;
  const int64_t n = Q.n;
  const bool star = Q.use_star != 0;
  FS_HIP(hipSetDevice(g->device));
  if (!g->mem_call.blocks.empty()) {  // a call on a caller's stream keeps its buffers
    FS_HIP(hipStreamSynchronize(g->stream));
    g->mem_call.release();
  }
  g->surf_labels_info[0] = -1;
  if (B <= 0) return FS_OK;
  if (g->n_tiles <= 0 || n >= (1 << 30)) {
    set_error("fs_plan_surf_score_labels: the plan owns no tiles, or n >= 2^30");
    return FS_ENOTSUP;
  }
  if (star) {
    // the walk's sizes: kStThreads * kStMaxIpt samples, kStMaxClasses packed counters
    if (!star_split_fits(n, 1)) {
      set_error("fs_plan_surf_score_labels: SURF* labellings on the GPU take 2 <= n <= 24576");
      return FS_ENOTSUP;
    }
    for (int64_t q = 0; q < B * n; q++)
      if (labels[q] < 0 || labels[q] >= 8) {
        set_error("fs_plan_surf_score_labels: SURF* labellings on the GPU take label codes in "
                  "[0, 8); labelling " + std::to_string(q / n) + " holds " +
                  std::to_string(labels[q]));
        return FS_ENOTSUP;
      }
  }
  int64_t chunk = kSfB;
  if (test_hooks().labels_chunk >= 1) chunk = std::min<int64_t>(kSfB, test_hooks().labels_chunk);
  const int64_t nchunks = (B + chunk - 1) / chunk;
  FS_TRY(surf_labels_events(g, (size_t)(4 + 6 * nchunks)));
  hipEvent_t* ev = g->ev_surf_labels.data();
  hipStream_t st = g->stream;
  DevArena& M = g->mem_call;
  // ---- once per call: distances, means, records
  FS_HIP(hipEventRecord(ev[0], st));
  FS_TRY(surf_distances(g));
  // SURF*'s own column terms (fork_star_terms, the side stream) read xsT too
  if (g->star_split) FS_HIP(hipStreamWaitEvent(st, g->ev_join, 0));
  uint32_t *wcnt = nullptr, *Nn = nullptr;
  int64_t* goff = nullptr;
  int2* rec = nullptr;
  int64_t nrec = 0;
  FS_TRY(lab_records(g, true, &wcnt, &goff, &Nn, &rec, &nrec));
  FS_HIP(hipEventRecord(ev[1], st));
  unsigned long long* dinfo = nullptr;
  FS_TRY(M.alloc(&dinfo, (size_t)2));
  FS_HIP(hipMemsetAsync(dinfo, 0, sizeof(unsigned long long) * 2, st));
  {
    const int64_t nw = 4 * g->n_tiles, span = std::max(nw, n);
    k_surf_lab_info<<<(unsigned)((span + 255) / 256), 256, 0, st>>>(wcnt, nw, Nn, n, dinfo);
    FS_TRY(launch_check("k_surf_lab_info"));
  }
  // ---- SURF*: one sort of every scored column
  float* sval = nullptr;
  uint16_t* sidx = nullptr;
  double *tcol = nullptr, *hs = nullptr;
  uint64_t *ncls = nullptr, *cnt = nullptr;
  int64_t seg_items = n, nsegS = 1;
  if (star) {
    const float* xsT = g->xsT;
    if (!xsT) {
      float* t = nullptr;
      FS_TRY(M.alloc(&t, (size_t)Q.PW * Q.n_pad));
      k_surf_lab_xsT<<<dim3((unsigned)(Q.PW / 32), (unsigned)(Q.n_pad / 32)), 256, 0, st>>>(
          g->xs, Q.n_pad, Q.PW, t);
      FS_TRY(launch_check("k_surf_lab_xsT"));
      xsT = t;
    }
    star_lab_split(g, &seg_items, &nsegS);
    FS_TRY(M.alloc(&sval, (size_t)Q.PW * Q.n_pad));
    FS_TRY(M.alloc(&sidx, (size_t)Q.PW * Q.n_pad));
    FS_TRY(M.alloc(&tcol, (size_t)Q.PW));
    FS_TRY(M.alloc(&hs, (size_t)Q.PW * nsegS * kSfB));
    FS_TRY(M.alloc(&ncls, (size_t)2 * kSfB));
    FS_TRY(M.alloc(&cnt, (size_t)4 * Q.PW * nsegS * kSfB));
    FS_HIP(hipEventRecord(ev[2], st));
    FS_TRY(star_lab_sort(g, xsT, sval, sidx, tcol, st));
    FS_HIP(hipEventRecord(ev[3], st));
  }
  // ---- the split of the score kernel, a chunk's buffers
  int64_t seg_len = 1, nseg = 1;
  lab_score_split(g, g->n_tiles, &seg_len, &nseg);
  int32_t *lab_raw = nullptr, *labT = nullptr;
  float* W = nullptr;
  double* part = nullptr;
  FS_TRY(M.alloc(&lab_raw, (size_t)chunk * n));
  FS_TRY(M.alloc(&labT, (size_t)kSfB * n));
  FS_TRY(M.alloc(&W, (size_t)std::max<int64_t>(nrec, 1) * kSfB));
  FS_TRY(M.alloc(&part, (size_t)chunk * nseg * Q.PW));
  for (int64_t c = 0; c < nchunks; c++) {
    const int64_t b0 = c * chunk;
    const int nb = (int)std::min(chunk, B - b0);
    hipEvent_t* e = ev + 4 + 6 * c;
    FS_HIP(hipMemcpyAsync(lab_raw, labels + b0 * n, sizeof(int32_t) * (size_t)nb * n,
                          hipMemcpyHostToDevice, st));
    FS_HIP(hipEventRecord(e[0], st));
    FS_TRY(lab_transpose(g, lab_raw, nb, labT));
    if (nrec > 0) {
      k_surf_lab_weights<<<(unsigned)((nrec * kSfB + 255) / 256), 256, 0, st>>>(rec, nrec, labT, nb,
                                                                               W);
      FS_TRY(launch_check("k_surf_lab_weights"));
    }
    FS_HIP(hipEventRecord(e[1], st));
    FS_HIP(hipEventRecord(e[2], st));
    FS_TRY(lab_score_reduce(g, rec, goff, W, g->n_tiles, seg_len, nseg, nb, part,
                            scores + b0 * Q.n_kept, e[3]));
    if (star) {
      FS_HIP(hipEventRecord(e[4], st));
      FS_TRY(star_lab_walk(g, sval, sidx, labT, nb, seg_items, nsegS, ncls, cnt, hs, st));
      FS_TRY(star_lab_apply(g, tcol, hs, nsegS, nb, scores + b0 * Q.n_kept, st));
      FS_HIP(hipEventRecord(e[5], st));
    }
  }
  unsigned long long hinfo[2] = {0, 0};
  FS_HIP(hipMemcpyAsync(hinfo, dinfo, sizeof(hinfo), hipMemcpyDeviceToHost, st));
  // the labels are host memory: the call ends when the device has finished
  FS_HIP(hipStreamSynchronize(st));
  M.release();
  auto span = [&](size_t a, size_t b) -> double {
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, ev[a], ev[b]) != hipSuccess) {
      (void)hipGetLastError();
      return -1.0;
    }
    return (double)ms;
  };
  double* ms = g->surf_labels_ms;
  ms[0] = span(0, 1);
  ms[1] = ms[2] = 0.0;
  ms[3] = star ? span(2, 3) : -1.0;
  for (int64_t c = 0; c < nchunks; c++) {
    const size_t e = 4 + 6 * (size_t)c;
    const double w = span(e, e + 1), s = span(e + 2, e + 3), t = star ? span(e + 4, e + 5) : 0.0;
    ms[1] = (ms[1] < 0.0 || w < 0.0) ? -1.0 : ms[1] + w;
    ms[2] = (ms[2] < 0.0 || s < 0.0) ? -1.0 : ms[2] + s;
    if (star) ms[3] = (ms[3] < 0.0 || t < 0.0) ? -1.0 : ms[3] + t;
  }
  g->surf_labels_info[1] = (int64_t)hinfo[1];
  g->surf_labels_info[2] = nchunks;
  g->surf_labels_info[3] = star ? 1 : 0;
  g->surf_labels_info[0] = (int64_t)hinfo[0];
  return FS_OK;
}

int plan_surf_labels_info(const Plan* g, int64_t* out4) {
  if (g->surf_labels_info[0] < 0) {
    set_error("fs_plan_surf_labels_info: no completed fs_plan_surf_score_labels call");
    return FS_EINVAL;
  }
  for (int q = 0; q < 4; q++) out4[q] = g->surf_labels_info[q];
  return FS_OK;
}

double plan_surf_labels_kernel_ms(const Plan* g, int which) {
  if (g->surf_labels_info[0] < 0 || which < 0 || which > 3) return -1.0;
  return g->surf_labels_ms[which];
}

int surf_labels_run(const Prepared& P, const void* x, int device, const int32_t* labels,
                    int64_t B, float* scores_out) {
  if (!rows_fit_one_plan(P, device)) {
    set_error("fs_surf_score_labels: the distance rows do not fit one plan (a plan that scores "
              "in row panels cannot score labellings)");
    return FS_ENOTSUP;
  }
  Plan* g = nullptr;
  FS_TRY(plan_create(&g, P, x, 1, device, 0, 1, 0, 0, P.n));
  double* out = nullptr;
  std::vector<double> host((size_t)B * P.n_kept);
  int rc = g->mem_plan.alloc(&out, host.size());
  if (rc == FS_OK) rc = plan_surf_score_labels(g, labels, B, out);
  if (rc == FS_OK &&
      hipMemcpy(host.data(), out, sizeof(double) * host.size(), hipMemcpyDeviceToHost) !=
          hipSuccess) {
    (void)hipGetLastError();
    set_error("fs_surf_score_labels: copying the scores to the host failed");
    rc = FS_EHIP;
  }
  plan_destroy(g);
  if (rc != FS_OK) return rc;
  for (size_t q = 0; q < host.size(); q++) scores_out[q] = (float)(host[q] / (double)P.n);
  return FS_OK;
}

}  // namespace gpu
}  // namespace fs
