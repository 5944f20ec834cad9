// fs_stir_cpu.cpp -- the STIR sums on the CPU backend (definitions: fs_stir.h).
//
// The near pairs are the CPU plan's own: D and thr of its CpuState, as its
// pass 2 reads them.  Each focal sample i of [r_lo, r_hi) contributes its
// side of every owned pair (i, j) with D_ij < thr_i; the diffs are the
// reference's float32 ones (MultiSURF.py:184-187), summed in float64.  The
// focal rows are cut into chunks that depend on the row range alone, each
// chunk sums its pairs in (i, j) order and the chunks are added in chunk
// order, so the result does not depend on n_jobs.  relieff_stir (below) sums
// the same way over ReliefF's neighbour lists.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <thread>
#include <vector>

#include "../../include/fastselect_amd.h"
#include "fs_stir.h"

namespace fs {
namespace cpu {

// at most kMaxChunks chunks (each holds 4 n_kept partial sums) of at least
// kMinRows focal rows: a function of the row range alone
constexpr int64_t kMaxChunks = 64, kMinRows = 16;

int multisurf_stir(const Prepared& P, const float* x, const CpuState& S, int rank, int world,
                   int n_jobs, int64_t r_lo, int64_t r_hi, double* sums) {
  const int64_t n = P.n, nk = P.n_kept, nb = P.n_pad / kTile;
  std::fill(sums, sums + 4 * nk, 0.0);
  if (r_hi <= r_lo) return FS_OK;
  if (S.D.size() != (size_t)n * n || S.thr.size() != (size_t)n) {
    set_error("fs_plan_stir: the plan holds no distances (run pass1 and select first)");
    return FS_EINVAL;
  }
  const int64_t rows = r_hi - r_lo;
  const int64_t nchunk = std::min<int64_t>(kMaxChunks, (rows + kMinRows - 1) / kMinRows);
  const int64_t per = (rows + nchunk - 1) / nchunk;
  std::vector<double> part((size_t)nchunk * 4 * nk, 0.0);
  auto chunk = [&](int64_t c) {
    double* s = part.data() + (size_t)c * 4 * nk;
    const int64_t i_lo = r_lo + c * per, i_hi = std::min(r_hi, i_lo + per);
    for (int64_t i = i_lo; i < i_hi; i++) {
      const float* xi = x + i * P.p_in;
      for (int64_t j = 0; j < n; j++) {
        if (j == i || !(S.D[(size_t)i * n + j] < S.thr[i])) continue;
        if (world > 1) {
          const int64_t a = std::min(i, j) / kTile, b = std::max(i, j) / kTile;
          if (tile_linear(nb, a, b) % world != rank) continue;
        }
        double* q = s + (P.labels[j] == P.labels[i] ? 0 : 2 * nk);
        const float* xj = x + j * P.p_in;
        for (int64_t k = 0; k < nk; k++) {
          const int64_t col = P.kept_col[k];
          const float d = P.disc_in[col] ? (xi[col] != xj[col] ? 1.0f : 0.0f)
                                         : std::fabs(xi[col] - xj[col]) * P.recip_in[col];
          q[k] += (double)d;
          q[nk + k] += (double)d * (double)d;
        }
      }
    }
  };
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(hardware_threads(n_jobs), nchunk));
  if (nt <= 1) {
    for (int64_t c = 0; c < nchunk; c++) chunk(c);
  } else {
    std::atomic<int64_t> next{0};
    std::vector<std::thread> th;
    th.reserve(nt);
    for (int w = 0; w < nt; w++)
      th.emplace_back([&]() {
        for (int64_t c = next++; c < nchunk; c = next++) chunk(c);
      });
    for (auto& t : th) t.join();
  }
  for (int64_t c = 0; c < nchunk; c++)
    for (int64_t k = 0; k < 4 * nk; k++) sums[k] += part[(size_t)c * 4 * nk + k];
  return FS_OK;
}

// STIR for ReliefF: the pairs are (i, j) with j in one of focal sample i's
// neighbour lists (relieff_neighbours: the lists relieff_run weighs), hits
// from the list of i's own class, misses pooled over the others.  The same
// chunk scheme as above: chunks of the row range, each summed in (i, class,
// list) order, added in chunk order.
int relieff_stir(const Prepared& P, const float* x, int n_jobs, int64_t r_lo, int64_t r_hi,
                 double* stir_sums, double* pair_counts) {
  const int64_t nk = P.n_kept;
  const int C = P.n_classes;
  std::fill(stir_sums, stir_sums + 4 * nk, 0.0);
  pair_counts[0] = pair_counts[1] = 0.0;
  if (r_hi <= r_lo) return FS_OK;
  std::vector<std::vector<int32_t>> lists;
  relieff_neighbours(P, x, n_jobs, r_lo, r_hi, lists);
  const int64_t rows = r_hi - r_lo;
  const int64_t nchunk = std::min<int64_t>(kMaxChunks, (rows + kMinRows - 1) / kMinRows);
  const int64_t per = (rows + nchunk - 1) / nchunk;
  std::vector<double> part((size_t)nchunk * 4 * nk, 0.0);
  auto chunk = [&](int64_t c) {
    double* s = part.data() + (size_t)c * 4 * nk;
    const int64_t i_lo = r_lo + c * per, i_hi = std::min(r_hi, i_lo + per);
    for (int64_t i = i_lo; i < i_hi; i++) {
      const float* xi = x + i * P.p_in;
      for (int cl = 0; cl < C; cl++) {
        double* q = s + (cl == P.labels[i] ? 0 : 2 * nk);
        for (int32_t j : lists[(size_t)(i - r_lo) * C + cl]) {
          const float* xj = x + (int64_t)j * P.p_in;
          for (int64_t k = 0; k < nk; k++) {
            const int64_t col = P.kept_col[k];
            const float d = P.disc_in[col] ? (xi[col] != xj[col] ? 1.0f : 0.0f)
                                           : std::fabs(xi[col] - xj[col]) * P.recip_in[col];
            q[k] += (double)d;
            q[nk + k] += (double)d * (double)d;
          }
        }
      }
    }
  };
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(hardware_threads(n_jobs), nchunk));
  if (nt <= 1) {
    for (int64_t c = 0; c < nchunk; c++) chunk(c);
  } else {
    std::atomic<int64_t> next{0};
    std::vector<std::thread> th;
    th.reserve(nt);
    for (int w = 0; w < nt; w++)
      th.emplace_back([&]() {
        for (int64_t c = next++; c < nchunk; c = next++) chunk(c);
      });
    for (auto& t : th) t.join();
  }
  for (int64_t c = 0; c < nchunk; c++)
    for (int64_t k = 0; k < 4 * nk; k++) stir_sums[k] += part[(size_t)c * 4 * nk + k];
  int64_t nh = 0, nm = 0;
  for (int64_t i = r_lo; i < r_hi; i++)
    for (int cl = 0; cl < C; cl++) {
      const int64_t f = (int64_t)lists[(size_t)(i - r_lo) * C + cl].size();
      if (cl == P.labels[i]) nh += f;
      else nm += f;
    }
  pair_counts[0] = (double)nh;
  pair_counts[1] = (double)nm;
  return FS_OK;
}

}  // namespace cpu
}  // namespace fs
