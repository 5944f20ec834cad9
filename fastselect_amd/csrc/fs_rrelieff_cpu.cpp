// fs_rrelieff_cpu.cpp -- the RReliefF sums on the CPU backend (definitions:
// fs_rrelieff.h).
//
// The neighbour lists are relieff_neighbours' on the plan's one-class
// Prepared: the lists cpu::relieff_run weighs, computed once per call for any
// number of targets.  The sums follow cpu::relieff_stir's scheme: the focal
// rows are cut into chunks that depend on the row range alone, a chunk sums
// its pairs in (i, list) order and the chunks are added in chunk order, so
// the thread count does not change the bits.  Targets are walked in blocks of
// kBlock to bound the partials; a target's terms and their order do not
// depend on its block, so row b of any call has the bits of the B = 1 call.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <thread>
#include <vector>

#include "../../include/fastselect_amd.h"
#include "fs_rrelieff.h"
#include "fs_stir.h"

namespace fs {
namespace cpu {

namespace {
// chunks as fs_stir_cpu.cpp: at most kMaxChunks of at least kMinRows rows
constexpr int64_t kMaxChunks = 64, kMinRows = 16;
constexpr int64_t kBlock = 16;  // targets per walk of the lists
}  // namespace

int rrelieff_sums(const Prepared& P, const float* x, int n_jobs, int64_t r_lo, int64_t r_hi,
                  const double* u, int64_t B, double* s_a, double* s_ca, double* s_c) {
  const int64_t nk = P.n_kept, n = P.n;
  std::fill(s_a, s_a + nk, 0.0);
  std::fill(s_ca, s_ca + B * nk, 0.0);
  std::fill(s_c, s_c + B, 0.0);
  if (r_hi <= r_lo) return FS_OK;
  std::vector<std::vector<int32_t>> lists;
  relieff_neighbours(P, x, n_jobs, r_lo, r_hi, lists);
  const int64_t rows = r_hi - r_lo;
  const int64_t nchunk = std::min<int64_t>(kMaxChunks, (rows + kMinRows - 1) / kMinRows);
  const int64_t per = (rows + nchunk - 1) / nchunk;
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(hardware_threads(n_jobs), nchunk));
  // per chunk: [S_A | S_CA of the block's targets | S_C of the block's targets]
  const int64_t pitch = (1 + kBlock) * nk + kBlock;
  std::vector<double> part((size_t)(nchunk * pitch));
  std::vector<double> d((size_t)nt * nk);
  for (int64_t b0 = 0; b0 < B; b0 += kBlock) {
    const int64_t nb = std::min<int64_t>(kBlock, B - b0);
    const bool first = b0 == 0;  // S_A comes with the first block
    std::fill(part.begin(), part.end(), 0.0);
    auto chunk = [&](int64_t c, int w) {
      double* sa = part.data() + (size_t)(c * pitch);
      double* sca = sa + nk;
      double* sc = sa + (1 + kBlock) * nk;
      double* dv = d.data() + (size_t)w * nk;
      const int64_t i_lo = r_lo + c * per, i_hi = std::min(r_hi, i_lo + per);
      for (int64_t i = i_lo; i < i_hi; i++) {
        const float* xi = x + i * P.p_in;
        for (int32_t j : lists[(size_t)(i - r_lo)]) {
          const float* xj = x + (int64_t)j * P.p_in;
          for (int64_t k = 0; k < nk; k++) {
            const int64_t col = P.kept_col[k];
            const float v = P.disc_in[col] ? (xi[col] != xj[col] ? 1.0f : 0.0f)
                                           : std::fabs(xi[col] - xj[col]) * P.recip_in[col];
            dv[k] = (double)v;
          }
          if (first)
            for (int64_t k = 0; k < nk; k++) sa[k] += dv[k];
          for (int64_t q = 0; q < nb; q++) {
            const double* ub = u + (b0 + q) * n;
            const double dy = std::fabs(ub[i] - ub[j]);
            sc[q] += dy;
            double* row = sca + q * nk;
            for (int64_t k = 0; k < nk; k++) row[k] += dy * dv[k];
          }
        }
      }
    };
    if (nt <= 1) {
      for (int64_t c = 0; c < nchunk; c++) chunk(c, 0);
    } else {
      std::atomic<int64_t> next{0};
      std::vector<std::thread> th;
      th.reserve(nt);
      for (int w = 0; w < nt; w++)
        th.emplace_back([&, w]() {
          for (int64_t c = next++; c < nchunk; c = next++) chunk(c, w);
        });
      for (auto& t : th) t.join();
    }
    for (int64_t c = 0; c < nchunk; c++) {
      const double* sa = part.data() + (size_t)(c * pitch);
      if (first)
        for (int64_t k = 0; k < nk; k++) s_a[k] += sa[k];
      for (int64_t q = 0; q < nb; q++) {
        for (int64_t k = 0; k < nk; k++) s_ca[(b0 + q) * nk + k] += sa[(1 + q) * nk + k];
        s_c[b0 + q] += sa[(1 + kBlock) * nk + q];
      }
    }
  }
  return FS_OK;
}

}  // namespace cpu
}  // namespace fs
