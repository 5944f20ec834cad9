// fs_surf_labels_cpu.cpp -- the SURF / SURF* permutation test on the CPU
// backend: the score sums of B labellings of one problem's samples (GPU
// stage: fs_surf_labels.hip).
//
// SURF's near sets N_i = { j != i : (double)(float)D_ij < avg_i } never read
// the labels, so the pass-2 operands, the float32 distances and the means
// (surf_shared) serve every labelling.  Per labelling the labels of a copy of
// the problem are swapped and surf_run's own pair loop and weighted sum
// (surf_fast_sums) run on them: row b is bit for bit what surf_run returns
// for a problem with labelling b as y, star or not.  Labels are compared by
// equality only: any codes, any number of classes, any n.
#include <vector>

#include "../../include/fastselect_amd.h"
#include "fs_internal.h"

namespace fs {
namespace cpu {

int surf_score_labels(const Prepared& P, const void* x, const int32_t* labels, int64_t B,
                      int n_jobs, double* scores, int64_t* info) {
  const int64_t n = P.n;
  SurfShared S;
  surf_shared(P, x, n_jobs, 0, n, S);
  if (info) {  // the pairs with a near side, the near sides, the labellings walked, no star walk
    info[0] = info[1] = 0;
    for (int64_t i = 0; i < n; i++)
      for (int64_t j = i + 1; j < n; j++) {
        const double df = (double)S.Df[(size_t)i * n + j];
        const int c = (df < S.avg[i] ? 1 : 0) + (df < S.avg[j] ? 1 : 0);
        info[0] += c != 0;
        info[1] += c;
      }
    info[2] = B;
    info[3] = 0;
  }
  Prepared Q = P;
  for (int64_t b = 0; b < B; b++) {
    Q.labels.assign(labels + b * n, labels + (b + 1) * n);
    const int rc = surf_fast_sums(Q, S, n_jobs, 0, n, scores + b * P.n_kept);
    if (rc != FS_OK) return rc;
  }
  return FS_OK;
}

}  // namespace cpu
}  // namespace fs
