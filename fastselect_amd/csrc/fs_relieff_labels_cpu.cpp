// fs_relieff_labels_cpu.cpp -- the ReliefF permutation test on the CPU
// backend: the score sums of B labellings of one problem's samples (GPU
// stage: fs_relieff_labels.hip).
//
// ReliefF's neighbour sets read the labels, but what comes before them does
// not: the pass-2 operands, the quantised distances and the refinement band
// (relieff_shared) serve every labelling.  Per labelling the labels, the
// class count and the priors of a copy of the problem are swapped and the
// plan's own selection and update (relieff_fast_sums) run on them: row b is
// bit for bit what relieff_run returns for a problem with labelling b as y.
#include <vector>

#include "../../include/fastselect_amd.h"
#include "fs_internal.h"

namespace fs {
namespace cpu {

int relieff_score_labels(const Prepared& P, const void* x, const int32_t* labels, int64_t B,
                         int n_jobs, double* scores) {
  const int64_t n = P.n;
  Prepared Q = P;
  // every labelling is checked before any is scored
  for (int64_t b = 0; b < B; b++)
    if (const int bad = relieff_set_labelling(Q, labels + b * n)) {
      set_error("ReliefF labellings: labelling " + std::to_string(b) +
                (bad == 1 ? " holds a class code outside [0, 64)"
                          : " has fewer than 2 classes"));
      return FS_EINVAL;
    }
  RelieffShared S;
  relieff_shared(P, x, n_jobs, S);
  for (int64_t b = 0; b < B; b++) {
    relieff_set_labelling(Q, labels + b * n);
    const int rc = relieff_fast_sums(Q, x, S, n_jobs, 0, n, scores + b * P.n_kept);
    if (rc != FS_OK) return rc;
  }
  return FS_OK;
}

}  // namespace cpu
}  // namespace fs
