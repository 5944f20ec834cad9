// fs_labels_cpu.cpp -- the MultiSURF permutation test on the CPU backend:
// the score sums of B labellings on one plan's distances, thresholds and
// decisions (GPU stage and definitions: fs_labels.hip).
//
// Pass 1 and the select stage do not read the labels, so the CpuState of a
// plan serves every labelling.  Per labelling the labels of a copy of the
// problem are swapped and the plan's own count loop (multisurf_counts) and
// pass 2 (multisurf_pass2) run on them: row b is bit for bit what a plan
// created with labelling b as y returns from its pass 2.
#include <vector>

#include "../../include/fastselect_amd.h"
#include "fs_internal.h"

namespace fs {
namespace cpu {

int multisurf_score_labels(const Prepared& P, const void* x, const CpuState& S,
                           const int32_t* labels, int64_t B, int n_jobs, double* scores) {
  const int64_t n = P.n;
  if (S.D.size() != (size_t)n * n || S.thr.size() != (size_t)n) {
    set_error("fs_plan_score_labels: the plan holds no distances (run pass1 and select first)");
    return FS_EINVAL;
  }
  Prepared Q = P;
  std::vector<double> counts((size_t)2 * n);
  for (int64_t b = 0; b < B; b++) {
    Q.labels.assign(labels + b * n, labels + (b + 1) * n);
    multisurf_counts(Q, 0, 1, n_jobs, S, counts.data());
    const int rc =
        multisurf_pass2(Q, x, S, counts.data(), 0, 1, n_jobs, 0, n, scores + b * P.n_kept);
    if (rc != FS_OK) return rc;
  }
  return FS_OK;
}

}  // namespace cpu
}  // namespace fs
