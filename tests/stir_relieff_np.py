"""Float64 numpy model of STIR for ReliefF -- TEST INFRASTRUCTURE ONLY.

The definitions of fastselect_amd/csrc/fs_stir.h ("STIR for ReliefF")
restated on the ``relieff`` loop of ``oracle/relief_np.py``: the same
per-feature diffs (``_diff_rows``: the reference's float32 diffs widened to
float64), the same float32 keys with the focal key at inf, the same argsort
(stable by default; the caller passes ``oracle.numba_argsort`` where keys
tie) and each class's first k entries of it -- the focal sample excluded, so
the reference's self-hit is no pair -- with the four pooled sums per feature
in place of the weighted update.  The epilogue is ``stir_np.statistics``.
Nothing here calls the library.
"""
from __future__ import annotations

import numpy as np

from oracle import relief_np

from stir_np import statistics, t_tolerance  # noqa: F401  (the shared epilogue)


def preprocess(x, y, discrete_limit=10):
    """(y_enc int32, recip f32, is_discrete, class_probs f32) as ReliefF.fit
    derives them (ReliefF.py:366-380): ranges in float64, discrete and
    constant columns -> 1."""
    x64 = np.asarray(x, dtype=np.float64)
    isd = np.array([np.unique(x64[:, f]).size <= discrete_limit for f in range(x64.shape[1])])
    ranges = x64.max(0) - x64.min(0)
    ranges[isd] = 1.0
    ranges[ranges == 0] = 1.0
    labels, counts = np.unique(y, return_counts=True)
    y_enc = np.searchsorted(labels, y).astype(np.int32)
    return y_enc, (1.0 / ranges).astype(np.float32), isd, (counts / len(y)).astype(np.float32)


def neighbour_lists(x32, y_enc, recip, is_disc, k, i, argsort=None):
    """(d (n, p) float64, [list of class c for c in classes]) of focal sample i."""
    d = relief_np._diff_rows(x32, i, recip, is_disc)
    keys = d.sum(axis=1).astype(np.float32)
    keys[i] = np.inf
    order = np.argsort(keys, kind="stable") if argsort is None else argsort(keys)
    n_classes = int(y_enc.max()) + 1
    return d, [[int(j) for j in order if y_enc[j] == c and j != i][:k] for c in range(n_classes)]


def stir_sums(x32, y_enc, recip, is_disc, k, rows=None, argsort=None):
    """(sums[4, p], |H|, |M|) of the focal samples ``rows`` (default all):
    S1H, S2H, S1M, S2M over the ordered (focal, neighbour) pairs."""
    n, p = x32.shape
    lo, hi = (0, n) if rows is None else rows
    sums = np.zeros((4, p), dtype=np.float64)
    n_hit = n_miss = 0
    for i in range(lo, hi):
        d, lists = neighbour_lists(x32, y_enc, recip, is_disc, k, i, argsort)
        for c, lst in enumerate(lists):
            q = 0 if c == y_enc[i] else 2
            sums[q] += d[lst].sum(axis=0)
            sums[q + 1] += (d[lst] ** 2).sum(axis=0)
            if q == 0:
                n_hit += len(lst)
            else:
                n_miss += len(lst)
    return sums, n_hit, n_miss


def three_class_case(seed=1):
    """300 x 40 mixed columns as ``stir_np.mixed_case`` with y in {0, 1, 2}:
    class 2 has 4 members (fewer than k = 5 others: its hit lists hold 3, the
    reference's self-hit excluded)."""
    import stir_np
    x, y = stir_np.mixed_case(seed=seed)
    y = y.astype(np.int64)
    y[[7, 90, 131, 299]] = 2
    return x, y
