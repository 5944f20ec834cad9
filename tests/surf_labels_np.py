"""Float64 numpy model of SURF / SURF* scores under many labellings -- TEST
INFRASTRUCTURE ONLY.

The near sets are decided as ``oracle/relief_np.surf`` decides them: the
per-feature diffs are its ``_diff_rows`` (imported), a distance is the float32
of their float64 sum, the mean is the float32 sequential sum of a row's
distances divided by n - 1 in float64, and j is near i when
(double)(float)D_ij < avg_i.  ``relief_np.surf`` keeps that inside one loop and
offers no hook for it, so the three lines are repeated here and the tests hold
the model to ``relief_np.surf`` itself on labellings of their cases.  The per
pair terms are the float32-stored diffs widened to float64, as there.

Per labelling the four non-cancelling sums a score is made of are kept apart
(sums over the samples: not divided by n):

    NearMiss_f, NearHit_f, FarMiss_f, FarHit_f = the sums of d_f(i, j) over the
    ordered pairs (i, j != i) with j near / far of i and labelled differently /
    equally

    SURF  score_f = NearMiss_f - NearHit_f
    SURF* score_f = NearMiss_f - NearHit_f + FarHit_f - FarMiss_f

The near sets do not depend on the labels, so one pass over the samples serves
every labelling.  Nothing here calls the library.
"""
from __future__ import annotations

import numpy as np

from multisurf_labels_np import labellings  # noqa: F401  (the 37 labellings the tests use)
from oracle import relief_np
from stir_np import mixed_case  # noqa: F401  (the cases the tests use)


def preprocess(x64, discrete_limit=10):
    """(recip float32, is_discrete) as SURF.fit derives them (SURF.py:347-355)."""
    isd = np.array([np.unique(x64[:, f]).size <= discrete_limit for f in range(x64.shape[1])])
    ranges = x64.max(0) - x64.min(0)
    ranges[isd] = 1.0
    ranges[ranges == 0] = 1.0
    return (1.0 / ranges).astype(np.float32), isd


def near_sets(x64, recip, is_disc):
    """near[i, j]: j in N_i, the decisions of ``relief_np.surf``."""
    n = x64.shape[0]
    near = np.zeros((n, n), dtype=bool)
    for i in range(n):
        dist = relief_np._diff_rows(x64, i, recip, is_disc).sum(axis=1).astype(np.float32)
        dist[i] = 0.0
        s = np.float32(0.0)
        for v in dist:            # float32 sequential sum (SURF.py:162)
            s = np.float32(s + v)
        avg = float(s) / (n - 1)
        near[i] = dist.astype(np.float64) < avg
        near[i, i] = False
    return near


def score_parts(x64, labels, recip, is_disc):
    """(near_miss, near_hit, far_miss, far_hit), each (B, p) float64, and
    sum_i |N_i|, of the labellings ``labels`` ((n,) for one or (B, n))."""
    n, p = x64.shape
    lab = np.atleast_2d(np.asarray(labels))
    B = lab.shape[0]
    near = near_sets(x64, recip, is_disc)
    nm, nh, fm, fh = (np.zeros((B, p), dtype=np.float64) for _ in range(4))
    for i in range(n):
        d = relief_np._diff_rows(x64, i, recip, is_disc).astype(np.float32).astype(np.float64)
        others = np.arange(n) != i
        same = (lab == lab[:, i][:, None]) & others[None, :]       # (B, n)
        diff = (lab != lab[:, i][:, None])
        ni = near[i][None, :]
        nh += (same & ni).astype(np.float64) @ d
        nm += (diff & ni).astype(np.float64) @ d
        fh += (same & ~ni).astype(np.float64) @ d
        fm += (diff & ~ni).astype(np.float64) @ d
    return nm, nh, fm, fh, int(near.sum())


def scores(parts, use_star):
    """(score[B, p], the sum of the parts it is made of [B, p])."""
    nm, nh, fm, fh = parts[:4]
    if use_star:
        return nm - nh + fh - fm, nm + nh + fh + fm
    return nm - nh, nm + nh
