"""Float64 numpy model of MultiSURF scores under many labellings -- TEST
INFRASTRUCTURE ONLY.

The ``multisurf`` loop of ``oracle/relief_np.py`` (the same per-feature diffs,
``_diff_rows``: the reference's float32 diffs widened to float64; the same
distances, thresholds D_ij < mu_i - sigma_i / 2 and near sets, all float64)
with the two sums a score is made of kept apart, per labelling:

    Miss_f = sum_i (1 / M_i) sum over the near misses of i of d_f
    Hit_f  = sum_i (1 / H_i) sum over the near hits of i of d_f
    score_f = Miss_f - Hit_f        (a sum over the samples: not divided by n)

A sample without near hits (H_i = 0) has no hit term, one without near misses
no miss term.  The near sets do not depend on the labels, so one pass over the
samples serves every labelling.  Nothing here calls the library.
"""
from __future__ import annotations

import numpy as np

from oracle import relief_np
from stir_np import mixed_case, preprocess  # noqa: F401  (the cases the tests use)


def score_parts(x32, labels, recip, is_disc):
    """(miss[B, p], hit[B, p], score[B, p], counts[B, n, 2]) of the labellings
    ``labels`` ((n,) for one labelling or (B, n)), float64; counts[b, i] =
    (H_i, M_i) under labelling b."""
    n, p = x32.shape
    lab = np.atleast_2d(np.asarray(labels))
    B = lab.shape[0]
    miss = np.zeros((B, p), dtype=np.float64)
    hit = np.zeros((B, p), dtype=np.float64)
    counts = np.zeros((B, n, 2), dtype=np.int64)
    for i in range(n):
        d = relief_np._diff_rows(x32, i, recip, is_disc)     # (n, p) float64
        dist = d.sum(axis=1)
        others = np.arange(n) != i
        mu = dist[others].sum() / (n - 1)
        var = max(0.0, (dist[others] ** 2).sum() / (n - 1) - mu * mu)
        near = (dist < mu - 0.5 * np.sqrt(var)) & others
        dn = d[near]                                          # (|N_i|, p)
        same = lab[:, near] == lab[:, i][:, None]             # (B, |N_i|)
        h = same.sum(axis=1)
        m = (~same).sum(axis=1)
        counts[:, i, 0], counts[:, i, 1] = h, m
        with np.errstate(divide="ignore"):
            wh = np.where(same, 1.0 / np.maximum(h, 1)[:, None], 0.0)
            wm = np.where(~same, 1.0 / np.maximum(m, 1)[:, None], 0.0)
        hit += wh @ dn
        miss += wm @ dn
    return miss, hit, miss - hit, counts


def labellings(y, seed=1):
    """The 37 labellings of the GPU tests (one full chunk of 32 and a ragged
    one): y, 32 permutations of y, a 3-class labelling, a permutation of it, a
    labelling with a class of a single sample (its H is 0: no hit term) and an
    all-equal one (M = 0 everywhere: the scores are the pure hit part)."""
    rng = np.random.default_rng(seed)
    y = np.asarray(y)
    n = y.size
    enc = np.unique(y, return_inverse=True)[1].astype(np.int32).reshape(-1)
    rows = [enc] + [rng.permutation(enc) for _ in range(32)]
    three = rng.integers(0, 3, size=n).astype(np.int32)
    rows += [three, rng.permutation(three)]
    single = enc.copy()
    single[n // 2] = 7
    rows += [single, np.full(n, 5, dtype=np.int32)]
    lab = np.stack(rows).astype(np.int32)
    assert lab.shape == (37, n)
    return lab
