"""Float64 numpy model of ReliefF scores under many labellings -- TEST
INFRASTRUCTURE ONLY.

The ``relieff`` loop of ``oracle/relief_np.py`` (the same per-feature diffs,
``_diff_rows``: the reference's float32 diffs widened to float64; the same
float32 keys with the focal key at inf; one argsort of the key row per focal
sample, ``oracle.numba_argsort`` where the caller passes it) with the two sums
a score is made of kept apart, per labelling:

    Hit_f  = sum_i (1 / h_i) sum over the k nearest hits of i of d_f
    Miss_f = sum_i sum_{c != y_i} (P_c / (1 - P_{y_i})) / k
                   * sum over the k nearest members of class c of d_f
    score_f = Miss_f - Hit_f        (a sum over the samples: not divided by n)

The argsort does not read the labels: for any labelling the neighbours of a
class are the first k of that class met on the walk of the one order.  The
focal sample sits last on it (key inf) and is met as a hit when its class has
fewer than k other members: it adds a zero diff and counts in h_i
(ReliefF.py:144-168).  The priors of a labelling are its class shares rounded
to float32, as ``ReliefF.fit`` forms them; a code without a member takes no
part.  Nothing here calls the library.
"""
from __future__ import annotations

import numpy as np

from oracle import relief_np
from stir_np import mixed_case  # noqa: F401  (the cases the tests use)
from stir_relieff_np import preprocess, three_class_case  # noqa: F401


def score_parts(x32, labels, recip, is_disc, k, argsort=None, neighbours=False):
    """(miss[B, p], hit[B, p], score[B, p], sets) of the labellings ``labels``
    ((n,) for one labelling or (B, n)), float64.  sets[b][i] = {class: [the
    chosen samples in walk order]} with ``neighbours``, else None."""
    n, p = x32.shape
    lab = np.atleast_2d(np.asarray(labels))
    B = lab.shape[0]
    miss = np.zeros((B, p), dtype=np.float64)
    hit = np.zeros((B, p), dtype=np.float64)
    sets = [[None] * n for _ in range(B)] if neighbours else None
    priors = []
    for b in range(B):
        cnt = np.bincount(lab[b])
        priors.append((cnt / n).astype(np.float32).astype(np.float64))
    for i in range(n):
        d = relief_np._diff_rows(x32, i, recip, is_disc)     # (n, p) float64
        keys = d.sum(axis=1).astype(np.float32)
        keys[i] = np.inf
        order = np.argsort(keys, kind="stable") if argsort is None else argsort(keys)
        order = np.asarray(order, dtype=np.int64)
        dord = d[order]                                       # rows in walk order
        for b in range(B):
            lo = lab[b][order]
            li = lab[b, i]
            pr = priors[b]
            denom = 1.0 - pr[li]
            if denom == 0:
                denom = 1.0
            chosen = {}
            for c in np.flatnonzero(pr > 0):
                pos = np.flatnonzero(lo == c)[:k]
                if pos.size == 0:
                    continue
                s = dord[pos].sum(axis=0)
                if c == li:
                    hit[b] += s / pos.size
                else:
                    miss[b] += (pr[c] / denom) * s / k
                if neighbours:
                    chosen[int(c)] = [int(j) for j in order[pos] if j != i]
            if neighbours:
                sets[b][i] = chosen
    return miss, hit, miss - hit, sets


def labellings(y, n_perm=34, small=4, seed=1):
    """The labellings of the GPU tests: y, ``n_perm`` permutations of it and
    one labelling with a class of ``small`` members (code 5: the codes in
    between have no member)."""
    rng = np.random.default_rng(seed)
    enc = np.unique(np.asarray(y), return_inverse=True)[1].astype(np.int32).reshape(-1)
    rows = [enc] + [rng.permutation(enc) for _ in range(n_perm)]
    last = enc.copy()
    last[rng.choice(enc.size, size=small, replace=False)] = 5
    rows.append(last)
    return np.stack(rows).astype(np.int32)


def duplicates_case(n=130, p=64, dup=10, seed=2):
    """n x p continuous columns in which rows n - dup .. n - 1 repeat rows
    0 .. dup - 1: every row's keys to such a pair tie exactly."""
    rng = np.random.default_rng(seed)
    x = rng.random((n, p)).astype(np.float32)
    x[n - dup:] = x[:dup]
    y = (x[:, 3] + 0.3 * rng.standard_normal(n) > 0.5).astype(np.float64)
    return x, y
