"""A plain numpy restatement of CFS (helper, not collected): symmetrical
uncertainty, the merit, the best-first search and the prune.

Every CFS test compares against this file because the reference itself cannot
produce fixtures: its kernels need numba, which the test machines do not
have.  It is written from the description of the method, with compiled
numba's typing (float32 counts / int64 n is float64, and so is everything
after, until the float32 store):

* a pair's table counts the samples per (state of the first column, state of
  the second); the column with the lower index is the first, the target counts
  as column p; ``pxy = count / n``;
* ``px[a]`` sums ``pxy[a][b]`` over b and ``py[b]`` over a, each in index
  order from 0.0 (a loop, not ``ndarray.sum``);
* a column's entropy is ``h -= prob * log2(prob)`` over its states in index
  order with ``prob = (state count) / n > 1e-12``;
* ``hx + hy < 1e-12`` gives 0.0; else ``mi += pxy * log2(pxy / (px * py))``
  row-major over the cells where all three exceed 1e-12, and
  ``SU = 2 * mi / (hx + hy)`` stored as float32;
* ``merit(sum_r_cf, k, sum_r_ff)``: ``r_cf_avg = sum_r_cf / k``, ``r_ff_avg =
  (2 * sum_r_ff) / (k * (k - 1))`` (0.0 for k = 1), ``denom = sqrt(k + k *
  (k - 1) * r_ff_avg)``, ``k * r_cf_avg / denom`` (0.0 when denom <= 1e-12);
* the search starts at ``argmax(r_cf)`` (nothing when that is < 0.1); a step
  scans the unselected i with ``r_cf[i] >= 0.1``; ``sum_r_cf`` adds the
  selected features in selection order, then i; ``sum_r_ff`` adds
  ``r_ff[a, b]`` over ``for a in selected: for b in selected: if a < b``, then
  ``r_ff[i, s]`` for s in selection order; float64 sums over the float32
  values; the lowest-index candidate with ``merit > best`` wins; the search
  stops when no candidate improves the merit;
* the prune keeps, in descending ``r_cf`` order (stable over ascending
  indices), each feature with no ``r_ff[idx, j] >= r_cf[idx]`` for a kept j;
  the final merit takes ``np.sum`` of the float32 ``r_cf`` entries and of the
  upper triangle of the float32 submatrix, converts both to Python floats and
  applies ``merit``.
"""
import math

import numpy as np

import mi_np

EPS = 1e-12
MIN_R_CF = 0.1


def su_of_tables(tabs, n):
    """float32 SU of each table of ``tabs`` (int [..., S, S]; rows = states of
    the pair's first column)."""
    tabs = np.asarray(tabs)
    S = tabs.shape[-1]
    fn = float(n)
    pxy = tabs.astype(np.float64) / fn
    px = np.zeros(tabs.shape[:-1])
    py = np.zeros(tabs.shape[:-2] + (S,))
    for b in range(S):
        px = px + pxy[..., :, b]
    for a in range(S):
        py = py + pxy[..., a, :]

    def entropy(cnt):
        prob = cnt.astype(np.float64) / fn
        h = np.zeros(cnt.shape[:-1])
        for s in range(S):
            q = prob[..., s]
            with np.errstate(divide="ignore", invalid="ignore"):
                h = np.where(q > EPS, h - q * np.log2(q), h)
        return h

    hx = entropy(tabs.sum(axis=-1))
    hy = entropy(tabs.sum(axis=-2))
    mi = np.zeros(tabs.shape[:-2])
    for a in range(S):
        for b in range(S):
            c = pxy[..., a, b]
            on = (c > EPS) & (px[..., a] > EPS) & (py[..., b] > EPS)
            with np.errstate(divide="ignore", invalid="ignore"):
                term = c * np.log2(c / (px[..., a] * py[..., b]))
            mi = np.where(on, mi + term, mi)
    hs = hx + hy
    with np.errstate(divide="ignore", invalid="ignore"):
        su = np.where(hs < EPS, 0.0, 2.0 * mi / hs)
    return su.astype(np.float32)


def matrices(X, y, n_states):
    """(r_cf float32 [p], r_ff float32 [p, p] symmetric, zero diagonal)."""
    n, p = np.asarray(X).shape
    cxx, cxy = mi_np.counts(X, y, n_states)
    upper = np.triu(np.ones((p, p), dtype=bool), 1)
    r_cf = su_of_tables(cxy, n)
    m = np.where(upper, su_of_tables(cxx, n), np.float32(0.0)).astype(np.float32)
    return r_cf, m + m.T


def merit(sum_r_cf, k, sum_r_ff):
    if k == 0:
        return 0.0
    r_cf_avg = sum_r_cf / k
    r_ff_avg = (2.0 * sum_r_ff) / (k * (k - 1)) if k > 1 else 0.0
    denom = math.sqrt(k + k * (k - 1) * r_ff_avg)
    return (k * r_cf_avg / denom) if denom > 1e-12 else 0.0


def best_first(r_cf, r_ff, min_r_cf=MIN_R_CF):
    """(selected list in selection order, merits list, margins list).
    margins: per accepting step (best - max(runner-up, current)) / best, and
    for the stopping step (current - best) / current (inf without a
    candidate)."""
    p = r_cf.shape[0]
    first = int(np.argmax(r_cf))
    if float(r_cf[first]) < min_r_cf:
        return [], [], []
    selected = [first]
    current = float(r_cf[first])
    merits = [current]
    margins = []
    while True:
        k = len(selected) + 1
        base_cf = 0.0
        for idx in selected:
            base_cf += float(r_cf[idx])
        base_ff = 0.0
        for a in selected:
            for b in selected:
                if a < b:
                    base_ff += float(r_ff[a, b])
        best_i, best = -1, current
        cand = []
        for i in range(p):
            if i in selected or float(r_cf[i]) < min_r_cf:
                continue
            sum_r_cf = base_cf + float(r_cf[i])
            sum_r_ff = base_ff
            for s in selected:
                sum_r_ff += float(r_ff[i, s])
            m = merit(sum_r_cf, k, sum_r_ff)
            cand.append(m)
            if m > best:
                best, best_i = m, i
        top = sorted(cand, reverse=True)
        if best_i != -1:
            other = max(top[1], current) if len(top) > 1 else current
            margins.append((best - other) / best)
            selected.append(best_i)
            merits.append(best)
            current = best
        else:
            margins.append((current - top[0]) / current if top else np.inf)
            break
    return selected, merits, margins


def prune(selected, r_cf, r_ff):
    """(kept list, the smallest |r_ff - r_cf| gap of the comparisons made)."""
    kept, gap = [], np.inf
    for idx in sorted(sorted(selected), key=lambda i: -r_cf[i]):
        drop = False
        for j in kept:
            gap = min(gap, abs(float(r_ff[idx, j]) - float(r_cf[idx])))
            drop = drop or bool(r_ff[idx, j] >= r_cf[idx])
        if not drop:
            kept.append(idx)
    return kept, gap


def final_merit(kept, r_cf, r_ff):
    idx = np.sort(np.array(kept, dtype=int))
    if idx.size == 0:
        return 0.0
    sum_r_cf = np.sum(r_cf[idx])
    sum_r_ff = np.sum(np.triu(r_ff[np.ix_(idx, idx)], k=1))
    return merit(float(sum_r_cf), int(idx.size), float(sum_r_ff))


# ---- data families -----------------------------------------------------------
PLANT_NOISE = (0.20, 0.26, 0.32, 0.38, 0.44, 0.50)


def planted_columns(p):
    return (1, p // 2, p - 1, p // 3, 2 * p // 3, p // 5)


def planted(n, p, states, seed):
    """y uniform over min(states, 3) classes; the columns planted_columns(p)
    are copies of y with a fraction PLANT_NOISE of their entries replaced by
    uniform noise; column 3 is a copy of column 1 with 5 % replaced; every
    other column is uniform noise over 0..states-1.  Keep p >= 10."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, min(states, 3), size=n)
    X = rng.integers(0, states, size=(n, p))
    for col, frac in zip(planted_columns(p), PLANT_NOISE):
        noisy = rng.random(n) < frac
        X[:, col] = np.where(noisy, rng.integers(0, states, size=n), y)
    noisy = rng.random(n) < 0.05
    X[:, 3] = np.where(noisy, rng.integers(0, states, size=n), X[:, 1])
    return X.astype(np.int64), y.astype(np.int64)


# (n, p, states, seed) of the planted selection cases
PLANTED = [(203, 37, 3, 1), (257, 20, 32, 3), (65, 130, 5, 2), (97, 17, 2, 4), (2049, 12, 3, 5),
           (513, 40, 10, 6)]
MARGIN = 1e-4

_PLANTED = {}


def planted_case(key):
    """(X, y, S, r_cf, r_ff, selected, merits, kept, merit) of one planted
    case, computed once per session and shared read-only, after asserting on
    the restatement itself that the case decides nothing narrowly."""
    if key not in _PLANTED:
        n, p, states, seed = key
        X, y = planted(n, p, states, seed)
        r_cf, r_ff = matrices(X, y, states)
        sel, mer, margins = best_first(r_cf, r_ff)
        kept, gap = prune(sel, r_cf, r_ff)
        assert min(margins) >= MARGIN, (key, margins)
        assert gap >= MARGIN, (key, gap)
        # "the selection" is the one the estimator reports, after the prune:
        # at (2049, 12, 3, 5) the search takes all 7 candidates and the prune
        # drops the duplicate, so only this reading holds on every case
        assert len(kept) >= 3, (key, kept)
        assert int(np.sum(r_cf.astype(np.float64) >= MIN_R_CF)) > len(kept), key
        for a in (X, y, r_cf, r_ff):
            a.setflags(write=False)
        _PLANTED[key] = (X, y, states, r_cf, r_ff, sel, mer, kept, final_merit(kept, r_cf, r_ff))
    return _PLANTED[key]


def random_matrix(p, seed, eighths=False):
    """(r_cf float32 [p], r_ff float32 [p, p] symmetric, zero diagonal): class
    correlations in [0, 1), pairwise ones in [0, 0.5); with ``eighths`` both
    are multiples of 1/8, so that equal merits occur and the lowest-index rule
    decides."""
    rng = np.random.default_rng(seed)
    if eighths:
        r_cf = (rng.integers(0, 8, size=p) / 8.0).astype(np.float32)
        m = (rng.integers(0, 4, size=(p, p)) / 8.0).astype(np.float32)
    else:
        r_cf = rng.random(p).astype(np.float32)
        m = (0.5 * rng.random((p, p))).astype(np.float32)
    m = np.triu(m, 1)
    return r_cf, m + m.T


_SU = {}


def su_case(key, make):
    """(X, y, S, r_cf, r_ff) of one SU parity case, shared read-only."""
    if key not in _SU:
        X, y, S = make()
        r_cf, r_ff = matrices(X, y, S)
        for a in (X, y, r_cf, r_ff):
            a.setflags(write=False)
        _SU[key] = (X, y, S, r_cf, r_ff)
    return _SU[key]


def f32_steps(a, b):
    """Per entry, how many float32 values apart a and b are (0: equal bits up
    to the sign of zero)."""
    ia = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)
