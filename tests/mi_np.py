"""A plain numpy restatement of discrete mutual information and the mRMR
greedy loop (helper, not collected).

Every mutual-information test compares against this file because the
reference itself cannot produce fixtures: its kernels need numba, which the
test machines do not have.  It is written from the description of the
method, in float64 as stated there:

* a pair's table counts the samples per (state of the first column, state of
  the second); ``pxy = count / n``;
* ``p1[a]`` sums ``pxy[a][b]`` over b and ``p2[b]`` over a, each in index
  order from 0.0 (a loop, not ``ndarray.sum``, whose pairwise order differs);
* ``mi += pxy * log(pxy / (p1[a] * p2[b] + 1e-12))`` over the cells with
  ``pxy > 1e-12``, row-major; divided by ``log(2.0)`` for bits;
* a pair is computed once for i < j with the rows taken from column i and
  mirrored; the diagonal is 0; the relevance of column f is the pair (f, y);
* the greedy loop: first the most relevant column; then the best MID / MIQ
  score, candidates within ``np.isclose(scores, max, atol=1e-12)`` (default
  rtol) resolved by the lowest mean redundancy.

The package deviates in one place, which this file does not copy: a pair with
a single-valued column is exactly 0.0 there, about -k * 1e-12 here (inside the
tests' 1e-10).

The loops run over the table's cells with all pairs side by side, so the
order of every float64 operation is the stated one.
"""
import math

import numpy as np

EPS = 1e-12


def counts(X, y, n_states):
    """(cxx int64 [p, p, S, S], cxy int64 [p, S, S]): the table of every
    ordered pair of columns, and of every column with y."""
    X = np.asarray(X, dtype=np.int64)
    y = np.asarray(y, dtype=np.int64)
    n, p = X.shape
    S = int(n_states)
    onehot = (X[:, :, None] == np.arange(S)).astype(np.int64).reshape(n, p * S)
    yhot = (y[:, None] == np.arange(S)).astype(np.int64)
    cxx = (onehot.T @ onehot).reshape(p, S, p, S).transpose(0, 2, 1, 3)
    cxy = (onehot.T @ yhot).reshape(p, S, S)
    return np.ascontiguousarray(cxx), cxy


def mi_of_tables(tabs, n, unit="bit"):
    """float64 MI of each table of ``tabs`` (int [..., S, S])."""
    tabs = np.asarray(tabs)
    S = tabs.shape[-1]
    pxy = tabs.astype(np.float64) / float(n)
    p1 = np.zeros(tabs.shape[:-1])
    p2 = np.zeros(tabs.shape[:-2] + (S,))
    for b in range(S):
        p1 = p1 + pxy[..., :, b]
    for a in range(S):
        p2 = p2 + pxy[..., a, :]
    mi = np.zeros(tabs.shape[:-2])
    for a in range(S):
        for b in range(S):
            c = pxy[..., a, b]
            on = c > EPS
            with np.errstate(divide="ignore", invalid="ignore"):
                term = c * np.log(c / (p1[..., a] * p2[..., b] + EPS))
            mi = np.where(on, mi + term, mi)
    return mi / math.log(2.0) if unit == "bit" else mi


def matrices(X, y, n_states, unit="bit"):
    """(relevance [p], redundancy [p, p], counts int32 [p, p, S, S]): counts
    holds the table of i < j (row = state of column i), zeros elsewhere."""
    p = np.asarray(X).shape[1]
    n = np.asarray(X).shape[0]
    cxx, cxy = counts(X, y, n_states)
    upper = np.triu(np.ones((p, p), dtype=bool), 1)
    cxx = np.where(upper[:, :, None, None], cxx, 0)
    rel = mi_of_tables(cxy, n, unit)
    m = np.where(upper, mi_of_tables(cxx, n, unit), 0.0)
    return rel, m + m.T, cxx.astype(np.int32)


def greedy(rel, red, k, method):
    """The selection loop.  Returns (selected int32 [k], margins): margins[s]
    is (best - runner-up) / |best| of step s's scores (inf with one
    candidate)."""
    p = rel.shape[0]
    sel = np.zeros(k, dtype=np.int32)
    left = np.ones(p, dtype=bool)
    margins = []

    def margin(scores):
        if scores.size < 2:
            return np.inf
        top = np.sort(scores)[::-1]
        return (top[0] - top[1]) / abs(top[0])

    first = int(np.argmax(rel))
    margins.append(margin(rel))
    sel[0] = first
    left[first] = False
    rsum = red[:, first].copy()
    for i in range(1, k):
        idx = np.where(left)[0]
        if method == "MID":
            scores = rel[idx] - (rsum[idx] / i)
        else:
            scores = rel[idx] / ((rsum[idx] / i) + 1e-9)
        margins.append(margin(scores))
        top = idx[np.isclose(scores, np.max(scores), atol=1e-12)]
        best = top[np.argmin(rsum[top] / i)] if top.size > 1 else top[0]
        sel[i] = best
        left[best] = False
        rsum = rsum + red[:, best]
    return sel, np.array(margins)


def uniform(n, p, states, seed, y_states=None):
    """default_rng(seed) noise: X in 0..states-1, y in 0..y_states-1."""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, states, size=(n, p)).astype(np.uint8)
    y = rng.integers(0, y_states or states, size=n).astype(np.uint8)
    return X, y


PLANT_NOISE = (0.05, 0.12, 0.20, 0.28, 0.35)


def planted(n, p, states, seed):
    """y uniform in {0, 1, 2}; columns 1, p//2, p-1, p//3, 2p//3 are copies of
    y with a fraction PLANT_NOISE of their entries replaced by uniform noise;
    every other column is uniform noise over 0..states-1 (the replaced
    entries: over y's range too when states < 3).  Far from a greedy tie."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 3, size=n)
    X = rng.integers(0, states, size=(n, p))
    for col, frac in zip((1, p // 2, p - 1, p // 3, 2 * p // 3), PLANT_NOISE):
        noisy = rng.random(n) < frac
        X[:, col] = np.where(noisy, rng.integers(0, max(states, 3), size=n), y)
    return X.astype(np.int64), y.astype(np.int64)


# (n, p, states, seed) of the planted estimator cases and the margin every
# greedy step must keep on this file's own scores
PLANTED = [(203, 37, 3, 1), (65, 130, 5, 2), (257, 20, 32, 3), (64, 17, 2, 4)]
PLANT_MARGIN = 7e-3

_CASES = {}


def case(key, make):
    """(X, y, S, rel, red, counts) of one parity case, computed once per
    session and shared read-only.  ``make`` returns (X, y, S)."""
    if key not in _CASES:
        X, y, S = make()
        rel, red, cnt = matrices(X, y, S)
        for a in (X, y, rel, red, cnt):
            a.setflags(write=False)
        _CASES[key] = (X, y, S, rel, red, cnt)
    return _CASES[key]


def mixed_columns(n=130, seed=9):
    """One matrix with a constant column, a column using only codes {0, 4}, a
    2-state column beside a 32-state column, and noise."""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 6, size=(n, 9)).astype(np.uint8)
    X[:, 0] = 0
    X[:, 2] = 4 * rng.integers(0, 2, size=n)
    X[:, 3] = rng.integers(0, 2, size=n)
    X[:, 4] = rng.integers(0, 32, size=n)
    X[0, 4] = 31
    X[:, 7] = 3
    y = rng.integers(0, 4, size=n).astype(np.uint8)
    return X, y, 32


def mixed_bound(n, S, seed):
    """mixed_columns with the state bound at S: a constant column, a column
    using only codes {0, S - 1}, a 2-state column beside one over 0..S-1 (its
    first entry S - 1), another constant column, and 6-state noise."""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 6, size=(n, 9)).astype(np.uint8)
    X[:, 0] = 0
    X[:, 2] = (S - 1) * rng.integers(0, 2, size=n)
    X[:, 3] = rng.integers(0, 2, size=n)
    X[:, 4] = rng.integers(0, S, size=n)
    X[0, 4] = S - 1
    X[:, 7] = 3
    y = rng.integers(0, 4, size=n).astype(np.uint8)
    return X, y, S


# name -> () -> (X, y, n_states): the shapes both backends are checked on
def _u(n, p, states, seed, y_states=None):
    return lambda: uniform(n, p, states, seed, y_states) + (max(states, y_states or 0),)


SHAPES = {
    "n33": _u(33, 5, 3, 11),
    "n64": _u(64, 5, 3, 12),
    "n203": _u(203, 5, 3, 13),
    "p17_tile16": _u(65, 17, 3, 14),
    "p34_tile16": _u(65, 34, 3, 15),
    "p9_tile8": _u(65, 9, 5, 16),
    "p18_tile8": _u(65, 18, 5, 17),
    "p130": _u(65, 130, 3, 18),
    "states2": _u(97, 7, 2, 19),
    "states5": _u(97, 7, 5, 20),
    "states10": _u(150, 11, 10, 21),
    "states32": _u(257, 20, 32, 22),
    "mixed": mixed_columns,
    "y4": _u(120, 6, 3, 23, 4),
    "restage": _u(2049, 12, 3, 24),
}


# ---- every lane geometry of the pair-table kernels ---------------------------
# k_mi_scan, k_mi_row, k_cfs_row, k_jmi_rel, k_jmi_row and k_mi_pack take their
# thread layout from NB = ceil(states / 4): a pair gets NB^2 lanes, a tile of
# the scan is T = 16 / NB columns wide and a workgroup of the row kernels holds
# CPW = 256 / NB^2 columns (250, 252 and 245 of its 256 lanes at NB = 5, 6, 7).
def nb(states):
    return (states + 3) // 4


def tile(states):
    return 16 // nb(states)


def cpw(states):
    return 256 // nb(states) ** 2


# both ends of every NB in 1..7, the low end of NB = 8, and every count with no
# padding plane (a multiple of 4)
GEOMETRY_STATES = (4, 8, 12, 13, 16, 17, 20, 21, 24, 25, 28, 29)
GEOMETRY_N = (97, 257)


def geometry_dims():
    """(n, p, states): per state count p = CPW - 1 (y, one more column, is the
    last used lane of the only workgroup), CPW (y alone in a second one),
    CPW + 1, and 2T + 1 (with y a whole third tile of the scan beside two
    diagonal and one off-diagonal; the others end in a ragged tile)."""
    out = []
    for s in GEOMETRY_STATES:
        for p in sorted({cpw(s) - 1, cpw(s), cpw(s) + 1, 2 * tile(s) + 1}):
            out.extend((n, p, s) for n in GEOMETRY_N)
    return out


def geometry_name(n, p, states, classes=None):
    c = "" if classes is None else "_c%d" % classes
    return "geo_s%02d%s_p%d_n%d" % (states, c, p, n)


def geometry_case(n, p, states, classes=4):
    """Uniform codes over 0..states-1 and y over 0..classes-1.  With 13 to 29
    states and 97 or 257 samples many cells and some states stay empty."""
    return _u(n, p, states, 1000 * states + 10 * p + n % 10 + classes, classes)


GEOMETRY = {geometry_name(*d): geometry_case(*d) for d in geometry_dims()}
GEOMETRY["geo_mixed_s21"] = lambda: mixed_bound(97, 21, 121)
GEOMETRY["geo_mixed_s25"] = lambda: mixed_bound(257, 25, 125)

# ---- long sample axes --------------------------------------------------------
# The row kernels stage 64 words (2048 samples) per chunk: one whole chunk, two
# whole chunks, two chunks and one sample (two restages).
LONG = {"n%d" % n: _u(n, 5, 3, 30 + n % 7) for n in (2048, 4096, 4097)}

# SHAPES and the two tables above: what both backends are held to
ALL_SHAPES = {**SHAPES, **GEOMETRY, **LONG}


def two_slabs():
    """(X, y, fold): n = 65535 * 32 + 33, so that word 65536 is the first of a
    second pack slab (grid.y holds 65535) and the last word is ragged.  Three
    3-state columns, y the parity of columns 0 and 2 with 20 % flipped, fold
    ids i % 3."""
    n = 65535 * 32 + 33
    rng = np.random.default_rng(77)
    X = rng.integers(0, 3, size=(n, 3)).astype(np.uint8)
    y = ((X[:, 0] + X[:, 2]) & 1).astype(np.uint8)
    y ^= (rng.random(n) < 0.20).astype(np.uint8)
    fold = (np.arange(n) % 3).astype(np.int32)
    return X, y, fold


_SLABS = []


def two_slabs_case():
    """two_slabs(), built once per session and shared read-only."""
    if not _SLABS:
        _SLABS.extend(two_slabs())
        for a in _SLABS:
            a.setflags(write=False)
    return tuple(_SLABS)
