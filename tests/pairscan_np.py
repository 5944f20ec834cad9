"""What the pair screen (fs_pair_screen) must return, restated in numpy from the
definitions in fastselect_amd/csrc/fs_pairscan.h (helper, not collected), and
the planted data its tests share.

* ``expected`` takes a full symmetric matrix of joint relevance J and a
  relevance vector, forms the score by the written expression (``J`` for
  "joint", ``(J - rel[i]) - rel[j]`` for "gain", float64 in that order) and
  orders the pairs of ``np.triu_indices(p, 1)``, which is already the order of
  ``itertools.combinations(range(p), 2)``, by a stable argsort of the negated
  score: score descending, rank ascending, no closeness rule.
* ``pure`` plants a pair with no main effect: ``y = (x_a + x_b) mod states``
  (XOR for two states) on uniform columns, a fraction ``noise`` of the labels
  moved to the next class.
"""
import numpy as np


def scores(J, rel, score):
    """float64 [C(p,2)] in rank order, and the index arrays (i, j)."""
    J = np.asarray(J, dtype=np.float64)
    rel = np.asarray(rel, dtype=np.float64)
    i, j = np.triu_indices(J.shape[0], 1)
    s = J[i, j] if score == "joint" else (J[i, j] - rel[i]) - rel[j]
    return s, i, j


def expected(J, rel, score, n_top):
    """(top_score float64 [m], top_pairs int64 [m, 2], feature_best float64 [p]),
    m = min(n_top, C(p,2))."""
    s, i, j = scores(J, rel, score)
    order = np.argsort(-s, kind="stable")[:n_top]
    p = np.asarray(J).shape[0]
    best = np.full(p, -np.inf)
    np.maximum.at(best, i, s)
    np.maximum.at(best, j, s)
    return s[order], np.stack([i[order], j[order]], axis=1).astype(np.int64), best


def pure(n, p, seed, a, b, states, noise=0.1):
    """(X int64 [n, p], y int64 [n]) with the pair (a, b) planted."""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, states, (n, p))
    y = (X[:, a] + X[:, b]) % states
    flip = rng.random(n) < noise
    y = np.where(flip, (y + 1) % states, y)
    return X.astype(np.int64), y.astype(np.int64)


# (n, p, seed, a, b, states), the planted pair's J and the next pair's J in bits
# (measured with jmi_np), and whether JMI's first four picks miss a and b
PLANTED = [
    ((400, 40, 11, 7, 23, 2), 0.524, 0.028, True),
    ((300, 64, 12, 63, 0, 2), 0.511, 0.039, True),
    ((600, 30, 13, 5, 17, 3), 1.170, 0.051, False),
]


def tied():
    """(X uint8 [97, 8], y, S): columns 1 and 4 constant, columns 2, 5 and 6
    the same column, 3-state noise elsewhere and two classes of y.  A pair with
    a constant column has the J of its other column's own table up to rows of
    zeros, a pair of constants exactly 0.0, and the pairs (c, 2), (c, 5), (c, 6)
    share one table, so whole runs of scores are equal bit for bit."""
    rng = np.random.default_rng(401)
    X = rng.integers(0, 3, size=(97, 8)).astype(np.uint8)
    X[:, 1] = 2
    X[:, 4] = 0
    X[:, 5] = X[:, 2]
    X[:, 6] = X[:, 2]
    y = rng.integers(0, 2, size=97).astype(np.uint8)
    return X, y, 3


def all_constant():
    """Every column constant: every score is exactly 0.0."""
    X = np.tile(np.array([0, 2, 1, 1, 0, 2, 0], dtype=np.uint8), (64, 1))
    y = (np.arange(64) % 2).astype(np.uint8)
    return X, y, 3
