"""A plain numpy restatement of joint relevance and the JMI / CMIM greedy
loops (helper, not collected), written from the definitions in
fastselect_amd/csrc/fs_jmi.h, in float64 as stated there:

* for two columns lo < hi the table ``T[(a * S + b), c]`` counts the samples
  with ``x_lo = a``, ``x_hi = b``, ``y = c`` (S: any bound of the states; rows
  of states that never occur hold zeros and add exact zeros);
* ``J(lo, hi)`` is the mutual information of the table's rows and columns by
  the steps of ``mi_np.mi_of_tables``, here for a rectangular table:
  ``pxy = count / n``, ``p1`` summed over the classes and ``p2`` over the rows
  in index order from 0.0 (loops, not ``ndarray.sum``),
  ``mi += pxy * log(pxy / (p1 * p2 + 1e-12))`` over the cells with
  ``pxy > 1e-12``, row-major; divided by ``log(2.0)`` for bits;
* ``J(f, f) = 0``; the relevance of column f is ``mi_np``'s pair (f, y);
* the greedy loop: first the most relevant column, then the largest
  accumulator, JMI ``acc += J(., s)`` from 0.0, CMIM
  ``acc = min(acc, J(., s) - rel[s])`` from +inf; the lowest index among exact
  equals (``np.argmax``), no closeness rule.

As in mi_np, the package's one deviation is not copied: a table whose rows or
columns take a single value is exactly 0.0 there, about -k * 1e-12 here.
"""
import math

import numpy as np

import mi_np

EPS = 1e-12
METHODS = ("JMI", "CMIM")


def mi_of_tables(tabs, n, unit="bit"):
    """float64 MI of each table of ``tabs`` (int [..., R, C]): the rows against
    the columns."""
    tabs = np.asarray(tabs)
    R, C = tabs.shape[-2:]
    pxy = tabs.astype(np.float64) / float(n)
    p1 = np.zeros(tabs.shape[:-1])
    p2 = np.zeros(tabs.shape[:-2] + (C,))
    for c in range(C):
        p1 = p1 + pxy[..., :, c]
    for r in range(R):
        p2 = p2 + pxy[..., r, :]
    mi = np.zeros(tabs.shape[:-2])
    for r in range(R):
        for c in range(C):
            v = pxy[..., r, c]
            on = v > EPS
            with np.errstate(divide="ignore", invalid="ignore"):
                term = v * np.log(v / (p1[..., r] * p2[..., c] + EPS))
            mi = np.where(on, mi + term, mi)
    return mi / math.log(2.0) if unit == "bit" else mi


def three_way(X, y, anchor, S, C):
    """int64 [p, S * S, C]: for every column f the table of (lo, hi) =
    (min(f, anchor), max(f, anchor)) with y; row ``a * S + b`` is
    ``x_lo = a, x_hi = b``."""
    X = np.asarray(X, dtype=np.int64)
    y = np.asarray(y, dtype=np.int64)
    n, p = X.shape
    out = np.zeros((p, S * S * C), dtype=np.int64)
    xa = X[:, anchor]
    for f in range(p):
        lo, hi = (X[:, f], xa) if f < anchor else (xa, X[:, f])
        out[f] = np.bincount((lo * S + hi) * C + y, minlength=S * S * C)
    return out.reshape(p, S * S, C)


def row(X, y, anchor, S, C, unit="bit"):
    """float64 [p]: J(f, anchor), 0.0 at f == anchor."""
    r = mi_of_tables(three_way(X, y, anchor, S, C), np.asarray(X).shape[0], unit)
    r[anchor] = 0.0
    return r


def rows(X, y, anchors, S, C, unit="bit"):
    return np.stack([row(X, y, a, S, C, unit) for a in anchors])


def synthetic(X, anchor, K):
    """uint8 [n, p]: the joint column of every column with the anchor,
    ``x_lo * K + x_hi`` (the anchor's own column: itself)."""
    X = np.asarray(X, dtype=np.int64)
    Z = np.empty_like(X)
    for f in range(X.shape[1]):
        lo, hi = (f, anchor) if f < anchor else (anchor, f)
        Z[:, f] = X[:, lo] * K + X[:, hi] if f != anchor else X[:, f]
    assert Z.max() < 256
    return Z.astype(np.uint8)


def relevance(X, y, S, unit="bit"):
    """float64 [p]: I(X_f; y) by mi_np's steps."""
    _, cxy = mi_np.counts(X, y, S)
    return mi_np.mi_of_tables(cxy, np.asarray(X).shape[0], unit)


def greedy(rel, row_of, k, method):
    """The selection loop.  ``row_of(s)`` returns J(., s) over the p columns.
    Returns (selected int64 [k], margins): margins[i] is
    (best - runner-up) / |best| of step i's scores (inf with one candidate)."""
    rel = np.asarray(rel, dtype=np.float64)
    p = rel.shape[0]
    sel = np.zeros(k, dtype=np.int64)
    left = np.ones(p, dtype=bool)
    margins = []

    def margin(scores):
        if scores.size < 2:
            return np.inf
        top = np.sort(scores)[::-1]
        with np.errstate(divide="ignore", invalid="ignore"):   # all-zero scores: nan
            return (top[0] - top[1]) / abs(top[0])

    acc = np.zeros(p) if method == "JMI" else np.full(p, np.inf)
    for i in range(k):
        idx = np.where(left)[0]
        scores = rel[idx] if i == 0 else acc[idx]
        margins.append(margin(scores))
        best = idx[np.argmax(scores)]   # the first of exact equals
        sel[i] = best
        left[best] = False
        if i + 1 < k:
            r = np.asarray(row_of(int(best)), dtype=np.float64)
            acc = acc + r if method == "JMI" else np.minimum(acc, r - rel[best])
    return sel, np.array(margins)


def planted_pair(n, p, seed, a, b, states=2, classes=None):
    """A planted interaction.  Columns uniform over 0..states-1 from
    ``default_rng(seed).integers``; with ``g(u, v) = (u + v) mod states`` (XOR
    for two states) y is ``x_a`` on a random 25% of the samples and
    ``g(x_a, x_b)`` on the rest, reduced to ``classes`` classes by
    ``mod classes`` when given, and 5% of the labels are replaced by the next
    class.  Column a is relevant on its own; column b only together with a."""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, states, size=(n, p))
    own = rng.random(n) < 0.25
    y = np.where(own, X[:, a], (X[:, a] + X[:, b]) % states)
    C = classes or states
    y = y % C
    flip = rng.random(n) < 0.05
    y = np.where(flip, (y + 1) % C, y)
    return X.astype(np.int64), y.astype(np.int64)


# (n, p, seed, a, b, states, classes): two binary cases (in the first, b ranks
# 17th of 40 by its own relevance and mRMR's second pick is noise column 34; in
# the second 40th of 64 and column 49), one 3-state and one 5-state case (the
# latter with two classes of y, so that it runs on the GPU backend too)
PLANTED = [
    (400, 40, 2, 7, 23, 2, None),
    (300, 64, 4, 63, 0, 2, None),
    (400, 30, 3, 5, 17, 3, None),
    (600, 24, 5, 20, 2, 5, 2),
]


def tie_inputs(p, seed):
    """(rel, joint) with values on a coarse dyadic grid, so that sums and
    differences are exact and exact ties occur at many steps, for both methods;
    the CMIM minimum is attained by different selected features for different
    candidates."""
    rng = np.random.default_rng(seed)
    rel = rng.integers(1, 4, size=p) / 8.0
    j = rng.integers(4, 9, size=(p, p)) / 8.0
    j = np.triu(j, 1)
    j = j + j.T
    return rel, j


TIE_CASES = [(40, 40, 1), (257, 30, 2), (513, 30, 3)]


def exact_tie_steps(rel, joint, k, method):
    """Steps of the greedy loop at which the best score is shared by at least
    two candidates and the winner is therefore decided by the index."""
    p = rel.shape[0]
    left = np.ones(p, dtype=bool)
    acc = np.zeros(p) if method == "JMI" else np.full(p, np.inf)
    ties = 0
    for i in range(k):
        idx = np.where(left)[0]
        scores = rel[idx] if i == 0 else acc[idx]
        ties += int((scores == scores.max()).sum() > 1)
        best = idx[np.argmax(scores)]
        left[best] = False
        acc = acc + joint[best] if method == "JMI" else np.minimum(acc, joint[best] - rel[best])
    return ties


def cmim_argmin_spread(rel, joint, sel):
    """The number of distinct selected features that attain the CMIM minimum
    for some candidate, after ``sel`` was selected."""
    d = joint[sel] - rel[sel][:, None]
    return np.unique(np.argmin(d, axis=0)).size
