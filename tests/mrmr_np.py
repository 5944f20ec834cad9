"""Inputs and numpy checks shared by the selection-only mRMR tests (helper,
not collected).  The greedy loop itself is ``mi_np.greedy``."""
import numpy as np

import mi_np

METHODS = ("MID", "MIQ")

# (p, k, seed) of the crafted tie inputs; 257 and 513 cross the step kernels'
# 256-lane workgroup boundary
TIE_CASES = [(40, 40, 1), (257, 60, 2), (513, 30, 3)]
# steps with more than one top candidate whose winner is neither the
# lowest-index candidate nor the arg-max score, computed with numpy when the
# cases were chosen: (MID, MIQ) per case, and the columns tied for the first
# arg-max (without the lowest-index clause the counts are 9, 14; 23, 36; 11, 22)
TIE_STEPS = {(40, 40, 1): (7, 11), (257, 60, 2): (22, 36), (513, 30, 3): (11, 22)}
TIE_FIRST = {(40, 40, 1): 13, (257, 60, 2): 64, (513, 30, 3): 132}


def tie_inputs(p, seed):
    """Relevances of four levels, three of them within isclose's rtol of each
    other, over redundancies that differ by up to 1e-6: many steps have several
    top candidates and the mean redundancy decides."""
    rng = np.random.default_rng(seed)
    rel = rng.choice([0.5, 0.5 * (1 + 3e-6), 0.5 * (1 - 4e-6), 0.3], p)
    up = np.triu(0.2 + 1e-6 * rng.random((p, p)), 1)
    red = up + up.T
    return rel, red


def meaningful_tie_steps(rel, red, k, method):
    """The number of steps i >= 1 of the greedy loop with more than one top
    candidate and a winner that is neither the lowest-index top candidate nor
    the arg-max of the scores (a plain numpy loop of its own)."""
    p = rel.shape[0]
    left = np.ones(p, dtype=bool)
    first = int(np.argmax(rel))
    left[first] = False
    rsum = red[:, first].copy()
    count = 0
    for i in range(1, k):
        idx = np.where(left)[0]
        avg = rsum[idx] / i
        scores = rel[idx] - avg if method == "MID" else rel[idx] / (avg + 1e-9)
        mx = np.max(scores)
        top = np.abs(scores - mx) <= 1e-12 + 1e-5 * abs(mx)
        cand = idx[top]
        best = cand[np.argmin(avg[top])]
        if cand.size > 1 and best != cand[0] and best != idx[np.argmax(scores)]:
            count += 1
        left[best] = False
        rsum = rsum + red[:, best]
    return count


def exact_tie_steps(rel, red, k, method):
    """Steps i >= 1 at which two candidates share the maximum score exactly."""
    p = rel.shape[0]
    left = np.ones(p, dtype=bool)
    sel, _ = mi_np.greedy(rel, red, k, method)
    left[sel[0]] = False
    rsum = red[:, sel[0]].copy()
    count = 0
    for i in range(1, k):
        idx = np.where(left)[0]
        avg = rsum[idx] / i
        scores = rel[idx] - avg if method == "MID" else rel[idx] / (avg + 1e-9)
        count += int((scores == np.max(scores)).sum() > 1)
        left[sel[i]] = False
        rsum = rsum + red[:, sel[i]]
    return count


def duplicated():
    """(X, y, S): noise with columns p - 1 and p // 2 equal to column 2 and
    column 5 equal to column p - 2, so that candidates tie exactly."""
    X, y = mi_np.uniform(65, 40, 3, 51)
    X = X.copy()
    p = X.shape[1]
    X[:, p - 1] = X[:, 2]
    X[:, p // 2] = X[:, 2]
    X[:, 5] = X[:, p - 2]
    return X, y, 3


def ks(p):
    """k = 1, a middle value, p."""
    return sorted({1, max(1, p // 2), p})
