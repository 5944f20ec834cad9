"""A plain numpy restatement of the MDR contract (helper, not collected).

Written from the description of the method, in float64 as stated there:

* a sample is a case iff its label is 1, every other label is a control;
* a combination's 3^k table counts cases and controls of the training rows
  per cell, ``cell = cell * 3 + genotype`` with the first column most
  significant;
* scan rule: a cell is high risk iff it has no controls or
  ``case / control > total_case / total_control``; ``tp`` sums the cases of
  high-risk cells, ``tn`` the controls of the others; ``BA = (tp / total_case
  + tn / total_control) / 2.0`` rounded to float32, or 0 without training
  cases or controls;
* a fold's model is the first combination with the largest float32 BA;
* lookup-table rule (different): ``case / (control + 1e-9) > threshold``,
  ``threshold = total_case / total_control`` (inf without controls);
* the fitted model has the highest cross-validation consistency, then the
  highest mean test BA.
"""
from collections import Counter
from itertools import combinations

import numpy as np
from sklearn.model_selection import StratifiedKFold


def planted(n, p, seed=7, pair=None):
    """default_rng(seed) genotypes with one planted pair: P(case | g_a, g_b)
    from a 3 x 3 penetrance table.  Returns (X uint8, y uint8)."""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 3, size=(n, p)).astype(np.uint8)
    if pair is None:
        pair = (1, p - 2) if p >= 4 else (0, p - 1)
    pen = np.array([[0.08, 0.12, 0.88], [0.12, 0.90, 0.10], [0.90, 0.10, 0.15]])
    a, b = pair
    prob = pen[X[:, a], X[:, b]] if a != b else pen[X[:, a], X[:, a]]
    y = (rng.random(n) < prob).astype(np.uint8)
    return X, y


def fold_ids(X, y, cv):
    """fold[i] = the fold whose test set holds sample i, and the splits."""
    splits = list(StratifiedKFold(n_splits=cv, shuffle=True, random_state=42).split(X, y))
    fold = np.empty(X.shape[0], dtype=np.int32)
    for i, (_, te) in enumerate(splits):
        fold[te] = i
    return fold, splits


def cells(X, combo):
    c = np.zeros(X.shape[0], dtype=np.int64)
    for j in combo:
        c = c * 3 + X[:, j].astype(np.int64)
    return c


def table(X, is_case, combo):
    nc = 3 ** len(combo)
    c = cells(X, combo)
    return (np.bincount(c[is_case], minlength=nc).astype(np.float64),
            np.bincount(c[~is_case], minlength=nc).astype(np.float64))


def all_bas(X, is_case, k):
    """float32 BA of every k-combination, itertools.combinations order."""
    is_case = np.asarray(is_case, dtype=bool)
    combos = list(combinations(range(X.shape[1]), k))
    out = np.zeros(len(combos), dtype=np.float32)
    total_case = float(is_case.sum())
    total_control = float((~is_case).sum())
    if total_case == 0 or total_control == 0:
        return out
    thr = total_case / total_control
    for i, combo in enumerate(combos):
        case, control = table(X, is_case, combo)
        with np.errstate(divide="ignore", invalid="ignore"):
            high = (control == 0) | (case / control > thr)
        tp = case[high].sum()
        tn = control[~high].sum()
        out[i] = np.float32((tp / total_case + tn / total_control) / 2.0)
    return out


def scan(X, is_case, k, fold=None, n_folds=0):
    """F x C(p,k) float32 BAs; fold f trains on the samples outside fold f."""
    is_case = np.asarray(is_case, dtype=bool)
    if fold is None:
        return all_bas(X, is_case, k)[None, :]
    return np.stack([all_bas(X[fold != f], is_case[fold != f], k) for f in range(n_folds)])


def lookup(X, y, combo):
    case, control = table(X, y == 1, combo)
    tc, tn = case.sum(), control.sum()
    thr = np.inf if tn == 0 else tc / tn
    return (case / (control + 1e-9) > thr).astype(np.uint8)


def predict(X, combo, lut):
    return lut[cells(X, combo)]


def fit(X, y, k, cv):
    """The whole fit: a dict of the fitted attributes."""
    X = np.asarray(X, dtype=np.uint8)
    combos = list(combinations(range(X.shape[1]), k))
    _, splits = fold_ids(X, y, cv)
    models, test_bas = [], []
    for tr, te in splits:
        bas = all_bas(X[tr], y[tr] == 1, k)
        combo = tuple(int(v) for v in combos[int(np.argmax(bas))])
        models.append(combo)
        pred = predict(X[te], combo, lookup(X[tr], y[tr], combo))
        yt = y[te]
        n_pos, n_neg = np.sum(yt == 1), np.sum(yt == 0)
        sens = np.sum((yt == 1) & (pred == 1)) / n_pos if n_pos else 0
        spec = np.sum((yt == 0) & (pred == 0)) / n_neg if n_neg else 0
        test_bas.append((sens + spec) / 2.0)
    counts = Counter(models)
    cvc = max(counts.values())
    best, best_ba = None, -1.0
    for m, c in counts.items():
        if c != cvc:
            continue
        avg = float(np.mean([b for b, mm in zip(test_bas, models) if mm == m]))
        if avg > best_ba:
            best, best_ba = m, avg
    return {"best_interaction_": best, "best_cvc_": cvc, "best_mean_testing_ba_": best_ba,
            "best_model_lookup_table_": lookup(X, y, best), "fold_models": models}


# (n, p, k, cv) of the full-array parity cases shared by the CPU and GPU tests
SHAPES = [(203, 40, 2, 5), (203, 14, 3, 3), (97, 9, 4, 2), (50, 7, 6, 2), (33, 5, 1, 2),
          (2049, 12, 2, 10)]
_CASES = {}


def case(n, p, k, cv):
    """(X, y, fold, expected F x C float32 BAs) of one parity case, computed
    once per session and shared read-only."""
    key = (n, p, k, cv)
    if key not in _CASES:
        X, y = planted(n, p)
        fold, _ = fold_ids(X, y, cv)
        ba = scan(X, y == 1, k, fold, cv)
        for a in (X, y, fold, ba):
            a.setflags(write=False)
        _CASES[key] = (X, y, fold, ba)
    return _CASES[key]


def noise_16x30():
    """The 16 x 30 noise set of the tie test (k = 3: many combinations share
    the maximum)."""
    rng = np.random.default_rng(11)
    X = rng.integers(0, 3, size=(16, 30)).astype(np.uint8)
    y = (np.arange(16) % 2).astype(np.uint8)
    return X, y
