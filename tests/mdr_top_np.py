"""numpy restatement of the MDR top-N contract on top of mdr_np (helper, not
collected): the expected lists of fs_mdr_scan_top and the attributes of
``MDR.rank_interactions``."""
from itertools import combinations

import numpy as np

import mdr_np


def expected(ba, n_top):
    """(top_ba, top_rank) of an F x C array of float32 BAs: per fold
    ``np.argsort(-ba, kind="stable")[:n_top]``, padded with rank -1, BA 0."""
    F, C = ba.shape
    top_ba = np.zeros((F, n_top), dtype=np.float32)
    top_rank = np.full((F, n_top), -1, dtype=np.int64)
    m = min(n_top, C)
    for f in range(F):
        order = np.argsort(-ba[f], kind="stable")[:m]
        top_rank[f, :m] = order
        top_ba[f, :m] = ba[f, order]
    return top_ba, top_rank


def same_bits(a, b):
    """float32 arrays equal as bit patterns."""
    return (a.dtype == b.dtype == np.float32 and a.shape == b.shape
            and np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                               np.ascontiguousarray(b).view(np.uint32)))


def same(got, want):
    """(top_ba, top_rank) pairs equal bit for bit."""
    return same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])


def fold_test_ba(X, y, combo, tr, te):
    """Test BA of one model in one fold: lookup table on the training rows."""
    pred = mdr_np.predict(X[te], combo, mdr_np.lookup(X[tr], y[tr], combo))
    yt = y[te]
    n_pos, n_neg = np.sum(yt == 1), np.sum(yt == 0)
    sens = np.sum((yt == 1) & (pred == 1)) / n_pos if n_pos else 0
    spec = np.sum((yt == 0) & (pred == 0)) / n_neg if n_neg else 0
    return (sens + spec) / 2.0


def landscape(X, y, k, cv, n_top):
    """The attributes ``rank_interactions`` adds, as a dict."""
    combos = list(combinations(range(X.shape[1]), k))
    fold, splits = mdr_np.fold_ids(X, y, cv)
    _, all_rank = expected(mdr_np.scan(X, y == 1, k), n_top)
    _, fold_rank = expected(mdr_np.scan(X, y == 1, k, fold, cv), n_top)
    ranks = all_rank[0][all_rank[0] >= 0]
    ba_all = mdr_np.scan(X, y == 1, k)[0]
    return {
        "top_interactions_": np.array([combos[r] for r in ranks], dtype=np.int64).reshape(-1, k),
        "top_training_ba_": ba_all[ranks],
        "top_mean_testing_ba_": np.array(
            [np.mean([fold_test_ba(X, y, combos[r], tr, te) for tr, te in splits]) for r in ranks]),
        "top_cvc_": np.array([np.sum(fold_rank[:, 0] == r) for r in ranks]),
        "top_fold_hits_": np.array([np.sum(np.any(fold_rank == r, axis=1)) for r in ranks]),
    }


FIT_ATTRS = ("best_interaction_", "best_cvc_", "best_mean_testing_ba_", "classes_",
             "n_features_in_", "effective_backend_")
TOP_ATTRS = ("top_interactions_", "top_training_ba_", "top_mean_testing_ba_", "top_cvc_",
             "top_fold_hits_")


def check_estimator(backend, n, p, k, cv, n_top):
    """``rank_interactions`` against ``fit`` and against ``landscape``; the
    fitted estimator."""
    from fastselect_amd import MDR, _lib
    X, y, _, _ = mdr_np.case(n, p, k, cv)
    est = MDR(k=k, cv=cv, backend=backend).rank_interactions(X, y, n_top=n_top)
    fit = MDR(k=k, cv=cv, backend=backend).fit(X, y)
    for name in FIT_ATTRS:
        assert np.array_equal(getattr(est, name), getattr(fit, name)), name
    assert np.array_equal(est.best_model_lookup_table_, fit.best_model_lookup_table_)
    assert np.array_equal(est.predict(X), fit.predict(X))
    want = landscape(X, y, k, cv, n_top)
    m = min(n_top, _lib.mdr_combinations(p, k))
    assert est.top_interactions_.shape == (m, k)
    assert est.top_training_ba_.dtype == np.float32
    assert est.top_mean_testing_ba_.dtype == np.float64
    for name in TOP_ATTRS:
        assert np.array_equal(getattr(est, name), want[name]), name
    return est
