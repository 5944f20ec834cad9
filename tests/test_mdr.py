"""MDR on the CPU backend: the reference's known-answer data and validation
cases, bit-exact parity of fs_mdr_scan with the numpy restatement
(tests/mdr_np.py), ties, degenerate inputs and the estimator surface."""
import itertools
import os
import pickle

import numpy as np
import pytest

import mdr_np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "mdr_reference_fixtures.npz")


@pytest.fixture(scope="module")
def toy():
    d = np.load(GOLDEN)
    return d


def test_reference_known_answer(toy):
    from fastselect_amd import MDR
    X, y = toy["X"], toy["y"]
    clf = MDR(k=int(toy["k"]), cv=int(toy["cv"]), backend="cpu").fit(X, y)
    assert clf.best_interaction_ == tuple(int(v) for v in toy["best_interaction"]) == (0, 1)
    assert clf.best_cvc_ == int(toy["best_cvc"]) == 2
    assert abs(clf.best_mean_testing_ba_ - float(toy["best_mean_testing_ba"])) <= 1e-6
    pred = clf.predict(X)
    assert np.array_equal(pred, y)
    assert np.array_equal(clf.transform(X), pred.reshape(-1, 1))
    assert clf.best_model_lookup_table_.dtype == np.uint8
    assert clf.best_model_lookup_table_.shape == (9,)
    assert clf.n_features_in_ == 2 and clf.effective_backend_ == "cpu"
    assert list(clf.classes_) == [0, 1]
    with pytest.raises(NotImplementedError):
        clf.predict_proba(X)


@pytest.mark.parametrize("bad_y", [np.array([0, 0, 0, 2, 1, 1, 0, 1], dtype=np.uint8),
                                   np.zeros(8, dtype=np.uint8)])
def test_non_binary_y_is_rejected(toy, bad_y):
    from fastselect_amd import MDR
    with pytest.raises(ValueError, match="binary"):
        MDR(cv=2, backend="cpu").fit(toy["X"], bad_y)


def test_genotype_range_is_checked(toy):
    from fastselect_amd import MDR
    X, y = toy["X"], toy["y"]
    X3 = X.copy()
    X3[4, 1] = 3
    with pytest.raises(ValueError, match="0/1/2"):
        MDR(cv=2, backend="cpu").fit(X3, y)
    Xn = X.astype(np.int8)
    Xn[0, 0] = -1  # wraps to 255 in the uint8 cast, as in the reference
    with pytest.raises(ValueError, match="0/1/2"):
        MDR(cv=2, backend="cpu").fit(Xn, y)


def test_k_limits(toy):
    from fastselect_amd import MDR
    X, y = toy["X"], toy["y"]
    clf = MDR(k=X.shape[1], cv=2, backend="cpu").fit(X, y)  # k = n_features allowed
    assert clf.best_interaction_ == (0, 1)
    with pytest.raises(ValueError, match="n_features"):
        MDR(k=X.shape[1] + 1, cv=2, backend="cpu").fit(X, y)
    with pytest.raises(ValueError, match="MAX_K_FOR_KERNEL"):
        MDR(k=7, backend="cpu").fit(X, y)


def test_backend_spelling_and_missing_gpu(toy):
    from fastselect_amd import MDR, _lib
    X, y = toy["X"], toy["y"]
    clf = MDR(k=2, cv=2, backend="CPU").fit(X, y)
    assert clf.backend == "CPU" and clf.effective_backend_ == "cpu"
    with pytest.raises(ValueError, match="backend"):
        MDR(cv=2, backend="tpu").fit(X, y)
    if _lib.device_count() == 0:
        with pytest.raises(RuntimeError, match="no compatible"):
            MDR(k=2, cv=2, backend="gpu").fit(X, y)
        assert MDR(k=2, cv=2).fit(X, y).effective_backend_ == "cpu"


@pytest.mark.parametrize("n,p,k,cv", mdr_np.SHAPES)
def test_scan_equals_numpy(n, p, k, cv):
    from fastselect_amd import _lib
    X, y, fold, want = mdr_np.case(n, p, k, cv)
    best_ba, best_rank, ba = _lib.mdr_scan("cpu", X, y == 1, k, fold, cv, want_ba=True)
    assert ba.dtype == np.float32 and ba.shape == want.shape
    assert np.array_equal(ba, want)
    assert np.array_equal(best_rank, np.argmax(want, axis=1))
    assert np.array_equal(best_ba, want.max(axis=1))
    # the thread count changes nothing
    b1, r1 = _lib.mdr_scan("cpu", X, y == 1, k, fold, cv, n_jobs=1)
    assert np.array_equal(b1, best_ba) and np.array_equal(r1, best_rank)


def test_scan_without_folds_trains_on_all_samples():
    from fastselect_amd import _lib
    X, y, _, _ = mdr_np.case(203, 40, 2, 5)
    want = mdr_np.scan(X, y == 1, 2)
    best_ba, best_rank, ba = _lib.mdr_scan("cpu", X, y == 1, 2, want_ba=True)
    assert ba.shape == (1, 780) and np.array_equal(ba, want)
    assert best_rank[0] == np.argmax(want[0]) and best_ba[0] == want[0].max()
    # the planted pair (1, 38) wins
    assert _lib.mdr_unrank(40, 2, int(best_rank[0])) == (1, 38)


def test_labels_other_than_one_are_controls():
    """Labels {0, 2}: no sample equals 1, so every sample is a control and
    every BA is 0 -- the reference's rule, kept."""
    from fastselect_amd import MDR
    X, y, _, _ = mdr_np.case(97, 9, 4, 2)
    y2 = (y * 2).astype(np.uint8)
    clf = MDR(k=2, cv=2, backend="cpu").fit(X, y2)
    ref = mdr_np.fit(X, y2, 2, 2)
    assert clf.best_interaction_ == ref["best_interaction_"] == (0, 1)


def test_duplicated_column_ties_go_to_the_earlier_copy():
    from fastselect_amd import MDR, _lib
    X, y = mdr_np.planted(203, 12, pair=(2, 5))
    X = np.concatenate([X, X[:, 5:6]], axis=1)  # column 12 duplicates column 5
    fold, _ = mdr_np.fold_ids(X, y, 3)
    _, best_rank, ba = _lib.mdr_scan("cpu", X, y == 1, 2, fold, 3, want_ba=True)
    combos = list(itertools.combinations(range(13), 2))
    assert np.array_equal(ba[:, combos.index((2, 5))], ba[:, combos.index((2, 12))])
    assert [combos[r] for r in best_rank] == [(2, 5)] * 3
    assert MDR(k=2, cv=3, backend="cpu").fit(X, y).best_interaction_ == (2, 5)


def test_noise_ties_take_the_first_maximum():
    from fastselect_amd import _lib
    X, y = mdr_np.noise_16x30()
    want = mdr_np.scan(X, y == 1, 3)
    best_ba, best_rank, ba = _lib.mdr_scan("cpu", X, y == 1, 3, want_ba=True)
    assert np.array_equal(ba, want)
    assert np.sum(want[0] == want[0].max()) > 1  # ties are the norm
    assert best_rank[0] == np.argmax(want[0]) and best_ba[0] == want[0].max()


def test_all_controls_gives_zero_and_rank_zero():
    from fastselect_amd import _lib
    X, y, fold, _ = mdr_np.case(203, 14, 3, 3)
    zero = np.zeros(203, dtype=np.uint8)
    best_ba, best_rank, ba = _lib.mdr_scan("cpu", X, zero, 3, fold, 3, want_ba=True)
    assert not ba.any() and not best_ba.any() and not best_rank.any()
    best_ba, best_rank = _lib.mdr_scan("cpu", X, zero, 3)
    assert best_ba[0] == 0.0 and best_rank[0] == 0


def test_k_equal_p_is_one_combination():
    from fastselect_amd import _lib
    X, y, fold, _ = mdr_np.case(50, 7, 6, 2)
    X5 = np.ascontiguousarray(X[:, :5])
    want = mdr_np.scan(X5, y == 1, 5, fold, 2)
    best_ba, best_rank, ba = _lib.mdr_scan("cpu", X5, y == 1, 5, fold, 2, want_ba=True)
    assert ba.shape == (2, 1) and np.array_equal(ba, want)
    assert not best_rank.any() and _lib.mdr_combinations(5, 5) == 1


def test_unrank_is_itertools_order():
    from fastselect_amd import _lib
    combos = list(itertools.combinations(range(9), 4))
    assert _lib.mdr_combinations(9, 4) == len(combos)
    for r, c in enumerate(combos):
        assert _lib.mdr_unrank(9, 4, r) == c
    # large ranks: the last combination of 2400 columns at k = 3, and k = 6
    c3 = _lib.mdr_combinations(2400, 3)
    assert c3 == 2400 * 2399 * 2398 // 6 > 2 ** 31
    assert _lib.mdr_unrank(2400, 3, c3 - 1) == (2397, 2398, 2399)
    assert _lib.mdr_unrank(2400, 3, c3 - 2) == (2396, 2398, 2399)
    c6 = _lib.mdr_combinations(3000, 6)
    assert _lib.mdr_unrank(3000, 6, c6 - 1) == tuple(range(2994, 3000))
    assert _lib.mdr_unrank(3000, 6, 0) == tuple(range(6))
    with pytest.raises(ValueError):
        _lib.mdr_unrank(9, 4, len(combos))


@pytest.mark.parametrize("n,p,k,cv", [(203, 40, 2, 5), (203, 14, 3, 3), (97, 9, 4, 2)])
def test_estimator_equals_numpy_fit(n, p, k, cv):
    from fastselect_amd import MDR
    X, y, _, _ = mdr_np.case(n, p, k, cv)
    Xtr, ytr, Xte = X[:-40], y[:-40], X[-40:]
    clf = MDR(k=k, cv=cv, backend="cpu").fit(Xtr, ytr)
    ref = mdr_np.fit(Xtr, ytr, k, cv)
    assert clf.best_interaction_ == ref["best_interaction_"]
    assert all(isinstance(v, int) for v in clf.best_interaction_)
    assert clf.best_cvc_ == ref["best_cvc_"]
    assert clf.best_mean_testing_ba_ == ref["best_mean_testing_ba_"]
    assert np.array_equal(clf.best_model_lookup_table_, ref["best_model_lookup_table_"])
    assert clf.best_model_lookup_table_.dtype == np.uint8
    assert np.array_equal(clf.predict(Xte), mdr_np.predict(Xte, ref["best_interaction_"],
                                                           ref["best_model_lookup_table_"]))


def test_clone_params_and_pickle_round_trip():
    from sklearn.base import clone
    from fastselect_amd import MDR
    est = MDR(k=3, cv=4, backend="CPU", verbose=False, n_jobs=2, device=0)
    assert est.get_params() == {"k": 3, "cv": 4, "backend": "CPU", "verbose": False,
                                "n_jobs": 2, "device": 0}
    assert clone(est).get_params() == est.get_params()
    assert MDR.__module__ == "fastselect_amd"
    X, y, _, _ = mdr_np.case(203, 14, 3, 3)
    est = MDR(k=2, cv=3, backend="cpu").fit(X, y)
    back = pickle.loads(pickle.dumps(est))
    assert back.best_interaction_ == est.best_interaction_
    assert np.array_equal(back.predict(X), est.predict(X))


def test_readme_pipeline_runs():
    from sklearn.pipeline import Pipeline
    from fastselect_amd import MDR, MultiSURF
    X, y = mdr_np.planted(160, 60, pair=(7, 41))
    pipe = Pipeline([("filter", MultiSURF(n_features_to_select=50)), ("mdr", MDR(k=2, cv=3))])
    pred = pipe.fit(X, y).predict(X)
    assert pred.shape == (160,) and set(np.unique(pred)) <= {0, 1}
    assert pipe.named_steps["mdr"].n_features_in_ == 50
