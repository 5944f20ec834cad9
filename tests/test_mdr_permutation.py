"""MDR.permutation_test on the CPU backend: the fit it reports is fit's own,
the null comes from one batched scan that agrees with single scans end to
end, and the p-values follow (1 + #{null >= observed}) / (1 + B)."""
import pickle

import numpy as np
import pytest

import mdr_np
from fastselect_amd import MDR, _lib
from fastselect_amd.MDR import summarise_folds

FIT_ATTRS = ("best_interaction_", "best_cvc_", "best_mean_testing_ba_", "n_features_in_",
             "effective_backend_")


@pytest.fixture(scope="module")
def xor():
    """n = 400, p = 12: the case flag is the parity of columns 3 and 8."""
    rng = np.random.default_rng(0)
    X = rng.integers(0, 3, size=(400, 12)).astype(np.uint8)
    y = ((X[:, 3] + X[:, 8]) % 2).astype(np.uint8)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


@pytest.fixture(scope="module")
def tested(xor):
    X, y = xor
    return MDR(k=2, cv=5, backend="cpu").permutation_test(X, y, 19, random_state=0)


def test_fit_attributes_equal_fit(xor, tested):
    X, y = xor
    f = MDR(k=2, cv=5, backend="cpu").fit(X, y)
    for name in FIT_ATTRS:
        assert getattr(tested, name) == getattr(f, name), name
    assert np.array_equal(tested.classes_, f.classes_)
    assert np.array_equal(tested.best_model_lookup_table_, f.best_model_lookup_table_)
    assert np.array_equal(tested.predict(X), f.predict(X))
    want = mdr_np.fit(X, y, 2, 5)
    assert tested.best_interaction_ == want["best_interaction_"] == (3, 8)
    assert tested.best_mean_testing_ba_ == want["best_mean_testing_ba_"]


def test_planted_pair_gets_the_smallest_p_value(tested):
    assert tested.n_permutations_ == 19
    assert tested.null_testing_ba_.shape == (19,) and tested.null_testing_ba_.dtype == np.float64
    assert tested.null_cvc_.shape == (19,) and tested.null_cvc_.dtype.kind == "i"
    assert tested.p_value_ == 1 / 20
    assert tested.best_cvc_ == 5
    assert tested.cvc_p_value_ == (1 + int(np.sum(tested.null_cvc_ >= 5))) / 20
    assert np.all(tested.null_testing_ba_ < tested.best_mean_testing_ba_)


def test_p_value_counts_ties_and_larger_nulls():
    """Pure noise: the observed statistic sits inside its null."""
    rng = np.random.default_rng(8)
    X = rng.integers(0, 3, size=(120, 6)).astype(np.uint8)
    y = rng.integers(0, 2, size=120).astype(np.uint8)
    m = MDR(k=2, cv=3, backend="cpu").permutation_test(X, y, 29, random_state=1)
    ge = int(np.sum(m.null_testing_ba_ >= m.best_mean_testing_ba_))
    assert ge > 0 and m.p_value_ == (1 + ge) / 30
    assert m.cvc_p_value_ == (1 + int(np.sum(m.null_cvc_ >= m.best_cvc_))) / 30


def test_seed_decides_the_null(xor, tested):
    X, y = xor
    again = MDR(k=2, cv=5, backend="cpu").permutation_test(X, y, 19, random_state=0)
    assert np.array_equal(again.null_testing_ba_, tested.null_testing_ba_)
    assert np.array_equal(again.null_cvc_, tested.null_cvc_)
    other = MDR(k=2, cv=5, backend="cpu").permutation_test(X, y, 19, random_state=1)
    assert not np.array_equal(other.null_testing_ba_, tested.null_testing_ba_)


def test_null_equals_single_scans_through_the_shared_helper(xor, tested):
    """The documented draw (default_rng(seed); labellings in order, folds in
    order, rng.permutation of the fold's flags), one fs_mdr_scan per labelling
    and the helper fit uses give the same null, value for value."""
    X, y = xor
    fold, splits = mdr_np.fold_ids(X, y, 5)
    rng = np.random.default_rng(0)
    flags = (y == 1).astype(np.uint8)
    for b in range(19):
        lab = np.empty_like(flags)
        for _, te in splits:
            lab[te] = rng.permutation(flags[te])
        for f in range(5):   # permuting within folds keeps every fold's class counts
            assert lab[fold == f].sum() == flags[fold == f].sum()
        _, rank = _lib.mdr_scan("cpu", X, lab, 2, fold, 5)
        _, cvc, ba = summarise_folds(X, lab, splits, rank, 2)
        assert tested.null_testing_ba_[b] == ba, b
        assert tested.null_cvc_[b] == cvc, b


def test_labels_other_than_zero_and_one(xor):
    """Cases are the samples labelled 1, whatever the other label is."""
    X, y = xor
    y2 = np.where(y == 1, 1, 2)
    a = MDR(k=2, cv=5, backend="cpu").permutation_test(X, y2, 5, random_state=0)
    f = MDR(k=2, cv=5, backend="cpu").fit(X, y2)
    assert a.best_interaction_ == f.best_interaction_
    assert a.best_mean_testing_ba_ == f.best_mean_testing_ba_


@pytest.mark.parametrize("bad", [0, -3])
def test_n_permutations_below_one_raises(xor, bad):
    X, y = xor
    with pytest.raises(ValueError, match="n_permutations"):
        MDR(k=2, cv=5, backend="cpu").permutation_test(X, y, bad)


def test_validates_as_fit(xor):
    X, y = xor
    with pytest.raises(ValueError, match="0/1/2"):
        MDR(backend="cpu").permutation_test(np.where(X == 2, 3, X), y, 3)
    with pytest.raises(ValueError, match="binary"):
        MDR(backend="cpu").permutation_test(X, np.arange(400) % 3, 3)


def test_get_params_is_unchanged():
    assert MDR().get_params() == {"k": 2, "cv": 10, "backend": "auto", "verbose": False,
                                  "n_jobs": -1, "device": 0}


def test_pickle_keeps_the_new_attributes(xor, tested):
    X, _ = xor
    back = pickle.loads(pickle.dumps(tested))
    assert back.p_value_ == tested.p_value_ and back.cvc_p_value_ == tested.cvc_p_value_
    assert back.n_permutations_ == 19
    assert np.array_equal(back.null_testing_ba_, tested.null_testing_ba_)
    assert np.array_equal(back.null_cvc_, tested.null_cvc_)
    assert np.array_equal(back.predict(X), tested.predict(X))
