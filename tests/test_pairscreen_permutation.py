"""PairScreen.permutation_test and mutual_information.pair_screen_null on the
CPU backend: the max-T permutation test of the pair screen.

The two data cases were checked in numpy first.  On
pairscan_np.pure(400, 20, 11, 7, 13, 2) the observed gain is 0.649 bit against
a null maximum of 0.027 over 99 permutations: p = 1 / 100 exactly.  On 300 x 20
uniform noise the observed 0.0330 is more than 2e-5 from every null value and
numpy's p is 0.90: no backend's rounding moves the count."""
import pickle

import numpy as np
import pytest

import pairscan_np
from fastselect_amd import PairScreen
from fastselect_amd import mutual_information as mi

FIT_ATTRS = ("relevance_scores_", "top_scores_", "top_pairs_", "interaction_scores_",
             "feature_importances_", "top_features_", "n_features_in_", "effective_backend_")
PERM_ATTRS = ("null_max_scores_", "null_best_pairs_", "n_permutations_", "p_value_",
              "top_p_values_")


def _planted():
    return pairscan_np.pure(400, 20, 11, 7, 13, 2)


def _noise():
    rng = np.random.default_rng(21)
    X = rng.integers(0, 3, (300, 20))
    y = rng.integers(0, 2, 300)
    return X, y


@pytest.fixture(scope="module")
def planted_test():
    X, y = _planted()
    return PairScreen(4, n_top=12, backend="cpu").permutation_test(X, y, 99, random_state=5)


def test_sets_what_fit_sets(planted_test):
    X, y = _planted()
    fitted = PairScreen(4, n_top=12, backend="cpu").fit(X, y)
    for name in FIT_ATTRS:
        a, b = getattr(planted_test, name), getattr(fitted, name)
        assert np.array_equal(a, b), name
        assert np.asarray(a).dtype == np.asarray(b).dtype, name
    for name in PERM_ATTRS:
        assert not hasattr(fitted, name)
    assert planted_test.null_max_scores_.shape == (99,)
    assert planted_test.null_max_scores_.dtype == np.float64
    assert planted_test.null_best_pairs_.shape == (99, 2)
    assert planted_test.n_permutations_ == 99
    assert np.array_equal(planted_test.transform(X), fitted.transform(X))


def test_planted_pair_is_significant(planted_test):
    assert tuple(planted_test.top_pairs_[0]) == (7, 13)
    assert planted_test.p_value_ == 0.01
    assert planted_test.top_scores_[0] > 0.6 and planted_test.null_max_scores_.max() < 0.05


def test_p_values_down_the_list(planted_test):
    t = planted_test
    assert t.top_p_values_.shape == t.top_scores_.shape
    assert t.top_p_values_[0] == t.p_value_
    assert np.all(np.diff(t.top_p_values_) >= 0.0)
    for k, s in enumerate(t.top_scores_):
        assert t.top_p_values_[k] == (1 + np.count_nonzero(t.null_max_scores_ >= s)) / 100
    # below the planted pair the list is noise: no better than the null's best
    assert t.top_p_values_[1] > 0.05


def test_noise_is_not_significant():
    X, y = _noise()
    t = PairScreen(4, backend="cpu").permutation_test(X, y, 99, random_state=5)
    assert t.p_value_ > 0.05
    # the observed score is isolated from every null value
    assert np.abs(t.null_max_scores_ - t.top_scores_[0]).min() > 2e-5
    assert t.p_value_ == pytest.approx(0.90, abs=0.005)


def test_reproducible_under_random_state():
    X, y = _noise()
    a = PairScreen(4, backend="cpu").permutation_test(X, y, 20, random_state=3)
    b = PairScreen(4, backend="cpu").permutation_test(X, y, 20, random_state=3)
    c = PairScreen(4, backend="cpu").permutation_test(X, y, 20, random_state=4)
    assert np.array_equal(a.null_max_scores_, b.null_max_scores_)
    assert np.array_equal(a.null_best_pairs_, b.null_best_pairs_)
    assert a.p_value_ == b.p_value_
    assert not np.array_equal(a.null_max_scores_, c.null_max_scores_)


@pytest.mark.parametrize("score", ["gain", "joint"])
def test_null_is_the_loop_of_single_screens(score):
    X, y = _noise()
    t = PairScreen(4, score=score, backend="cpu").permutation_test(X, y, 12, random_state=9)
    rng = np.random.default_rng(9)
    ycodes = np.unique(y, return_inverse=True)[1].astype(np.uint8)
    for b in range(12):
        perm = rng.permutation(ycodes)
        pairs, scores, _, _ = mi.rank_pair_interactions(X, perm, n_top=1, score=score,
                                                        backend="cpu")
        assert t.null_max_scores_[b] == scores[0], b
        assert tuple(t.null_best_pairs_[b]) == tuple(pairs[0]), b


def test_pair_screen_null_on_two_traits():
    """Trait 0 is the XOR of columns 1 and 4, trait 1 copies column 2: each row
    of the batch is that trait's own screen."""
    rng = np.random.default_rng(8)
    X = rng.integers(0, 2, (200, 6))
    labels = np.stack([X[:, 1] ^ X[:, 4], X[:, 2]])
    pairs, scores, rel = mi.pair_screen_null(X, labels, score="joint", backend="cpu")
    assert pairs.shape == (2, 2) and scores.shape == (2,) and rel.shape == (2, 6)
    assert tuple(pairs[0]) == (1, 4) and scores[0] == pytest.approx(1.0, abs=0.02)
    assert 2 in tuple(pairs[1]) and rel[1, 2] == pytest.approx(1.0, abs=0.02)
    for b in range(2):
        p1, s1, r1, _ = mi.rank_pair_interactions(X, labels[b], n_top=1, score="joint",
                                                  backend="cpu")
        assert scores[b] == s1[0] and tuple(pairs[b]) == tuple(p1[0])
        assert np.array_equal(rel[b], r1)
    with pytest.raises(ValueError, match="2‑D"):
        mi.pair_screen_null(X, labels[0], backend="cpu")
    with pytest.raises(ValueError, match="integer"):
        mi.pair_screen_null(X, labels.astype(float), backend="cpu")
    with pytest.raises(ValueError, match="two columns"):
        mi.pair_screen_null(X[:, :1], labels, backend="cpu")


def test_parameter_errors():
    X, y = _noise()
    for bad in (0, -1, 2.5, 65535):
        with pytest.raises(ValueError, match="n_permutations"):
            PairScreen(4, backend="cpu").permutation_test(X, y, bad)
    with pytest.raises(ValueError, match="score"):
        PairScreen(4, score="sum", backend="cpu").permutation_test(X, y, 5)
    with pytest.raises(ValueError, match="n_features_to_select"):
        PairScreen(40, backend="cpu").permutation_test(X, y, 5)


def test_pickle_after_permutation_test(planted_test):
    back = pickle.loads(pickle.dumps(planted_test))
    for name in FIT_ATTRS + PERM_ATTRS:
        assert np.array_equal(getattr(back, name), getattr(planted_test, name)), name
    X, _ = _planted()
    assert np.array_equal(back.transform(X), planted_test.transform(X))
