"""fs_mdr_scan_labels on the GPU (k_mdr_scan_labels, fs_mdr.hip): every BA and
every (best BA, best rank) must equal the CPU backend's bit for bit -- all
quantities are integer counts until three float64 operations, so there is no
tolerance.  Shapes are the smallest at which the kernel can go wrong: a partly
filled wave of labellings, a full one, one more and three waves; folds shorter
than one 128-sample quad and folds of several quads of unequal sizes; one,
ten and more folds than a launch holds; more combinations than a block's run
of ranks."""
import numpy as np
import pytest

import mdr_np

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from fastselect_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    return _lib


def labellings(y, n_labelings, seed=1):
    rng = np.random.default_rng(seed)
    rows = [(y == 1).astype(np.uint8)]
    for _ in range(1, n_labelings):
        rows.append(rng.permutation(rows[0]))
    return np.stack(rows)


_DATA = {}


def data(n, p, cv):
    """(X, y, fold, cv) of one shape, drawn once per session."""
    key = (n, p, cv)
    if key not in _DATA:
        X, y = mdr_np.planted(n, p)
        fold = mdr_np.fold_ids(X, y, cv)[0] if cv else None
        _DATA[key] = (X, y, fold, cv)
    return _DATA[key]


def same_as_cpu(L, X, labels, k, fold, cv, want_ba=True):
    if want_ba:
        gb, gr, gba = L.mdr_scan_labels("gpu", X, labels, k, fold, cv, want_ba=True)
        cb, cr, cba = L.mdr_scan_labels("cpu", X, labels, k, fold, cv, want_ba=True)
        assert np.array_equal(gba.view(np.uint32), cba.view(np.uint32))
    else:
        gb, gr = L.mdr_scan_labels("gpu", X, labels, k, fold, cv)
        cb, cr = L.mdr_scan_labels("cpu", X, labels, k, fold, cv)
    assert np.array_equal(gb.view(np.uint32), cb.view(np.uint32))
    assert np.array_equal(gr, cr)
    return gb, gr


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("cv", [0, 10, 17])
@pytest.mark.parametrize("p,k", [(24, 1), (24, 2), (24, 3), (8, 6)])
@pytest.mark.parametrize("n", [203, 1100])
def test_gpu_equals_cpu(L, n, p, k, cv, B):
    X, y, fold, cv = data(n, p, cv)
    labels = labellings(y, B)
    gb, gr = same_as_cpu(L, X, labels, k, fold, cv)
    # without ba_out the kernel takes the same path but writes no array
    gb2, gr2 = L.mdr_scan_labels("gpu", X, labels, k, fold, cv)
    assert np.array_equal(gb2, gb) and np.array_equal(gr2, gr)


def test_more_combinations_than_one_run_of_ranks(L):
    """p = 120, k = 2: 7140 combinations, more than the 1024 blocks x 4 waves
    of one launch take in one step, so waves advance their combination
    (mdr_advance carries into the first column) and the blocks' slots meet in
    the device reduction."""
    X, y, fold, cv = data(400, 120, 5)
    labels = labellings(y, 65)
    _, gr = same_as_cpu(L, X, labels, 2, fold, cv)
    assert L.mdr_unrank(120, 2, int(gr[0, 0])) == (1, 118)   # the planted pair


def test_row_zero_equals_the_single_scan_on_the_device(L):
    for n, p, k, cv in [(203, 24, 2, 10), (1100, 24, 3, 17), (1100, 24, 2, 0)]:
        X, y, fold, cv = data(n, p, cv)
        labels = labellings(y, 3)
        gb, gr, gba = L.mdr_scan_labels("gpu", X, labels, k, fold, cv, want_ba=True)
        sb, sr, sba = L.mdr_scan("gpu", X, labels[0], k, fold, cv, want_ba=True)
        assert np.array_equal(gba[0].view(np.uint32), sba.view(np.uint32))
        assert np.array_equal(gb[0].view(np.uint32), sb.view(np.uint32))
        assert np.array_equal(gr[0], sr)


def test_duplicated_column_ties_and_all_controls(L):
    X, y = mdr_np.planted(203, 12, pair=(2, 5))
    X = np.concatenate([X, X[:, 5:6]], axis=1)
    fold, _ = mdr_np.fold_ids(X, y, 3)
    labels = labellings(y, 66)
    labels[65] = 0
    gb, gr = same_as_cpu(L, X, labels, 2, fold, 3)
    assert [L.mdr_unrank(13, 2, int(r)) for r in gr[0]] == [(2, 5)] * 3
    assert not gb[65].any() and not gr[65].any()


def test_genotype_above_two_is_rejected(L):
    X, y, fold, cv = data(203, 24, 10)
    X = X.copy()
    X[202, 23] = 3
    with pytest.raises(ValueError, match="0/1/2"):
        L.mdr_scan_labels("gpu", X, labellings(y, 2), 2, fold, cv)


def test_estimator_gpu_equals_cpu(L):
    from fastselect_amd import MDR
    rng = np.random.default_rng(0)
    X = rng.integers(0, 3, size=(400, 12)).astype(np.uint8)
    y = ((X[:, 3] + X[:, 8]) % 2).astype(np.uint8)
    g = MDR(k=2, cv=5, backend="gpu").permutation_test(X, y, 70, random_state=3)
    c = MDR(k=2, cv=5, backend="cpu").permutation_test(X, y, 70, random_state=3)
    assert g.effective_backend_ == "gpu" and c.effective_backend_ == "cpu"
    for name in ("best_interaction_", "best_cvc_", "best_mean_testing_ba_", "p_value_",
                 "cvc_p_value_", "n_permutations_"):
        assert getattr(g, name) == getattr(c, name), name
    for name in ("best_model_lookup_table_", "null_testing_ba_", "null_cvc_"):
        assert np.array_equal(getattr(g, name), getattr(c, name)), name
    assert np.array_equal(g.predict(X), c.predict(X))
