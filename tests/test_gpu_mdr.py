"""MDR on the GPU (fs_mdr.hip): every balanced accuracy and every fold's
(best BA, best rank) must equal the CPU backend's and the numpy restatement's
bit for bit -- all quantities are integer counts until three float64
operations, so there is no tolerance.  Shapes are the smallest at which the
kernels can go wrong: segments that are no multiple of 32 samples, n one over
a word boundary, ~10-sample segments (cv = 10), more columns than one block of
lanes, rows of the combination triangle shorter and longer than a block, more
folds than one launch holds in registers, and ranks above 2^31."""
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


def _same_as_cpu(L, X, is_case, k, fold=None, n_folds=0):
    gb, gr, gba = L.mdr_scan("gpu", X, is_case, k, fold, n_folds, want_ba=True)
    cb, cr, cba = L.mdr_scan("cpu", X, is_case, k, fold, n_folds, want_ba=True)
    assert np.array_equal(gba, cba)
    assert np.array_equal(gb, cb) and np.array_equal(gr, cr)
    # without ba_out the kernels take the same path but write no array
    gb2, gr2 = L.mdr_scan("gpu", X, is_case, k, fold, n_folds)
    assert np.array_equal(gb2, cb) and np.array_equal(gr2, cr)
    return gb, gr, gba


@pytest.mark.parametrize("n,p,k,cv", mdr_np.SHAPES)
def test_scan_equals_cpu_and_numpy(L, n, p, k, cv):
    X, y, fold, want = mdr_np.case(n, p, k, cv)
    gb, gr, gba = _same_as_cpu(L, X, y == 1, k, fold, cv)
    assert np.array_equal(gba, want)
    assert np.array_equal(gr, np.argmax(want, axis=1))
    assert np.array_equal(gb, want.max(axis=1))


def test_scan_without_folds(L):
    X, y, _, _ = mdr_np.case(203, 40, 2, 5)
    _, _, gba = _same_as_cpu(L, X, y == 1, 2)
    assert np.array_equal(gba, mdr_np.scan(X, y == 1, 2))


@pytest.mark.parametrize("n,p,cv", [(64, 130, 3), (40, 65, 0)])
def test_pairs_across_block_edges(L, n, p, cv):
    """k = 2 with rows of the pair triangle longer and shorter than a block
    of 256 lanes, and column counts one over a multiple of 64."""
    X, y = mdr_np.planted(n, p, pair=(3, p - 1))
    fold = mdr_np.fold_ids(X, y, cv)[0] if cv else None
    _same_as_cpu(L, X, y == 1, 2, fold, cv)


def test_triples_across_block_edges(L):
    X, y = mdr_np.planted(64, 70, pair=(0, 69))
    fold, _ = mdr_np.fold_ids(X, y, 2)
    _same_as_cpu(L, X, y == 1, 3, fold, 2)


def test_more_folds_than_one_launch_holds(L):
    """cv = 20 runs in two groups of folds (16 + 4), each walking the other
    folds' words for the cell totals."""
    X, y = mdr_np.planted(400, 10, pair=(2, 7))
    fold, _ = mdr_np.fold_ids(X, y, 20)
    _, _, gba = _same_as_cpu(L, X, y == 1, 2, fold, 20)
    assert np.array_equal(gba, mdr_np.scan(X, y == 1, 2, fold, 20))


def test_duplicated_column_ties_go_to_the_earlier_copy(L):
    X, y = mdr_np.planted(203, 12, pair=(2, 5))
    X = np.concatenate([X, X[:, 5:6]], axis=1)
    fold, _ = mdr_np.fold_ids(X, y, 3)
    _, gr, _ = _same_as_cpu(L, X, y == 1, 2, fold, 3)
    assert [L.mdr_unrank(13, 2, int(r)) for r in gr] == [(2, 5)] * 3


def test_noise_ties_take_the_first_maximum(L):
    X, y = mdr_np.noise_16x30()
    gb, gr, gba = _same_as_cpu(L, X, y == 1, 3)
    assert np.sum(gba[0] == gba[0].max()) > 1
    assert gr[0] == np.argmax(gba[0]) and gb[0] == gba[0].max()


def test_all_controls_gives_zero_and_rank_zero(L):
    X, y, fold, _ = mdr_np.case(203, 14, 3, 3)
    zero = np.zeros(203, dtype=np.uint8)
    gb, gr, gba = _same_as_cpu(L, X, zero, 3, fold, 3)
    assert not gba.any() and not gb.any() and not gr.any()


def test_genotype_above_two_is_rejected(L):
    X, y, _, _ = mdr_np.case(203, 14, 3, 3)
    X = X.copy()
    X[202, 13] = 3
    with pytest.raises(ValueError, match="0/1/2"):
        L.mdr_scan("gpu", X, y == 1, 2)


def test_ranks_above_2_to_31(L):
    """p = 2400, k = 3: 2.30e9 combinations.  y is the parity of the LAST
    three columns' genotype sum, so the last rank alone reaches BA 1.0 (at
    n = 256 no random triple separates the classes): any spurious tie, and
    any rank computed in 32 bits, fails.  Not compared with the CPU backend,
    which would take minutes."""
    p, n = 2400, 256
    rng = np.random.default_rng(5)
    X = rng.integers(0, 3, size=(n, p)).astype(np.uint8)
    y = ((X[:, p - 3].astype(int) + X[:, p - 2] + X[:, p - 1]) % 2).astype(np.uint8)
    count = L.mdr_combinations(p, 3)
    assert count == 2400 * 2399 * 2398 // 6 and count > 2 ** 31
    best_ba, best_rank = L.mdr_scan("gpu", X, y == 1, 3)
    assert best_ba[0] == np.float32(1.0)
    assert best_rank[0] == count - 1
    assert L.mdr_unrank(p, 3, int(best_rank[0])) == (p - 3, p - 2, p - 1)


@pytest.mark.parametrize("n,p,k,cv", [(203, 40, 2, 5), (203, 14, 3, 3)])
def test_estimator_gpu_equals_cpu(L, n, p, k, cv):
    from fastselect_amd import MDR
    X, y, _, _ = mdr_np.case(n, p, k, cv)
    g = MDR(k=k, cv=cv, backend="gpu").fit(X, y)
    c = MDR(k=k, cv=cv, backend="cpu").fit(X, y)
    assert g.effective_backend_ == "gpu" and c.effective_backend_ == "cpu"
    assert g.best_interaction_ == c.best_interaction_
    assert g.best_cvc_ == c.best_cvc_
    assert g.best_mean_testing_ba_ == c.best_mean_testing_ba_
    assert np.array_equal(g.best_model_lookup_table_, c.best_model_lookup_table_)
    assert np.array_equal(g.predict(X), c.predict(X))
    assert MDR(k=k, cv=cv).fit(X, y).effective_backend_ == "gpu"  # 'auto' with a device


def test_readme_pipeline_on_auto(L):
    from sklearn.pipeline import Pipeline
    from fastselect_amd import MDR, MultiSURF
    X, y = mdr_np.planted(160, 60, pair=(7, 41))
    pipe = Pipeline([("filter", MultiSURF(n_features_to_select=50)), ("mdr", MDR(k=2, cv=3))])
    pred = pipe.fit(X, y).predict(X)
    assert pipe.named_steps["mdr"].effective_backend_ == "gpu"
    assert pred.shape == (160,)
