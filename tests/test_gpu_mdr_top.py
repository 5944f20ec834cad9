"""fs_mdr_scan_top on the GPU (fs_mdr.hip): every list must equal the CPU
backend's and the numpy restatement's bit for bit -- a histogram scan, a
threshold and a collecting scan select among integers-until-three-float64-ops
BAs, so there is no tolerance.  Shapes are the smallest at which this can go
wrong: the parity shapes of the plain scan, masses of equal BAs inside the
threshold bin, a duplicated column, two fold groups, rank runs that cross
block edges, one class only, the bounded-memory route forced by a small
candidate cap, and ranks above 2^31."""
import numpy as np
import pytest

import mdr_np
from mdr_top_np import expected, same, same_bits

pytestmark = pytest.mark.gpu

TOPS = (1, 7, 300)


@pytest.fixture(scope="module")
def L():
    from fastselect_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    return _lib


def _same_as_cpu(L, X, is_case, k, fold=None, n_folds=0, n_top=7, want=None):
    g = L.mdr_scan_top("gpu", X, is_case, k, fold, n_folds, n_top=n_top)
    c = L.mdr_scan_top("cpu", X, is_case, k, fold, n_folds, n_top=n_top)
    assert same(g, c)
    if want is not None:
        assert same(g, expected(want, n_top))
    return g


@pytest.mark.parametrize("n_top", TOPS)
@pytest.mark.parametrize("n,p,k,cv", mdr_np.SHAPES)
def test_top_equals_cpu_and_numpy(L, n, p, k, cv, n_top):
    X, y, fold, ba = mdr_np.case(n, p, k, cv)
    g = _same_as_cpu(L, X, y == 1, k, fold, cv, n_top, ba)
    best = L.mdr_scan("gpu", X, y == 1, k, fold, cv)
    assert same_bits(g[0][:, 0], best[0]) and np.array_equal(g[1][:, 0], best[1])


def test_top_without_folds(L):
    X, y, _, _ = mdr_np.case(203, 40, 2, 5)
    _same_as_cpu(L, X, y == 1, 2, n_top=300, want=mdr_np.scan(X, y == 1, 2))


@pytest.fixture(scope="module")
def noise():
    X, y = mdr_np.noise_16x30()
    return X, y, mdr_np.scan(X, y == 1, 3)


def test_ties_inside_the_threshold_bin(L, noise):
    """4060 triples on 16 samples: far more than n_top share the threshold
    bin, and exact keys repeat across the cut."""
    X, y, ba = noise
    want = expected(ba, 100)
    assert np.sum(ba[0] >= want[0][0, -1]) > 100
    _same_as_cpu(L, X, y == 1, 3, n_top=100, want=ba)


def test_duplicated_column_keeps_both_copies_in_rank_order(L):
    X, y = mdr_np.planted(203, 12, pair=(2, 5))
    X = np.concatenate([X, X[:, 5:6]], axis=1)
    fold, _ = mdr_np.fold_ids(X, y, 3)
    g = _same_as_cpu(L, X, y == 1, 2, fold, 3, n_top=7,
                     want=mdr_np.scan(X, y == 1, 2, fold, 3))
    for f in range(3):
        assert [L.mdr_unrank(13, 2, int(r)) for r in g[1][f, :2]] == [(2, 5), (2, 12)]
        assert g[0][f, 0] == g[0][f, 1]


def test_more_folds_than_one_launch_holds(L):
    X, y = mdr_np.planted(400, 10, pair=(2, 7))
    fold, _ = mdr_np.fold_ids(X, y, 20)
    _same_as_cpu(L, X, y == 1, 2, fold, 20, n_top=7, want=mdr_np.scan(X, y == 1, 2, fold, 20))


@pytest.mark.parametrize("n_top", (7, 300))
def test_pairs_across_block_edges(L, n_top):
    X, y = mdr_np.planted(64, 130, pair=(3, 129))
    fold, _ = mdr_np.fold_ids(X, y, 3)
    _same_as_cpu(L, X, y == 1, 2, fold, 3, n_top=n_top)


def test_triples_across_block_edges(L):
    X, y = mdr_np.planted(64, 70, pair=(0, 69))
    fold, _ = mdr_np.fold_ids(X, y, 2)
    _same_as_cpu(L, X, y == 1, 3, fold, 2, n_top=300)


def test_all_controls_lists_the_first_ranks(L):
    X, y, fold, _ = mdr_np.case(203, 14, 3, 3)
    zero = np.zeros(203, dtype=np.uint8)
    g = _same_as_cpu(L, X, zero, 3, fold, 3, n_top=300)
    assert not g[0].any()
    assert np.array_equal(g[1], np.tile(np.arange(300), (3, 1)))


@pytest.mark.parametrize("cap", (1, 64, 1000))
def test_small_candidate_cap_gives_the_same_bits(L, hooks, noise, cap):
    """The bounded-memory route: rank chunks, a running list per fold and a
    threshold that rises as the lists fill."""
    X, y, ba = noise
    plain = L.mdr_scan_top("gpu", X, y == 1, 3, n_top=100)
    Xs, ys, folds, bas = mdr_np.case(203, 40, 2, 5)
    plain_s = L.mdr_scan_top("gpu", Xs, ys == 1, 2, folds, 5, n_top=300)
    hooks("mdr_top_cap", cap)
    assert same(L.mdr_scan_top("gpu", X, y == 1, 3, n_top=100), plain)
    assert same(plain, expected(ba, 100))
    assert same(L.mdr_scan_top("gpu", Xs, ys == 1, 2, folds, 5, n_top=300), plain_s)
    assert same(plain_s, expected(bas, 300))
    hooks("reset")
    assert same(L.mdr_scan_top("gpu", X, y == 1, 3, n_top=100), plain)


def test_ranks_above_2_to_31(L):
    """The 2400-column construction of test_gpu_mdr.py: the last rank alone
    reaches BA 1.0.  The runners-up are checked against mdr_np on their own
    three combinations."""
    p, n = 2400, 256
    rng = np.random.default_rng(5)
    X = rng.integers(0, 3, size=(n, p)).astype(np.uint8)
    y = ((X[:, p - 3].astype(int) + X[:, p - 2] + X[:, p - 1]) % 2).astype(np.uint8)
    count = L.mdr_combinations(p, 3)
    top_ba, top_rank = L.mdr_scan_top("gpu", X, y == 1, 3, n_top=4)
    assert top_ba[0, 0] == np.float32(1.0) and top_rank[0, 0] == count - 1
    assert np.all(top_ba[0, 1:] < np.float32(1.0))
    for j in range(1, 3):  # BA descending, then rank ascending
        assert top_ba[0, j] > top_ba[0, j + 1] or (top_ba[0, j] == top_ba[0, j + 1]
                                                   and top_rank[0, j] < top_rank[0, j + 1])
    for j in range(1, 4):
        combo = L.mdr_unrank(p, 3, int(top_rank[0, j]))
        ba = mdr_np.all_bas(X[:, list(combo)], y == 1, 3)
        assert same_bits(ba, top_ba[0, j:j + 1])


def test_two_calls_return_the_same_arrays(L, noise):
    X, y, _ = noise
    assert same(L.mdr_scan_top("gpu", X, y == 1, 3, n_top=100),
                L.mdr_scan_top("gpu", X, y == 1, 3, n_top=100))
    Xs, ys, folds, _ = mdr_np.case(2049, 12, 2, 10)
    assert same(L.mdr_scan_top("gpu", Xs, ys == 1, 2, folds, 10, n_top=7),
                L.mdr_scan_top("gpu", Xs, ys == 1, 2, folds, 10, n_top=7))


def test_timing_reports_four_phases(L):
    X, y, fold, _ = mdr_np.case(203, 40, 2, 5)
    L.mdr_scan_top("gpu", X, y == 1, 2, fold, 5, n_top=7)
    assert all(t >= 0.0 for t in L.mdr_top_last_timing())


def test_genotype_above_two_is_rejected(L):
    X, y, _, _ = mdr_np.case(203, 14, 3, 3)
    X = X.copy()
    X[202, 13] = 3
    with pytest.raises(ValueError, match="0/1/2"):
        L.mdr_scan_top("gpu", X, y == 1, 2, n_top=3)


@pytest.mark.parametrize("n,p,k,cv,n_top", [(203, 40, 2, 5, 25), (203, 14, 3, 3, 7)])
def test_estimator_gpu_equals_cpu_and_numpy(L, n, p, k, cv, n_top):
    from fastselect_amd import MDR
    from mdr_top_np import FIT_ATTRS, TOP_ATTRS, check_estimator
    g = check_estimator("gpu", n, p, k, cv, n_top)
    X, y, _, _ = mdr_np.case(n, p, k, cv)
    c = MDR(k=k, cv=cv, backend="cpu").rank_interactions(X, y, n_top=n_top)
    assert g.effective_backend_ == "gpu" and c.effective_backend_ == "cpu"
    for name in FIT_ATTRS[:-1] + TOP_ATTRS:
        assert np.array_equal(getattr(g, name), getattr(c, name)), name
    assert np.array_equal(g.best_model_lookup_table_, c.best_model_lookup_table_)


def test_estimator_errors_on_gpu(L):
    from fastselect_amd import MDR
    X, y = mdr_np.planted(50, 6)
    with pytest.raises(ValueError, match="n_top"):
        MDR(k=2, cv=2, backend="gpu").rank_interactions(X, y, n_top=0)
    with pytest.raises(ValueError, match=str(L.MDR_MAX_TOP)):
        MDR(k=2, cv=2, backend="gpu").rank_interactions(X, y, n_top=L.MDR_MAX_TOP + 1)
