"""The row-major sparse pass 2 (k_weights_sparse3 + k_score_sparse3): a dense
weight block per (tile, half, wave), walked row by row with one LDS row read
shared by the wave's 8 columns.

Every case forces the sparse pass 2 (the ``sparse`` test hook) on shapes small
enough to take seconds and compares it with the oracle (scale-relative 1e-5,
identical top-k) and with the dense pass 2 (k_weights + k_score) of the same
data (<= 1e-6: same terms, another float32 summation order inside a tile).
"""
import numpy as np
import pytest
from conftest import assert_parity, scale_rel_err
from sklearn.datasets import make_classification

pytestmark = pytest.mark.gpu

TOL = 1e-5
DENSE_TOL = 1e-6


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    from fastselect_amd import _lib
    assert _lib.device_count() >= 1, "no HIP device visible: GPU tests cannot run"


def _data(n, p, ncls=2, seed=0, round_from=None):
    ninf = max(2, min(10, p // 2))
    X, y = make_classification(n_samples=n, n_features=p, n_informative=ninf,
                               n_redundant=min(20, p // 4), n_classes=ncls,
                               random_state=seed)
    if round_from is not None:
        X[:, round_from:] = np.round(X[:, round_from:])
    return X, y


def _fit(est_cls, X, y, **kw):
    est = est_cls(backend="gpu", n_features_to_select=1, **kw).fit(X, y)
    assert est.effective_backend_ == "gpu"
    return est.feature_importances_


def _sparse_and_dense(hooks, est_cls, X, y, **kw):
    out = {}
    for mode in (0, 1):
        hooks("sparse", mode)
        out[mode] = _fit(est_cls, X, y, **kw)
    return out[1], out[0]


# n, p, classes, first rounded column (None: all continuous)
MULTISURF_CASES = [
    # one diagonal tile; half 1 holds a single real row; one F = 4 block, mostly padding lanes
    pytest.param(65, 8, 2, None, id="n65-p8"),
    # a second row block with 2 rows; a tile half whose wave blocks are all zero
    pytest.param(130, 64, 2, None, id="n130-p64"),
    pytest.param(200, 70, 3, None, id="n200-p70-3cls"),
    # one F = 8 block plus the F = 4 tail
    pytest.param(257, 520, 2, None, id="n257-p520"),
    # a partial F = 8 block
    pytest.param(192, 800, 2, None, id="n192-p800"),
    # a block mixing continuous and discrete features: the plain-HIP walk beside the generated one
    pytest.param(257, 600, 2, 500, id="n257-p600-mixed"),
    # all-discrete blocks
    pytest.param(140, 520, 2, 0, id="n140-p520-discrete"),
]


@pytest.mark.parametrize("n,p,ncls,round_from", MULTISURF_CASES)
def test_multisurf_rows_walk(oracle, hooks, n, p, ncls, round_from):
    from fastselect_amd import MultiSURF
    X, y = _data(n, p, ncls, seed=n + p, round_from=round_from)
    sparse, dense = _sparse_and_dense(hooks, MultiSURF, X, y)
    ref = oracle.multisurf_scores(X, y)
    print(f"vs dense {scale_rel_err(sparse, dense):.3e}, vs oracle {scale_rel_err(sparse, ref):.3e}")
    assert np.all(np.isfinite(ref))
    assert scale_rel_err(sparse, dense) <= DENSE_TOL
    assert_parity(sparse, ref, TOL, k=min(10, p))


@pytest.mark.parametrize("star", [False, True])
def test_surf_rows_walk(oracle, hooks, star):
    from fastselect_amd import SURF
    X, y = _data(257, 520, seed=3)
    sparse, dense = _sparse_and_dense(hooks, SURF, X, y, use_star=star)
    ref = oracle.surf_scores(X, y, use_star=star)
    print(f"vs dense {scale_rel_err(sparse, dense):.3e}, vs oracle {scale_rel_err(sparse, ref):.3e}")
    assert scale_rel_err(sparse, dense) <= DENSE_TOL
    assert_parity(sparse, ref, TOL, k=10)


def _surf_rows_sums(X, y, rows, star=False):
    import torch
    from fastselect_amd import _lib
    from fastselect_amd.SURF import surf_inputs
    isd, recip = surf_inputs(X, 10, "gpu")
    plan = _lib.RowsPlan("gpu", "surf", np.ascontiguousarray(X), y.astype(np.int32), recip, isd,
                         use_star=star, rows=rows)
    try:
        sums = torch.zeros(X.shape[1], dtype=torch.float64, device="cuda")
        plan.score(sums.data_ptr())
        torch.cuda.synchronize()
        return sums.cpu().numpy(), plan.weighted_pairs()
    finally:
        plan.close()


def test_surf_row_shard(hooks):
    """A row-sharded SURF plan (focal rows 64..199 of 257): only the focal
    side of a pair is weighed, so the density is low and many rows of a
    wave's block hold 8 zero weights.  The shard's sums are those of the dense
    pass 2 on the same rows, and the three shards of the sample range add up
    to the unsharded plan's sums."""
    X, y = _data(257, 520, seed=5)
    hooks("sparse", 1)
    mid, nz = _surf_rows_sums(X, y, (64, 200))
    assert nz > 0
    parts = mid + _surf_rows_sums(X, y, (0, 64))[0] + _surf_rows_sums(X, y, (200, 257))[0]
    whole, nz_whole = _surf_rows_sums(X, y, None)
    assert 0 < nz < nz_whole
    hooks("sparse", 0)
    mid_dense, _ = _surf_rows_sums(X, y, (64, 200))
    whole_dense, _ = _surf_rows_sums(X, y, None)
    scale = np.abs(whole_dense).max()
    print(f"shard vs dense {np.abs(mid - mid_dense).max() / scale:.3e}, "
          f"shards vs whole {np.abs(parts - whole).max() / scale:.3e}")
    assert np.abs(mid - mid_dense).max() <= DENSE_TOL * scale
    assert np.abs(whole - whole_dense).max() <= DENSE_TOL * scale
    assert np.abs(parts - whole).max() <= DENSE_TOL * scale


def _multisurf_job(X, y):
    from fastselect_amd.parallel import ShardedMultiSURF
    X = X.astype(np.float32)
    recip = (1 / (X.max(0) - X.min(0))).astype(np.float32)
    return ShardedMultiSURF(X, y, recip, np.zeros(X.shape[1], bool), use_star=False,
                            backend="gpu", device=0), X, recip


def test_two_steps_are_bit_identical(hooks):
    """Every weight slot is rewritten on every step and the walk's order is
    fixed: two steps of one plan give the same bits."""
    X, y = _data(257, 520, seed=7)
    hooks("sparse", 1)
    job, _, _ = _multisurf_job(X, y)
    try:
        a = job.step().cpu().numpy().copy()
        b = job.step().cpu().numpy().copy()
        assert job.weighted_pairs() > 0
    finally:
        job.close()
    np.testing.assert_array_equal(a, b)


def test_weighted_pairs_count(hooks):
    """fs_plan_weighted_pairs counts the non-zero slots of the dense blocks
    exactly (a numpy restatement of the near decisions, as
    test_sparse_weighted_pairs_count)."""
    X, y = _data(257, 300, seed=9)
    hooks("sparse", 1)
    job, X32, recip = _multisurf_job(X, y)
    try:
        job.step()
        nz = job.weighted_pairs()
    finally:
        job.close()
    Xs = (X32 - X32.min(0)) * recip
    D = np.abs(Xs[:, None, :].astype(np.float64) - Xs[None, :, :]).sum(-1)
    n = len(X32)
    off = ~np.eye(n, dtype=bool)
    mu = D.sum(1) / (n - 1)
    sd = np.sqrt(np.maximum((D ** 2).sum(1) / (n - 1) - mu ** 2, 0))
    near = (D < (mu - sd / 2)[:, None]) & off
    want = int(np.triu(near | near.T, 1).sum())
    assert 0.2 * n * (n - 1) / 2 < nz < 0.7 * n * (n - 1) / 2
    assert abs(nz - want) <= max(3, want // 2000)
    # on grid data with the caller's thresholds (tests/pass2_np.py) no decision
    # is in doubt: the count is the predicted one exactly
    import pass2_np as R
    from fastselect_amd import _lib
    Xg, yg, isd, recip_g = R.grid_data(257, 300, 0, seed=9)
    ng = len(Xg)
    D = R.distances(Xg, isd)
    H, M = R.counts_pow2(ng)
    thr = R.patterns(D, ng)["q40"]
    e = R.expected(Xg, yg, isd, thr, H, M, False, D=D)
    R.check_exactness(Xg, isd, D, thr, H, M, e["W32"])
    plan = _lib.Plan("gpu", Xg, yg.astype(np.float64), recip_g, isd)
    try:
        bufs = R.DevBufs(*Xg.shape)
        plan.pass1(bufs.ptr("rs"))
        bufs.sync()
        R.select_and_score(plan, bufs, thr, R.pack_counts(H, M), plan.calibration()["SC"])
        nz_grid = plan.weighted_pairs()
    finally:
        plan.close()
    assert 0.2 * ng * (ng - 1) / 2 < e["weighted"] < 0.8 * ng * (ng - 1) / 2
    assert nz_grid == e["weighted"]
