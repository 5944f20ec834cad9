"""The segment walk of the sparse pass 2 (k_score_sparse3, continuous feature
blocks): one generated statement walks all tiles of a (unit, segment), the
tile loop, the fold into the f64 sums and the progress counter inside it.

At test sizes the plan computes one-tile segments, so every case sets the
``seg_len`` test hook (and forces the sparse pass 2).  Comparisons:
 (a) against the plain-HIP walk of every unit (``pass2_generic`` hook: the
     same terms in the same order with the same fold points) -- bit for bit;
 (b) against the dense pass 2 of the same data, <= 1e-6 scale-relative;
 (c) against the oracle, scale-relative 1e-5 and identical top-k.
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


_DATA = {}


def _data(n, p, seed, round_from=None):
    key = (n, p, seed, round_from)
    if key not in _DATA:
        X, y = make_classification(n_samples=n, n_features=p, n_informative=10, n_redundant=20,
                                   n_classes=2, random_state=seed)
        if round_from is not None:
            X[:, round_from:] = np.round(X[:, round_from:])
        _DATA[key] = (X, y)  # shared by the cases that use it; no test writes to it
    return _DATA[key]


def _fit(est_cls, X, y, **kw):
    est = est_cls(backend="gpu", n_features_to_select=1, **kw).fit(X, y)
    assert est.effective_backend_ == "gpu"
    return est.feature_importances_


def _three_ways(hooks, seg_len, run):
    """run() under the segment walk, the plain-HIP walk and the dense pass 2."""
    hooks("sparse", 1)
    hooks("seg_len", seg_len)
    seg = run()
    hooks("pass2_generic", 1)
    gen = run()
    hooks("pass2_generic", 0)
    hooks("sparse", 0)
    dense = run()
    return seg, gen, dense


# n, p, seg_len, first rounded column, bit equality with the plain-HIP walk, oracle
MULTISURF_CASES = [
    # six row blocks, segments of 4, 3, 2 and 1 tiles; one F = 8 block and the F = 4 tail
    pytest.param(700, 520, 4, None, True, True, id="n700-p520-seg4"),
    # a partial F = 8 block: lanes past PW, slack reads
    pytest.param(700, 800, 6, None, True, True, id="n700-p800-seg6"),
    # mixed blocks on the C++ loop beside continuous blocks on the statement
    pytest.param(700, 600, 3, 500, False, True, id="n700-p600-mixed-seg3"),
    # one-tile segments: the "after the last tile" path is the only path
    pytest.param(257, 520, 1, None, True, True, id="n257-p520-seg1"),
    # row blocks of more than 64 tiles: the 64-tile cap and the chunk boundary
    pytest.param(8400, 300, 100, None, True, False, id="n8400-p300-seg100"),
]


@pytest.mark.parametrize("n,p,seg_len,round_from,bits,with_oracle", MULTISURF_CASES)
def test_multisurf_segment_walk(oracle, hooks, n, p, seg_len, round_from, bits, with_oracle):
    from fastselect_amd import MultiSURF
    X, y = _data(n, p, n + p, round_from)
    seg, gen, dense = _three_ways(hooks, seg_len, lambda: _fit(MultiSURF, X, y))
    print(f"vs plain-HIP walk {scale_rel_err(seg, gen):.3e}, vs dense {scale_rel_err(seg, dense):.3e}")
    assert np.all(np.isfinite(seg))
    if bits:
        assert np.array_equal(seg, gen)
    assert scale_rel_err(seg, dense) <= DENSE_TOL
    if with_oracle:
        ref = oracle.multisurf_scores(X, y)
        print(f"vs oracle {scale_rel_err(seg, ref):.3e}")
        assert np.all(np.isfinite(ref))
        assert_parity(seg, ref, TOL, k=10)


@pytest.mark.parametrize("star", [False, True])
def test_surf_segment_walk(hooks, star):
    """SURF / SURF*: only near pairs are weighed, so a wave's blocks hold many
    all-zero rows."""
    from fastselect_amd import SURF
    X, y = _data(700, 520, 3)
    seg, gen, dense = _three_ways(hooks, 4, lambda: _fit(SURF, X, y, use_star=star))
    print(f"vs plain-HIP walk {scale_rel_err(seg, gen):.3e}, vs dense {scale_rel_err(seg, dense):.3e}")
    assert np.array_equal(seg, gen)
    assert scale_rel_err(seg, dense) <= DENSE_TOL


def _surf_rows_sums(X, y, rows):
    import torch
    from fastselect_amd import _lib
    from fastselect_amd.SURF import surf_inputs
    isd, recip = surf_inputs(X, 10, "gpu")
    plan = _lib.RowsPlan("gpu", "surf", np.ascontiguousarray(X), y.astype(np.int32), recip, isd,
                         use_star=False, rows=rows)
    try:
        sums = torch.zeros(X.shape[1], dtype=torch.float64, device="cuda")
        plan.score(sums.data_ptr())
        torch.cuda.synchronize()
        return sums.cpu().numpy()
    finally:
        plan.close()


def test_surf_row_shard_segment_walk(hooks):
    """A row-sharded SURF plan (focal rows 64..499 of 700): only the focal side
    of a pair is weighed, so whole wave blocks are zero."""
    X, y = _data(700, 520, 5)
    seg, gen, dense = _three_ways(hooks, 4, lambda: _surf_rows_sums(X, y, (64, 500)))
    scale = np.abs(dense).max()
    print(f"vs plain-HIP walk {np.abs(seg - gen).max() / scale:.3e}, vs dense {np.abs(seg - dense).max() / scale:.3e}")
    assert np.array_equal(seg, gen)
    assert np.abs(seg - dense).max() <= DENSE_TOL * scale


def test_two_steps_are_bit_identical(hooks):
    """Every weight slot is rewritten on every step, the walk's order is fixed
    and the statement leaves no state behind: two steps of one plan give the
    same bits."""
    from fastselect_amd.parallel import ShardedMultiSURF
    X, y = _data(700, 520, 7)
    hooks("sparse", 1)
    hooks("seg_len", 4)
    X32 = X.astype(np.float32)
    recip = (1 / (X32.max(0) - X32.min(0))).astype(np.float32)
    job = ShardedMultiSURF(X32, y, recip, np.zeros(X32.shape[1], bool), use_star=False,
                           backend="gpu", device=0)
    try:
        a = job.step().cpu().numpy().copy()
        b = job.step().cpu().numpy().copy()
        assert job.weighted_pairs() > 0
    finally:
        job.close()
    np.testing.assert_array_equal(a, b)
