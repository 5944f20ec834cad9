"""The 8-wave form of the sparse pass 2 (k_score_sparse3_w8): 256-feature
units at 64 VGPRs and a 64 KB row block, two workgroups per CU, for every
feature block whose real features are all continuous.

A feature's partial sums do not depend on the width of the unit that computes
them (same streams per wave, same terms, same order, same fold points), so the
``pass2_w8`` = 1 scores must equal the ``pass2_w8`` = 0 scores and those of the
plain-HIP walk (``pass2_generic`` = 1) bit for bit wherever the latter two are
bit-equal themselves; the dense pass 2 and the oracle bound the rest.  Sizes,
``seg_len`` and data as in test_gpu_pass2_segment.py.
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


def _data(n, p, seed, round_from=None, informative=10, redundant=20):
    key = (n, p, seed, round_from)
    if key not in _DATA:
        X, y = make_classification(n_samples=n, n_features=p, n_informative=informative,
                                   n_redundant=redundant, n_classes=2, random_state=seed)
        if round_from is not None:
            X[:, round_from:] = np.round(X[:, round_from:])
        _DATA[key] = (X, y)  # shared by the cases that use it; no test writes to it
    return _DATA[key]


def _fit(est_cls, X, y, **kw):
    est = est_cls(backend="gpu", n_features_to_select=1, **kw).fit(X, y)
    assert est.effective_backend_ == "gpu"
    return est.feature_importances_


def _four_ways(hooks, seg_len, run):
    """run() on the 8-wave kernel, on the 4-wave kernels, on the plain-HIP walk
    and on the dense pass 2."""
    hooks("sparse", 1)
    hooks("seg_len", seg_len)
    hooks("pass2_w8", 1)
    w8 = run()
    hooks("pass2_w8", 0)
    w4 = run()
    hooks("pass2_generic", 1)
    gen = run()
    hooks("pass2_generic", 0)
    hooks("sparse", 0)
    dense = run()
    return w8, w4, gen, dense


# n, p, seg_len, first rounded column, bit equality, oracle
MULTISURF_CASES = [
    # two full 256-feature blocks and an 8-feature partial block (lanes past
    # PW, slack reads); segments of 4, 3, 2 and 1 tiles
    pytest.param(700, 520, 4, None, True, True, id="n700-p520-seg4"),
    # one full block; one-tile segments: only the "after the last tile" path
    pytest.param(257, 256, 1, None, True, True, id="n257-p256-seg1"),
    # continuous blocks on the 8-wave kernel beside mixed blocks on the 4-wave one
    pytest.param(700, 600, 3, 500, False, True, id="n700-p600-mixed-seg3"),
    # row blocks of more than 64 tiles: the 64-tile cap and the chunk loop
    pytest.param(8400, 300, 100, None, True, False, id="n8400-p300-seg100"),
]


@pytest.mark.parametrize("n,p,seg_len,round_from,bits,with_oracle", MULTISURF_CASES)
def test_multisurf_w8(oracle, hooks, n, p, seg_len, round_from, bits, with_oracle):
    from fastselect_amd import MultiSURF
    X, y = _data(n, p, n + p, round_from)
    w8, w4, gen, dense = _four_ways(hooks, seg_len, lambda: _fit(MultiSURF, X, y))
    print(f"vs 4-wave {scale_rel_err(w8, w4):.3e}, vs plain-HIP walk {scale_rel_err(w8, gen):.3e}, "
          f"vs dense {scale_rel_err(w8, dense):.3e}")
    assert np.all(np.isfinite(w8))
    if bits:
        assert np.array_equal(w8, w4)
        assert np.array_equal(w8, gen)
    assert scale_rel_err(w8, dense) <= DENSE_TOL
    if with_oracle:
        ref = oracle.multisurf_scores(X, y)
        print(f"vs oracle {scale_rel_err(w8, ref):.3e}")
        assert np.all(np.isfinite(ref))
        assert_parity(w8, ref, TOL, k=10)


@pytest.mark.parametrize("star", [False, True])
def test_surf_w8(hooks, star):
    """SURF / SURF* above SURF's 4096-sample sparse limit (the split's near
    pairs for SURF*): many all-zero rows in a wave's blocks; one partial
    256-feature block."""
    import warnings
    from fastselect_amd import SURF
    X, y = _data(4200, 128, 21, informative=12)

    def run():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            return _fit(SURF, X, y, use_star=star)

    hooks("seg_len", 4)
    hooks("pass2_w8", 1)
    w8 = run()
    hooks("pass2_w8", 0)
    w4 = run()
    assert np.all(np.isfinite(w8))
    assert np.array_equal(w8, w4)


def test_two_steps_are_bit_identical(hooks):
    """The statement leaves no state behind: two steps of one plan on the
    8-wave kernel give the same bits, and they are the 4-wave kernels'."""
    from fastselect_amd.parallel import ShardedMultiSURF
    X, y = _data(700, 520, 7)
    hooks("sparse", 1)
    hooks("seg_len", 4)
    X32 = X.astype(np.float32)
    recip = (1 / (X32.max(0) - X32.min(0))).astype(np.float32)
    out = {}
    for w8 in (1, 0):
        hooks("pass2_w8", w8)
        job = ShardedMultiSURF(X32, y, recip, np.zeros(X32.shape[1], bool), use_star=False,
                               backend="gpu", device=0)
        try:
            a = job.step().cpu().numpy().copy()
            b = job.step().cpu().numpy().copy()
            assert job.weighted_pairs() > 0
        finally:
            job.close()
        np.testing.assert_array_equal(a, b)
        out[w8] = a
    np.testing.assert_array_equal(out[1], out[0])
