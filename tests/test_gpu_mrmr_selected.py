"""Selection-only mRMR on the GPU (fs_mrmr.hip).  Every relevance and row
entry must equal the GPU fs_mi_matrices entry bit for bit (k_mi_row runs
pt_epilogue of fs_pairtab.h, k_mi_scan the same steps in fs_mi.hip) and lie within
the suite's 1e-10 of the CPU backend's (derived in test_mi.py); the selection must be what
the numpy loop selects from the GPU matrix, and two calls must give identical
bits.  Shapes are the smallest at which the kernels can go wrong.  The row
kernel takes 256 / NB^2 columns per workgroup (NB = ceil(states / 4)), y is one
more column, it stages 64 words (2048 samples) per chunk, and the step kernels
use 256 lanes:

* 3 states: p = 255 (y is the last lane of the only workgroup), 256 (y alone
  in a second workgroup), 257;
* 5 states (64 columns per workgroup): p = 63, 64, 130;
* 10 states: p = 29 (28 pairs per workgroup, 4 idle lanes); 32 states: p = 9;
* mixed columns: per-column state counts; y with 4 classes beside 3 states;
* n = 33 / 64 / 203 / 2049: over a word boundary, whole words, a ragged word,
  and one restaging of LDS;
* 4, 8, 12, 13, 16, 17, 20, 21, 24, 25, 28 and 29 states at n = 97 and 257
  with a 4-class y (mi_np.GEOMETRY): both ends of every NB = ceil(states / 4),
  so 16-, 25-, 36- and 49-lane pairs, T = 4, 3, 2 and 10, 7, 5 columns per
  workgroup with idle lanes, and state counts with no padding plane; per state
  count p = CPW - 1, CPW, CPW + 1 and 2T + 1; mixed columns with the state
  bound at 21 and at 25;
* n = 2048, 4096 and 4097 (mi_np.LONG): whole staging chunks and two restages."""
import numpy as np
import pytest

import mi_np
import mrmr_np

pytestmark = pytest.mark.gpu

TOL = 1e-10


@pytest.fixture(scope="module")
def L():
    from fastselect_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    return _lib


def _u(n, p, states, seed):
    return lambda: mi_np.uniform(n, p, states, seed) + (states,)


SHAPES = {
    "s3_p255": _u(65, 255, 3, 61),
    "s3_p256": _u(65, 256, 3, 62),
    "s3_p257": _u(65, 257, 3, 63),
    "s5_p63": _u(65, 63, 5, 64),
    "s5_p64": _u(65, 64, 5, 65),
    "s5_p130": _u(65, 130, 5, 66),
    "s10_p29": _u(150, 29, 10, 67),
    "s32_p9": _u(257, 9, 32, 68),
    "mixed": mi_np.SHAPES["mixed"],
    "y4": mi_np.SHAPES["y4"],
    "n33": mi_np.SHAPES["n33"],
    "n64": mi_np.SHAPES["n64"],
    "n203": mi_np.SHAPES["n203"],
    "n2049": mi_np.SHAPES["restage"],
}
SHAPES.update(mi_np.GEOMETRY)
SHAPES.update(mi_np.LONG)

_MATS = {}


def _gpu_matrices(L, key, make):
    """(X, y, S, rel, red) with the GPU backend's matrices, once per session."""
    if key not in _MATS:
        X, y, S = make()
        rel, red = L.mi_matrices("gpu", X, y, S)
        rel.setflags(write=False)
        red.setflags(write=False)
        _MATS[key] = (X, y, S, rel, red)
    return _MATS[key]


def _check_data_path(L, X, y, S, rel, red, k):
    for method in mrmr_np.METHODS:
        sel, r, rows = L.mrmr_select("gpu", X, y, S, k, method=method)
        want, _ = mi_np.greedy(rel, red, k, method)
        assert np.array_equal(r, rel)
        assert np.array_equal(sel, want), method
        assert np.array_equal(rows, red[want]), method
        sel2, r2, rows2 = L.mrmr_select("gpu", X, y, S, k, method=method)
        assert np.array_equal(sel2, sel) and np.array_equal(r2, r) and np.array_equal(rows2, rows)
        sel3, r3, none = L.mrmr_select("gpu", X, y, S, k, method=method, want_rows=False)
        assert none is None and np.array_equal(sel3, sel) and np.array_equal(r3, r)
    # the CPU backend's values of the same rows (the last method's selection)
    cr, cR = L.mi_matrices("cpu", X, y, S)
    print("gpu-cpu", max(np.abs(r - cr).max(), np.abs(rows - cR[sel]).max()))
    assert np.abs(r - cr).max() <= TOL and np.abs(rows - cR[sel]).max() <= TOL


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_rows_equal_matrix_and_selection_equals_numpy(L, name):
    X, y, S, rel, red = _gpu_matrices(L, name, SHAPES[name])
    p = X.shape[1]
    _check_data_path(L, X, y, S, rel, red, p if p <= 130 else 24)


@pytest.mark.parametrize("method", mrmr_np.METHODS)
@pytest.mark.parametrize("p,k,seed", mrmr_np.TIE_CASES)
def test_tie_rules(L, p, k, seed, method):
    rel, red = mrmr_np.tie_inputs(p, seed)
    assert mrmr_np.meaningful_tie_steps(rel, red, k, method) >= 5
    want, _ = mi_np.greedy(rel, red, k, method)
    got = L.mrmr_search_matrix("gpu", rel, red, k, method=method)
    assert np.array_equal(got, want)
    assert np.array_equal(L.mrmr_search_matrix("gpu", rel, red, k, method=method), got)


def test_duplicated_columns(L):
    X, y, S, rel, red = _gpu_matrices(L, "duplicated", mrmr_np.duplicated)
    _check_data_path(L, X, y, S, rel, red, 20)


@pytest.mark.parametrize("method", mrmr_np.METHODS)
@pytest.mark.parametrize("n,p,states,seed", mi_np.PLANTED)
def test_estimator_selected_equals_matrix_and_cpu(L, n, p, states, seed, method):
    from fastselect_amd import mRMR
    X, y = mi_np.planted(n, p, states, seed)
    # the restatement's own scores keep every greedy step far from a tie
    S = int(max(X.max(), y.max())) + 1
    _, _, _, rel, red, _ = mi_np.case(("planted", n, p, states, seed), lambda: (X, y, S))
    want, margins = mi_np.greedy(rel, red, 5, method)
    assert margins.min() >= mi_np.PLANT_MARGIN
    g = mRMR(5, method=method, backend="gpu", redundancy="selected").fit(X, y)
    m = mRMR(5, method=method, backend="gpu", redundancy="matrix").fit(X, y)
    c = mRMR(5, method=method, backend="cpu", redundancy="selected").fit(X, y)
    assert g.effective_backend_ == "gpu" and c.effective_backend_ == "cpu"
    assert g.top_features_.dtype == np.int32 and not hasattr(g, "redundancy_matrix_")
    assert np.array_equal(g.top_features_, m.top_features_)
    assert np.array_equal(g.top_features_, c.top_features_)
    assert np.array_equal(g.top_features_, want)
    assert np.array_equal(g.relevance_scores_, m.relevance_scores_)
    assert np.array_equal(g.redundancy_rows_, m.redundancy_matrix_[m.top_features_])
    assert np.abs(g.redundancy_rows_ - c.redundancy_rows_).max() <= TOL
    assert np.abs(g.relevance_scores_ - c.relevance_scores_).max() <= TOL
    auto = mRMR(5, method=method, backend="auto", redundancy="selected").fit(X, y)
    assert auto.effective_backend_ == "gpu"
    assert np.array_equal(auto.top_features_, g.top_features_)


def test_width_100000(L):
    """p = 100000: the matrix mode would need 80 GB; the selected mode holds
    the planes, 5 rows and a few vectors."""
    from fastselect_amd import mRMR
    n, p = 64, 100000
    X, y = mi_np.planted(n, p, 3, 1)
    g = mRMR(5, redundancy="selected", backend="gpu").fit(X, y)
    timing = L.mrmr_last_timing()
    c = mRMR(5, redundancy="selected", backend="cpu").fit(X, y)
    assert sorted(c.top_features_.tolist()) == sorted([1, p // 2, p - 1, p // 3, 2 * p // 3])
    assert np.array_equal(g.top_features_, c.top_features_)
    assert g.redundancy_rows_.shape == (5, p)
    assert np.abs(g.redundancy_rows_ - c.redundancy_rows_).max() <= TOL
    assert np.abs(g.relevance_scores_ - c.relevance_scores_).max() <= TOL
    assert len(timing) == 5 and all(t >= 0.0 for t in timing)


def test_many_steps_are_timed_as_a_whole(L):
    """Above 64 steps the loop is timed by two events: rows holds it, steps
    is unavailable."""
    X, y, S, rel, red = _gpu_matrices(L, "s5_p130", SHAPES["s5_p130"])
    L.mrmr_select("gpu", X, y, S, 130)
    up, pack, relv, rows, steps = L.mrmr_last_timing()
    assert min(up, pack, relv, rows) >= 0.0 and steps == -1.0


def test_rejections(L):
    X, y = mi_np.uniform(64, 5, 3, 42)
    X = X.copy()
    X[63, 4] = 3
    with pytest.raises(ValueError, match=">= n_states"):
        L.mrmr_select("gpu", X, y, 3, 2)
    X[63, 4] = 0
    y = y.copy()
    y[10] = 3
    with pytest.raises(ValueError, match=">= n_states"):
        L.mrmr_select("gpu", X, y, 3, 2)
    # a code beyond the padded state count, too
    X[5, 1] = 200
    with pytest.raises(ValueError, match=">= n_states"):
        L.mrmr_select("gpu", X, np.zeros(64, np.uint8), 3, 5)
    X33, y33 = mi_np.uniform(90, 3, 33, 33)
    with pytest.raises(ValueError, match="32 states"):
        L.mrmr_select("gpu", X33, y33, 33, 2)
    # the device still answers
    Xo, yo = mi_np.uniform(64, 5, 3, 42)
    sel, _, _ = L.mrmr_select("gpu", Xo, yo, 3, 5)
    assert sorted(sel.tolist()) == [0, 1, 2, 3, 4]
