"""Selection-only mRMR on the CPU backend (fs_mrmr_cpu.cpp): fs_mrmr_select
must select what the numpy loop (mi_np.greedy) selects from the CPU backend's
own fs_mi_matrices output, and its relevance and rows must be that output's
entries bit for bit: both run the same table code and fs_mi.h expressions.
The tie rules of fs_mrmr.h are pinned through fs_mrmr_search_matrix on crafted
inputs that meet them at many steps."""
import numpy as np
import pytest

import mi_np
import mrmr_np

from fastselect_amd import _lib as L

_MATS = {}


def _cpu_matrices(key, make):
    """(X, y, S, rel, red) with the CPU backend's matrices, once per session."""
    if key not in _MATS:
        X, y, S = make()
        rel, red = L.mi_matrices("cpu", X, y, S)
        rel.setflags(write=False)
        red.setflags(write=False)
        _MATS[key] = (X, y, S, rel, red)
    return _MATS[key]


def _planted(n, p, states, seed):
    def make():
        X, y = mi_np.planted(n, p, states, seed)
        return X, y, int(max(X.max(), y.max())) + 1
    return make


# with the state counts 4 to 29 (mi_np.GEOMETRY) and n up to 4097 (mi_np.LONG)
DATA = {name: mi_np.ALL_SHAPES[name] for name in sorted(mi_np.ALL_SHAPES)}
DATA.update({"planted_%d_%d_%d_%d" % c: _planted(*c) for c in mi_np.PLANTED})


@pytest.mark.parametrize("method", mrmr_np.METHODS)
@pytest.mark.parametrize("name", sorted(DATA))
def test_data_path_equals_numpy_loop_on_cpu_matrix(name, method):
    X, y, S, rel, red = _cpu_matrices(name, DATA[name])
    p = X.shape[1]
    for k in mrmr_np.ks(p):
        sel, r, rows = L.mrmr_select("cpu", X, y, S, k, method=method)
        want, _ = mi_np.greedy(rel, red, k, method)
        assert np.array_equal(sel, want), k
        assert np.array_equal(r, rel)
        assert np.array_equal(rows, red[want]), k
        if k == p:   # every anchor was computed; one candidate was left at the end
            assert sorted(sel.tolist()) == list(range(p))
        sel2, r2, none = L.mrmr_select("cpu", X, y, S, k, method=method, want_rows=False)
        assert none is None and np.array_equal(sel2, sel) and np.array_equal(r2, r)


@pytest.mark.parametrize("method", mrmr_np.METHODS)
@pytest.mark.parametrize("p,k,seed", mrmr_np.TIE_CASES)
def test_tie_rules(p, k, seed, method):
    rel, red = mrmr_np.tie_inputs(p, seed)
    # what makes the case meaningful: steps where the mean redundancy decides
    # against both the lowest index and the highest score
    steps = mrmr_np.meaningful_tie_steps(rel, red, k, method)
    assert steps >= 5
    assert steps == mrmr_np.TIE_STEPS[(p, k, seed)][mrmr_np.METHODS.index(method)]
    assert int((rel == rel.max()).sum()) == mrmr_np.TIE_FIRST[(p, k, seed)]
    want, _ = mi_np.greedy(rel, red, k, method)
    assert np.array_equal(L.mrmr_search_matrix("cpu", rel, red, k, method=method), want)


@pytest.mark.parametrize("method", mrmr_np.METHODS)
def test_duplicated_columns(method):
    X, y, S, rel, red = _cpu_matrices("duplicated", mrmr_np.duplicated)
    assert mrmr_np.exact_tie_steps(rel, red, 20, method) == 2
    sel, r, rows = L.mrmr_select("cpu", X, y, S, 20, method=method)
    want, _ = mi_np.greedy(rel, red, 20, method)
    assert np.array_equal(sel, want)
    assert np.array_equal(r, rel) and np.array_equal(rows, red[want])


def test_nat_unit_rows():
    X, y, S, _, _ = _cpu_matrices("states5", mi_np.SHAPES["states5"])
    rel, red = L.mi_matrices("cpu", X, y, S, unit="nat")
    sel, r, rows = L.mrmr_select("cpu", X, y, S, 4, unit="nat")
    assert np.array_equal(r, rel) and np.array_equal(rows, red[sel])


@pytest.mark.parametrize("method", mrmr_np.METHODS)
@pytest.mark.parametrize("n,p,states,seed", mi_np.PLANTED)
def test_estimator_selected_equals_matrix(n, p, states, seed, method):
    from fastselect_amd import mRMR
    X, y = mi_np.planted(n, p, states, seed)
    a = mRMR(5, method=method, backend="cpu", redundancy="matrix").fit(X, y)
    b = mRMR(5, method=method, backend="cpu", redundancy="selected").fit(X, y)
    assert b.effective_backend_ == "cpu"
    assert b.top_features_.dtype == np.int32
    assert np.array_equal(a.top_features_, b.top_features_)
    assert np.array_equal(a.relevance_scores_, b.relevance_scores_)
    assert b.feature_importances_ is b.relevance_scores_
    assert b.redundancy_rows_.shape == (5, p)
    assert np.array_equal(b.redundancy_rows_, a.redundancy_matrix_[a.top_features_])
    assert not hasattr(b, "redundancy_matrix_") and not hasattr(a, "redundancy_rows_")
    assert np.array_equal(b.transform(X), X[:, a.top_features_])


def test_estimator_params():
    from sklearn.base import clone
    from fastselect_amd import mRMR
    est = mRMR(3, method="MIQ", redundancy="selected")
    assert est.get_params()["redundancy"] == "selected"
    assert clone(est).get_params() == est.get_params()
    assert mRMR(3).get_params()["redundancy"] == "matrix"
    assert mRMR(3).set_params(redundancy="selected").redundancy == "selected"
    with pytest.raises(ValueError, match="redundancy"):
        mRMR(3, redundancy="lazy")


def test_estimator_keeps_the_reference_checks():
    from fastselect_amd import mRMR
    X, y = mi_np.planted(64, 17, 2, 4)
    with pytest.raises(ValueError, match="integer"):
        mRMR(3, redundancy="selected").fit(X.astype(np.float64), y)
    with pytest.raises(ValueError, match="n_features_to_select"):
        mRMR(18, redundancy="selected").fit(X, y)
