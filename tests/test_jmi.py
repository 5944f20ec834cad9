"""JMI / CMIM on the CPU backend (fs_jmi_cpu.cpp, fastselect_amd/JMI.py)
against the numpy restatement (jmi_np.py).

Identities that hold without a tolerance (array_equal): a row of joint
relevance equals the CPU fs_mi_matrices relevance of the synthetic joint
columns x_lo * S + x_hi (both run mi_from_table over the same integer table up
to rows of zeros); fs_jmi_select's rows equal fs_jmi_rows at the selected
anchors and its relevance equals fs_mrmr_select's; the selection equals the
restatement's greedy loop on the backend's own rows.

Tolerance against the restatement.  tests/test_mi.py derives the suite's 1e-10
for a sum of at most S^2 = 1024 terms.  A joint table has S^2 * C cells, at most
4096 with the GPU limits, of which at most min(S^2 * C, n) are non-zero.  With
u = 1.1e-16 and sum(pxy * |log r|) <= log n <= 21.5 nats for n < 2^31: each
term carries about 5 u of relative error (division, product, sum, a <= 1 ulp
log, product), 1.2e-14 in the sum; the marginals are sums of at most S^2 terms,
relative error 1024 u = 1.1e-13, which moves every log by as much and the sum
by at most 1.1e-13; the T - 1 additions of the terms add at most T * 21.5 u =
1.0e-11 at T = 4096.  Together below 1.1e-11 nats = 1.5e-11 bits, so the
tolerance stays 1e-10: it leaves about 7x over the bound at the limits, and on
the shapes used here (at most 257 non-zero terms) more than 100x, while a
wrong count moves a value by about 1/n >= 5e-4.  The restatement's stated
deviation (about -1e-12 per non-zero cell of a table with a single row or a
single class) stays inside it for the shapes used: at most 25 such cells.

The shapes are mi_np.ALL_SHAPES, the state counts 4 to 29 of mi_np.GEOMETRY
(4 classes of y) and the long sample axes of mi_np.LONG included.
"""
import numpy as np
import pytest

import jmi_np
import mdr_np
import mi_np

from fastselect_amd import _lib as L

TOL = 1e-10

_CASES = {}


def _case(name):
    """(X, y, S, C, anchors, rows of the CPU backend at every column), once per
    session."""
    if name not in _CASES:
        X, y, S = mi_np.ALL_SHAPES[name]()
        X = np.ascontiguousarray(X, dtype=np.uint8)
        y = np.ascontiguousarray(y, dtype=np.uint8)
        p = X.shape[1]
        allrows = L.jmi_rows("cpu", X, y, S, np.arange(p))
        allrows.setflags(write=False)
        _CASES[name] = (X, y, S, int(y.max()) + 1, [0, p // 2, p - 1], allrows)
    return _CASES[name]


@pytest.mark.parametrize("name", sorted(mi_np.ALL_SHAPES))
def test_rows_equal_restatement(name):
    X, y, S, C, anchors, allrows = _case(name)
    want = jmi_np.rows(X, y, anchors, S, C)
    got = L.jmi_rows("cpu", X, y, S, anchors)
    assert np.abs(got - want).max() <= TOL
    assert np.array_equal(got, allrows[anchors])          # whatever the anchors' company
    assert all(got[t, a] == 0.0 for t, a in enumerate(anchors))
    assert np.array_equal(allrows, allrows.T)             # J(f, s) is one pair's value
    # the thread count changes no bit
    assert np.array_equal(L.jmi_rows("cpu", X, y, S, anchors, n_jobs=1), got)


# the synthetic columns need S^2 <= 256 states: every shape up to 16 states
@pytest.mark.parametrize("name", sorted(n for n, make in mi_np.ALL_SHAPES.items()
                                        if make()[2] ** 2 <= 256))
def test_rows_equal_relevance_of_synthetic_columns(name):
    X, y, S, C, anchors, allrows = _case(name)
    assert S * S <= 256
    for a in anchors:
        Z = jmi_np.synthetic(X, a, S)
        rel, _ = L.mi_matrices("cpu", Z, y, int(max(Z.max(), y.max())) + 1)
        keep = np.arange(X.shape[1]) != a
        assert np.array_equal(allrows[a][keep], rel[keep])


def test_nat_unit():
    X, y, S, C, anchors, allrows = _case("states5")
    nat = L.jmi_rows("cpu", X, y, S, anchors, unit="nat")
    assert np.abs(nat - jmi_np.rows(X, y, anchors, S, C, unit="nat")).max() <= TOL
    Z = jmi_np.synthetic(X, anchors[1], S)
    rel, _ = L.mi_matrices("cpu", Z, y, int(Z.max()) + 1, unit="nat")
    keep = np.arange(X.shape[1]) != anchors[1]
    assert np.array_equal(nat[1][keep], rel[keep])


@pytest.mark.parametrize("method", jmi_np.METHODS)
@pytest.mark.parametrize("name", sorted(mi_np.ALL_SHAPES))
def test_select_equals_greedy_on_own_rows(name, method):
    X, y, S, C, anchors, allrows = _case(name)
    p = X.shape[1]
    _, mrel, _ = L.mrmr_select("cpu", X, y, S, 1, want_rows=False)
    for k in sorted({1, max(1, p // 2), p}):
        sel, rel, rows = L.jmi_select("cpu", X, y, S, k, method=method)
        assert np.array_equal(rel, mrel)
        assert np.array_equal(rows, allrows[sel])
        want, _ = jmi_np.greedy(rel, lambda s: allrows[s], k, method)
        assert np.array_equal(sel, want), k
        if k == p:
            assert sorted(sel.tolist()) == list(range(p))
        sel2, rel2, rows2 = L.jmi_select("cpu", X, y, S, k, method=method)
        assert np.array_equal(sel2, sel) and np.array_equal(rel2, rel)
        assert np.array_equal(rows2, rows)
        sel3, rel3, none = L.jmi_select("cpu", X, y, S, k, method=method, want_rows=False)
        assert none is None and np.array_equal(sel3, sel) and np.array_equal(rel3, rel)


@pytest.mark.parametrize("method", jmi_np.METHODS)
@pytest.mark.parametrize("p,k,seed", jmi_np.TIE_CASES)
def test_tie_and_min_rules(p, k, seed, method):
    rel, joint = jmi_np.tie_inputs(p, seed)
    # what makes the case meaningful: exact ties that the index decides, at
    # step 0 and later, and a minimum that different selected features attain
    assert int((rel == rel.max()).sum()) > 1
    assert jmi_np.exact_tie_steps(rel, joint, k, method) >= 5
    want, _ = jmi_np.greedy(rel, lambda s: joint[s], k, method)
    if method == "CMIM":
        assert jmi_np.cmim_argmin_spread(rel, joint, want) >= 3
    got = L.jmi_search_matrix("cpu", rel, joint, k, method=method)
    assert np.array_equal(got, want)


def test_lowest_index_wins_everywhere():
    """All scores equal at every step: the selection is 0, 1, 2, ..."""
    p = 9
    rel = np.full(p, 0.25)
    joint = np.full((p, p), 0.5) - 0.5 * np.eye(p)
    for method in jmi_np.METHODS:
        assert L.jmi_search_matrix("cpu", rel, joint, p, method=method).tolist() == list(range(p))


def test_cmim_takes_the_minimum_not_the_sum():
    """Candidate 1 has the larger sum, candidate 2 the larger minimum."""
    rel = np.array([0.5, 0.25, 0.25, 0.375, 0.0])
    joint = np.zeros((5, 5))

    def put(i, j, v):
        joint[i, j] = joint[j, i] = v

    put(0, 3, 1.0)      # after 0: 3 is the best of both methods
    put(0, 1, 0.9375)
    put(0, 2, 0.75)
    put(3, 1, 0.5)      # given 3, candidate 1 adds little: 0.5 - 0.375
    put(3, 2, 0.625)
    assert L.jmi_search_matrix("cpu", rel, joint, 3, method="JMI").tolist() == [0, 3, 1]
    assert L.jmi_search_matrix("cpu", rel, joint, 3, method="CMIM").tolist() == [0, 3, 2]


@pytest.mark.parametrize("case", jmi_np.PLANTED)
def test_planted_interaction(case):
    from fastselect_amd import JMI, mRMR
    n, p, seed, a, b, states, classes = case
    X, y = jmi_np.planted_pair(n, p, seed, a, b, states, classes)
    S, C = int(max(X.max(), y.max())) + 1, int(y.max()) + 1
    rel = jmi_np.relevance(X, y, S)
    for method in jmi_np.METHODS:
        want, margins = jmi_np.greedy(rel, lambda s: jmi_np.row(X, y, s, S, C), 2, method)
        assert margins.min() >= mi_np.PLANT_MARGIN
        assert want.tolist() == [a, b]
        for backend in ("cpu", "auto"):
            est = JMI(2, method=method, backend=backend).fit(X, y)
            assert est.top_features_.tolist() == [a, b], (method, backend)
    if states == 2:
        # b has no relevance of its own: mRMR passes it over
        rank = int(np.where(np.argsort(-rel) == b)[0][0]) + 1
        assert rank > 10
        got = mRMR(2, redundancy="selected", backend="cpu").fit(X, y).top_features_
        assert got[0] == a and b not in got.tolist()


# ---- the estimator ----------------------------------------------------------

def test_estimator_attributes_and_params():
    from sklearn.base import clone
    from fastselect_amd import JMI
    n, p, seed, a, b, states, classes = jmi_np.PLANTED[2]
    X, y = jmi_np.planted_pair(n, p, seed, a, b, states, classes)
    est = JMI(4, method="CMIM", backend="cpu", n_jobs=2)
    assert est.get_params() == {"n_features_to_select": 4, "method": "CMIM", "backend": "cpu",
                                "n_jobs": 2, "device": 0, "unit": "bit"}
    assert clone(est).get_params() == est.get_params()
    assert JMI(3).get_params()["method"] == "JMI" and JMI(3).get_params()["backend"] == "auto"
    est.fit(X, y)
    S = int(max(X.max(), y.max())) + 1
    sel, rel, rows = L.jmi_select("cpu", X, y, S, 4, method="CMIM")
    assert est.effective_backend_ == "cpu" and est.n_features_in_ == p
    assert est.top_features_.dtype == np.int32 and np.array_equal(est.top_features_, sel)
    assert np.array_equal(est.relevance_scores_, rel)
    assert est.feature_importances_ is est.relevance_scores_
    assert est.joint_relevance_rows_.shape == (4, p)
    assert np.array_equal(est.joint_relevance_rows_, rows)
    assert np.array_equal(est.transform(X), X[:, sel])
    assert np.array_equal(JMI(4, method="CMIM", backend="cpu").fit_transform(X, y), X[:, sel])
    nat = JMI(4, method="CMIM", backend="cpu", unit="nat").fit(X, y)
    assert np.abs(nat.relevance_scores_ - rel * np.log(2.0)).max() <= TOL


def test_estimator_encodes_each_column_by_its_own_values():
    """Floats, and integers with gaps: the codes are each column's ranks."""
    from fastselect_amd import JMI
    n, p, seed, a, b, states, classes = jmi_np.PLANTED[2]
    X, y = jmi_np.planted_pair(n, p, seed, a, b, states, classes)
    base = JMI(3, backend="cpu").fit(X, y)
    gaps = X * 40 + 7                      # codes 7, 47, 87: more than 32 as raw states
    gaps[:, 1] = X[:, 1] * 100 - 100       # a negative value, another spacing
    ygap = y * 5 + 100
    for Xv, yv in ((gaps, ygap), (X * 0.5 - 1.0, y.astype(np.float64))):
        est = JMI(3, backend="cpu").fit(Xv, yv)
        assert np.array_equal(est.top_features_, base.top_features_)
        assert np.array_equal(est.relevance_scores_, base.relevance_scores_)
        assert np.array_equal(est.joint_relevance_rows_, base.joint_relevance_rows_)
        assert np.array_equal(est.transform(Xv), Xv[:, base.top_features_])


def test_estimator_in_a_pipeline_with_mdr():
    from sklearn.pipeline import Pipeline
    from fastselect_amd import JMI, MDR
    X, y = mdr_np.planted(160, 60, pair=(7, 41))
    pipe = Pipeline([("jmi", JMI(10)), ("mdr", MDR(k=2, cv=3))])
    pred = pipe.fit(X, y).predict(X)
    assert pred.shape == (160,) and set(np.unique(pred)) <= {0, 1}
    assert pipe.named_steps["mdr"].n_features_in_ == 10
    assert pipe.named_steps["jmi"].top_features_.shape == (10,)


def test_estimator_rejections():
    from sklearn.exceptions import NotFittedError
    from fastselect_amd import JMI
    X, y = jmi_np.planted_pair(120, 8, 1, 2, 5)
    with pytest.raises(ValueError, match="method"):
        JMI(2, method="MID").fit(X, y)
    with pytest.raises(ValueError, match="backend"):
        JMI(2, backend="tpu").fit(X, y)
    with pytest.raises(ValueError, match="unit"):
        JMI(2, unit="dit").fit(X, y)
    for k in (0, 9):
        with pytest.raises(ValueError, match="n_features_to_select"):
            JMI(k).fit(X, y)
    with pytest.raises(NotFittedError):
        JMI(2).transform(X)
    wide = np.arange(300 * 2).reshape(300, 2) % np.array([257, 3])
    with pytest.raises(ValueError, match="discretise"):
        JMI(1).fit(wide, np.arange(300) % 2)
    if not L.gpu_available():
        with pytest.raises(RuntimeError):
            JMI(2, backend="gpu").fit(X, y)


def test_auto_takes_the_cpu_beyond_the_gpu_limits():
    from fastselect_amd import JMI
    from fastselect_amd import mutual_information as mi
    X33, y33 = mi_np.uniform(90, 3, 33, 33, 2)
    X33 = X33.copy()
    X33[:33, 0] = np.arange(33)            # one column does take 33 values
    est = JMI(2, backend="auto").fit(X33, y33)
    assert est.effective_backend_ == "cpu"
    X5, y5 = mi_np.uniform(120, 4, 3, 34, 5)
    est = JMI(2, backend="auto").fit(X5, y5)
    assert est.effective_backend_ == "cpu"
    S = 5
    assert np.abs(est.joint_relevance_rows_
                  - jmi_np.rows(X5, y5, est.top_features_, S, 5)).max() <= TOL
    for Xv, yv in ((X33, y33), (X5, y5)):
        with pytest.raises(RuntimeError):   # no device, or beyond the limit: never a fallback
            JMI(2, backend="gpu").fit(Xv, yv)
        with pytest.raises(RuntimeError):
            mi.calculate_joint_relevance(Xv, yv, [0], backend="gpu")
    assert mi._choose_backend_joint("cpu", 33, 5) == "cpu"
    assert mi._choose_backend_joint("auto", 33, 2) == "cpu"
    assert mi._choose_backend_joint("auto", 3, 5) == "cpu"


def test_calculate_joint_relevance():
    from fastselect_amd import mutual_information as mi
    X, y, S, C, anchors, allrows = _case("states5")
    got = mi.calculate_joint_relevance(X, y, anchors, backend="cpu")
    assert np.array_equal(got, allrows[anchors])
    assert np.array_equal(mi.calculate_joint_relevance(X, y, 2, backend="cpu"), allrows[[2]])
    with pytest.raises(ValueError, match="anchor"):
        mi.calculate_joint_relevance(X, y, [X.shape[1]], backend="cpu")
    with pytest.raises(ValueError, match="anchor"):
        mi.calculate_joint_relevance(X, y, [], backend="cpu")
    with pytest.raises(ValueError, match="integer"):
        mi.calculate_joint_relevance(X.astype(np.float64), y, [0], backend="cpu")
    with pytest.raises(ValueError, match="backend"):
        mi.calculate_joint_relevance(X, y, [0], backend="tpu")
