"""JMI / CMIM on the GPU (fs_jmi.hip).  A row of joint relevance must equal the
GPU fs_mi_matrices relevance of the synthetic joint columns x_lo * S + x_hi bit
for bit wherever those fit the GPU's 32 states (2 to 5 states; k_jmi_row runs
mi_from_table's steps in k_mi_scan's order), and lie within TOL of the CPU
backend and of the numpy restatement everywhere (TOL = 1e-10, derived for
S^2 * C terms in test_jmi.py).  Routes of the same backend agree bit for bit.

Shapes are the smallest at which the row kernel can go wrong.  k_jmi_row takes
CPW(SP, C) = 256 / NB^2 columns per workgroup (NB = ceil(states / 4)) whatever
the class count C is: it keeps one table row in LDS, not the table, so CPW does
not shrink with C.  y is one more column of the planes, it stages 64 words
(2048 samples) per chunk, and C in 2..4 is a template parameter:

* 3 states (CPW = 256): p = 255 (y is the last lane's column of the only
  workgroup), 256 (y alone in a second workgroup), 257, 514 (three workgroups),
  each with 2, 3 and 4 classes;
* 5 states (CPW = 64, four lanes a pair): p = 63, 64, 65, 130 with 2 classes;
* 10 states x 2 classes at p = 29 (28 pairs per workgroup, 4 idle lanes);
  32 states x 4 classes at p = 9, n = 257: every byte of the staging area;
* n = 33 / 64 / 203 / 2049: over a word boundary, whole words, a ragged word,
  and one restaging of LDS;
* anchors 0, p // 2 and p - 1: both table orientations in every workgroup;
* mixed columns (a constant column, codes {0, 4} only, 2 beside 32 states) with
  4 classes of y; a one-class y (no scan); a pair of constant columns;
* 4, 8, 12, 13, 16, 17, 20, 21, 24, 25, 28 and 29 states at n = 97 and 257
  (mi_np.geometry_dims), each with 2, 3 and 4 classes: both ends of every NB, so
  16-, 25-, 36- and 49-lane pairs and 10, 7, 5 columns per workgroup with idle
  lanes; per state count p = CPW - 1, CPW, CPW + 1 and 2T + 1; mixed columns
  with the state bound at 21 and at 25.  The synthetic-column identity applies
  at 4 states only; rows and selection are checked on all of them;
* n = 2048, 4096 and 4097 (mi_np.LONG): whole staging chunks and two restages.
"""
import numpy as np
import pytest

import jmi_np
import mi_np

pytestmark = pytest.mark.gpu

TOL = 1e-10


@pytest.fixture(scope="module")
def L():
    from fastselect_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    return _lib


def _u(n, p, states, seed, classes):
    return lambda: mi_np.uniform(n, p, states, seed, classes) + (max(states, classes),)


def _one_class():
    X, _ = mi_np.uniform(97, 7, 3, 91)
    return X, np.zeros(97, np.uint8), 3


def _constant_pair():
    X, y = mi_np.uniform(97, 6, 3, 92, 2)
    X = X.copy()
    X[:, 1] = 2
    X[:, 3] = 1
    return X, y, 3


SHAPES = {}
for _c in (2, 3, 4):
    for _p in (255, 256, 257, 514):
        SHAPES["s3_c%d_p%d" % (_c, _p)] = _u(65, _p, 3, 100 * _c + _p % 97, _c)
for _p in (63, 64, 65, 130):
    SHAPES["s5_c2_p%d" % _p] = _u(65, _p, 5, 70 + _p % 11, 2)
SHAPES.update({
    "s10_c2_p29": _u(150, 29, 10, 81, 2),
    "s32_c4_p9": _u(257, 9, 32, 82, 4),
    "n33": mi_np.SHAPES["n33"],
    "n64": mi_np.SHAPES["n64"],
    "n203": mi_np.SHAPES["n203"],
    "n2049": mi_np.SHAPES["restage"],
    "mixed_c4": mi_np.SHAPES["mixed"],
    "one_class": _one_class,
    "constant_pair": _constant_pair,
})
GEOMETRY = {}
for _d in mi_np.geometry_dims():
    for _c in (2, 3, 4):
        GEOMETRY[mi_np.geometry_name(*_d, classes=_c)] = mi_np.geometry_case(*_d, classes=_c)
GEOMETRY["geo_mixed_s21"] = mi_np.GEOMETRY["geo_mixed_s21"]
GEOMETRY["geo_mixed_s25"] = mi_np.GEOMETRY["geo_mixed_s25"]
SHAPES.update(GEOMETRY)
SHAPES.update(mi_np.LONG)

_DATA = {}


def _data(name):
    if name not in _DATA:
        X, y, S = SHAPES[name]()
        X = np.ascontiguousarray(X, dtype=np.uint8)
        y = np.ascontiguousarray(y, dtype=np.uint8)
        X.setflags(write=False)
        y.setflags(write=False)
        _DATA[name] = (X, y, S, int(y.max()) + 1)
    return _DATA[name]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_rows(L, name):
    X, y, S, C = _data(name)
    p = X.shape[1]
    anchors = [0, p // 2, p - 1]
    got = L.jmi_rows("gpu", X, y, S, anchors)
    assert all(got[t, a] == 0.0 for t, a in enumerate(anchors))
    cpu = L.jmi_rows("cpu", X, y, S, anchors)
    want = jmi_np.rows(X, y, anchors, S, C)
    print(name, "gpu-cpu", np.abs(got - cpu).max(), "gpu-numpy", np.abs(got - want).max())
    assert np.abs(got - cpu).max() <= TOL
    assert np.abs(got - want).max() <= TOL
    if name == "one_class":
        assert not got.any()
    if name == "constant_pair":
        assert got[1, 1] == 0.0 and got[0, 1] == L.mrmr_select("gpu", X, y, S, 1)[1][0]
    if S * S <= 32:
        for t, a in enumerate(anchors):
            Z = jmi_np.synthetic(X, a, S)
            rel, _ = L.mi_matrices("gpu", Z, y, int(max(Z.max(), y.max())) + 1)
            keep = np.arange(p) != a
            assert np.array_equal(got[t][keep], rel[keep]), a
    # two calls, and another company of anchors: identical bits
    assert np.array_equal(L.jmi_rows("gpu", X, y, S, anchors[::-1]), got[::-1])


SELECT = ["s3_c2_p257", "s3_c3_p256", "s3_c4_p255", "s5_c2_p130", "s10_c2_p29", "s32_c4_p9",
          "mixed_c4", "n2049", "one_class", "constant_pair"] + sorted(GEOMETRY)


@pytest.mark.parametrize("name", SELECT)
def test_select(L, name):
    X, y, S, C = _data(name)
    p = X.shape[1]
    k = p if p <= 130 else 24
    allrows = L.jmi_rows("gpu", X, y, S, np.arange(p))
    assert np.array_equal(allrows, allrows.T)
    _, mrel, _ = L.mrmr_select("gpu", X, y, S, 1, want_rows=False)
    for method in jmi_np.METHODS:
        sel, rel, rows = L.jmi_select("gpu", X, y, S, k, method=method)
        assert np.array_equal(rel, mrel)
        assert np.array_equal(rows, allrows[sel]), method
        want, _ = jmi_np.greedy(rel, lambda s: allrows[s], k, method)
        assert np.array_equal(sel, want), method
        sel2, rel2, rows2 = L.jmi_select("gpu", X, y, S, k, method=method)
        assert np.array_equal(sel2, sel) and np.array_equal(rel2, rel)
        assert np.array_equal(rows2, rows)
        sel3, rel3, none = L.jmi_select("gpu", X, y, S, k, method=method, want_rows=False)
        assert none is None and np.array_equal(sel3, sel) and np.array_equal(rel3, rel)
        timing = L.jmi_last_timing()
        assert len(timing) == 5 and all(t >= 0.0 for t in timing[:3])


@pytest.mark.parametrize("method", jmi_np.METHODS)
@pytest.mark.parametrize("p,k,seed", jmi_np.TIE_CASES)
def test_tie_and_min_rules(L, p, k, seed, method):
    rel, joint = jmi_np.tie_inputs(p, seed)
    assert jmi_np.exact_tie_steps(rel, joint, k, method) >= 5
    want, _ = jmi_np.greedy(rel, lambda s: joint[s], k, method)
    got = L.jmi_search_matrix("gpu", rel, joint, k, method=method)
    assert np.array_equal(got, want)
    assert np.array_equal(L.jmi_search_matrix("gpu", rel, joint, k, method=method), got)
    assert np.array_equal(L.jmi_search_matrix("cpu", rel, joint, k, method=method), got)


@pytest.mark.parametrize("case", jmi_np.PLANTED)
def test_planted_interaction(L, case):
    from fastselect_amd import JMI
    n, p, seed, a, b, states, classes = case
    X, y = jmi_np.planted_pair(n, p, seed, a, b, states, classes)
    S, C = int(max(X.max(), y.max())) + 1, int(y.max()) + 1
    rel = jmi_np.relevance(X, y, S)
    for method in jmi_np.METHODS:
        want, margins = jmi_np.greedy(rel, lambda s: jmi_np.row(X, y, s, S, C), 2, method)
        assert margins.min() >= mi_np.PLANT_MARGIN
        g = JMI(2, method=method, backend="gpu").fit(X, y)
        c = JMI(2, method=method, backend="cpu").fit(X, y)
        auto = JMI(2, method=method).fit(X, y)
        assert g.effective_backend_ == "gpu" and auto.effective_backend_ == "gpu"
        assert g.top_features_.tolist() == [a, b] == want.tolist()
        assert np.array_equal(g.top_features_, c.top_features_)
        assert np.array_equal(auto.top_features_, g.top_features_)
        assert np.array_equal(auto.joint_relevance_rows_, g.joint_relevance_rows_)
        assert np.abs(g.joint_relevance_rows_ - c.joint_relevance_rows_).max() <= TOL
        assert np.abs(g.relevance_scores_ - c.relevance_scores_).max() <= TOL


def test_width_100000(L):
    """p = 100000, 391 workgroups a row.  With 65 samples and 100000 noise
    columns many candidates reach the same joint relevance in exact
    arithmetic, and the two backends' log() may order them differently; so the
    selection is checked against the greedy loop on the GPU's own rows, and the
    rows against the CPU backend at the same anchors."""
    n, p, k = 65, 100000, 3
    X, y = mi_np.planted(n, p, 3, 1)
    X = X.astype(np.uint8)
    y = y.astype(np.uint8)
    for method in jmi_np.METHODS:
        sel, rel, rows = L.jmi_select("gpu", X, y, 3, k, method=method)
        timing = L.jmi_last_timing()
        assert len(timing) == 5 and all(t >= 0.0 for t in timing)
        assert rows.shape == (k, p) and sel[0] == int(np.argmax(rel))
        place = {int(s): t for t, s in enumerate(sel)}
        want, _ = jmi_np.greedy(rel, lambda s: rows[place[s]], k, method)
        assert np.array_equal(sel, want)
        assert all(rows[t, s] == 0.0 for t, s in enumerate(sel))
        cpu = L.jmi_rows("cpu", X, y, 3, sel)
        assert np.abs(rows - cpu).max() <= TOL
        assert np.array_equal(L.jmi_rows("gpu", X, y, 3, sel), rows)
    _, crel, _ = L.jmi_select("cpu", X, y, 3, 1, want_rows=False)
    assert np.abs(rel - crel).max() <= TOL


def test_many_steps_are_timed_as_a_whole(L):
    """Above 64 steps the loop is timed by two events: rows holds it, steps
    is unavailable."""
    X, y, S, C = _data("s5_c2_p130")
    sel, _, _ = L.jmi_select("gpu", X, y, S, 70)
    up, pack, relv, rows, steps = L.jmi_last_timing()
    assert len(set(sel.tolist())) == 70
    assert min(up, pack, relv, rows) >= 0.0 and steps == -1.0


def test_rejections(L):
    from fastselect_amd import JMI
    from fastselect_amd import mutual_information as mi
    X, y = mi_np.uniform(64, 5, 3, 42, 2)
    X = X.copy()
    X[63, 4] = 3
    with pytest.raises(ValueError, match=">= n_states"):
        L.jmi_select("gpu", X, y, 3, 2)
    with pytest.raises(ValueError, match=">= n_states"):
        L.jmi_rows("gpu", X, y, 3, [0, 4])
    X[63, 4] = 0
    yb = y.copy()
    yb[10] = 3
    with pytest.raises(ValueError, match=">= n_states"):
        L.jmi_select("gpu", X, yb, 3, 2)
    # a code beyond the padded state count, too
    X[5, 1] = 200
    with pytest.raises(ValueError, match=">= n_states"):
        L.jmi_select("gpu", X, y, 3, 5)
    X5, y5 = mi_np.uniform(120, 4, 5, 34, 5)
    with pytest.raises(ValueError, match="4 classes"):
        L.jmi_select("gpu", X5, y5, 5, 2)
    with pytest.raises(ValueError, match="4 classes"):
        L.jmi_rows("gpu", X5, y5, 5, [0])
    with pytest.raises(RuntimeError, match="classes"):
        JMI(2, backend="gpu").fit(X5, y5)
    with pytest.raises(RuntimeError, match="classes"):
        mi.calculate_joint_relevance(X5, y5, [0], backend="gpu")
    assert JMI(2).fit(X5, y5).effective_backend_ == "cpu"
    X33, y33 = mi_np.uniform(90, 3, 33, 33, 2)
    with pytest.raises(ValueError, match="32 states"):
        L.jmi_select("gpu", X33, y33, 33, 2)
    with pytest.raises(ValueError, match="32 states"):
        L.jmi_rows("gpu", X33, y33, 33, [0])
    with pytest.raises(ValueError, match="anchor"):
        L.jmi_rows("gpu", X33[:, :3] % 3, y33, 3, [3])
    with pytest.raises(ValueError, match="k must be"):
        L.jmi_select("gpu", X33 % 3, y33, 3, 4)
    # the device still answers
    Xo, yo = mi_np.uniform(64, 5, 3, 42, 2)
    sel, _, rows = L.jmi_select("gpu", Xo, yo, 3, 5)
    assert sorted(sel.tolist()) == [0, 1, 2, 3, 4]
    assert np.abs(rows - L.jmi_rows("cpu", Xo, yo, 3, sel)).max() <= TOL
    got = mi.calculate_joint_relevance(Xo, yo, [1, 3], backend="gpu")
    assert np.array_equal(got, L.jmi_rows("gpu", Xo, yo, 3, [1, 3]))
