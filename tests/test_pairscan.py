"""The pair screen on the CPU backend (fs_pairscan_cpu.cpp, PairScreen.py,
mutual_information.rank_pair_interactions).

Without a tolerance (array_equal): the list and the per-feature maxima equal
pairscan_np.expected built from the same backend's fs_jmi_rows at every anchor
and fs_mi_matrices' relevance, for both scores, every thread count and every
list length: the screen runs the row code's table and mi_from_table on the same
integers and forms the score by the same float64 expression.

Against the numpy restatement (jmi_np) the scores lie within the TOL of
test_jmi.py, 1e-10, derived there for a table of S^2 * C cells; the gain adds
two subtractions of values below 22 nats, 5e-15.
"""
import math

import numpy as np
import pytest

import jmi_np
import mi_np
import pairscan_np

from fastselect_amd import _lib as L

TOL = 1e-10
SCORES = ("joint", "gain")

_CASES = {}


def _case(name, make):
    """(X, y, S, C, J of the CPU backend at every anchor, its relevance)."""
    if name not in _CASES:
        X, y, S = make()
        X = np.ascontiguousarray(X, dtype=np.uint8)
        y = np.ascontiguousarray(y, dtype=np.uint8)
        J = L.jmi_rows("cpu", X, y, S, np.arange(X.shape[1]))
        rel, _ = L.mi_matrices("cpu", X, y, S)
        for a in (X, y, J, rel):
            a.setflags(write=False)
        _CASES[name] = (X, y, S, int(y.max()) + 1, J, rel)
    return _CASES[name]


SHAPES = {
    "p17_tile16": mi_np.SHAPES["p17_tile16"],
    "p9_tile8": mi_np.SHAPES["p9_tile8"],
    "states10": mi_np.SHAPES["states10"],
    "mixed": mi_np.SHAPES["mixed"],
    "y4": mi_np.SHAPES["y4"],
    "n203": mi_np.SHAPES["n203"],
    "tied": pairscan_np.tied,
    "all_constant": pairscan_np.all_constant,
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_against_numpy(name):
    X, y, S, C, _, _ = _case(name, SHAPES[name])
    p = X.shape[1]
    J = jmi_np.rows(X, y, range(p), S, C)
    rel = jmi_np.relevance(X, y, S)
    total = p * (p - 1) // 2
    for score in SCORES:
        want, _, _ = pairscan_np.scores(J, rel, score)
        grel, gs, gp, gbest = L.pair_screen("cpu", X, y, S, n_top=total, score=score)
        assert gs.shape == (total,) and gp.shape == (total, 2)
        assert np.abs(grel - rel).max() <= TOL
        # every pair once, and each score within TOL of the restatement's
        rank = gp[:, 0] * (2 * p - gp[:, 0] - 1) // 2 + gp[:, 1] - gp[:, 0] - 1
        assert np.array_equal(np.sort(rank), np.arange(total))
        print(name, score, np.abs(gs - want[rank]).max())
        assert np.abs(gs - want[rank]).max() <= TOL
        assert np.all(np.diff(gs) <= 0.0)
        _, _, wbest = pairscan_np.expected(J, rel, score, total)
        assert np.abs(gbest - wbest).max() <= TOL


@pytest.mark.parametrize("score", SCORES)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_against_jmi_rows_bit_for_bit(name, score):
    X, y, S, C, J, rel = _case(name, SHAPES[name])
    p = X.shape[1]
    total = p * (p - 1) // 2
    for n_top in (1, 7, total, total + 5):
        ws, wp, wbest = pairscan_np.expected(J, rel, score, n_top)
        for n_jobs in (1, 3, 16):
            grel, gs, gp, gbest = L.pair_screen("cpu", X, y, S, n_top=n_top, score=score,
                                                n_jobs=n_jobs)
            assert np.array_equal(grel, rel)
            assert np.array_equal(gs, ws) and np.array_equal(gp, wp), (n_top, n_jobs)
            assert np.array_equal(gbest, wbest)


def test_fill_past_the_last_pair():
    """The raw arrays behind n_top = C(p,2) + 5: score 0.0 and i = j = -1."""
    import ctypes
    X, y, S, C, J, rel = _case("n203", SHAPES["n203"])
    p = X.shape[1]
    total = p * (p - 1) // 2
    n_top = total + 5
    f64p, i64p, u8p = (ctypes.POINTER(t) for t in (ctypes.c_double, ctypes.c_int64, ctypes.c_uint8))
    r = np.zeros(p)
    ts = np.full(n_top, 9.0)
    ti = np.full(n_top, 9, np.int64)
    tj = np.full(n_top, 9, np.int64)
    rc = L.lib().fs_pair_screen(L.BACKEND_CPU, 0, X.ctypes.data_as(u8p), y.ctypes.data_as(u8p),
                                X.shape[0], p, S, 0, 0, n_top, 2, r.ctypes.data_as(f64p),
                                ts.ctypes.data_as(f64p), ti.ctypes.data_as(i64p),
                                tj.ctypes.data_as(i64p), None)
    assert rc == L.FS_OK
    assert not ts[total:].any() and (ti[total:] == -1).all() and (tj[total:] == -1).all()
    ws, wp, _ = pairscan_np.expected(J, rel, "joint", total)
    assert np.array_equal(ts[:total], ws) and np.array_equal(ti[:total], wp[:, 0])
    assert np.array_equal(tj[:total], wp[:, 1])


@pytest.mark.parametrize("case", pairscan_np.PLANTED)
def test_planted_pairs(case):
    from fastselect_amd import JMI, PairScreen
    (n, p, seed, a, b, states), j_top, j_next, jmi_misses = case
    X, y = pairscan_np.pure(n, p, seed, a, b, states)
    lo, hi = min(a, b), max(a, b)
    for score in SCORES:
        rel, ts, tp, best = L.pair_screen("cpu", X, y, states, n_top=3, score=score)
        assert tp[0].tolist() == [lo, hi], score
        if score == "joint":
            assert abs(ts[0] - j_top) < 1e-3 and abs(ts[1] - j_next) < 1e-3
    est = PairScreen(n_features_to_select=2, backend="cpu").fit(X, y)
    assert set(est.top_features_.tolist()) == {a, b}
    assert est.top_pairs_[0].tolist() == [lo, hi]
    if jmi_misses:
        for method in jmi_np.METHODS:
            picks = JMI(n_features_to_select=4, method=method, backend="cpu").fit(X, y)
            assert a not in picks.top_features_ and b not in picks.top_features_


def test_ties_take_the_lowest_ranks():
    X, y, S, C, J, rel = _case("tied", pairscan_np.tied)
    p = X.shape[1]
    s, i, j = pairscan_np.scores(J, rel, "joint")
    # the pair of constants is exactly 0.0; the duplicated columns give runs of
    # equal scores
    assert J[1, 4] == 0.0
    assert J[0, 2] == J[0, 5] == J[0, 6] and J[3, 5] == J[3, 6]
    order = np.argsort(-s, kind="stable")
    runs = [t for t in range(1, s.size) if s[order[t]] == s[order[t - 1]]]
    assert len(runs) >= 4
    for cut in runs[:4]:               # n_top ends inside a run of equal scores
        ws, wp, _ = pairscan_np.expected(J, rel, "joint", cut)
        _, gs, gp, _ = L.pair_screen("cpu", X, y, S, n_top=cut, score="joint")
        assert np.array_equal(gs, ws) and np.array_equal(gp, wp)
        # the one left out has the same score and a higher rank
        assert s[order[cut]] == gs[-1] and order[cut] > order[cut - 1]


def test_all_constant_columns():
    X, y, S = pairscan_np.all_constant()
    p = X.shape[1]
    import itertools
    first = list(itertools.combinations(range(p), 2))
    for score in SCORES:
        for n_top in (1, 5, len(first)):
            rel, gs, gp, best = L.pair_screen("cpu", X, y, S, n_top=n_top, score=score)
            assert not rel.any() and not gs.any() and not best.any()
            assert not np.signbit(gs).any() and not np.signbit(best).any()
            assert [tuple(r) for r in gp.tolist()] == first[:n_top]


def test_rank_pair_interactions():
    from fastselect_amd import mutual_information as mi
    (n, p, seed, a, b, states), _, _, _ = pairscan_np.PLANTED[0]
    X, y = pairscan_np.pure(n, p, seed, a, b, states)
    pairs, sc, rel, best = mi.rank_pair_interactions(X, y, n_top=4, backend="cpu")
    wrel, ws, wp, wbest = L.pair_screen("cpu", X, y, states, n_top=4, score="gain")
    assert np.array_equal(pairs, wp) and np.array_equal(sc, ws)
    assert np.array_equal(rel, wrel) and np.array_equal(best, wbest)
    pj, sj, _, _ = mi.rank_pair_interactions(X, y, 4, score="joint", backend="cpu", unit="nat")
    _, wsj, wpj, _ = L.pair_screen("cpu", X, y, states, n_top=4, score="joint", unit="nat")
    assert np.array_equal(pj, wpj) and np.array_equal(sj, wsj)
    assert abs(sj[0] * (1.0 / math.log(2.0)) - 0.524) < 1e-3
    # JMI's functions' messages for float and negative input
    with pytest.raises(ValueError, match="integer"):
        mi.rank_pair_interactions(X.astype(np.float64), y, backend="cpu")
    with pytest.raises(ValueError, match="negative"):
        mi.rank_pair_interactions(X - 1, y, backend="cpu")
    with pytest.raises(ValueError, match="integer"):
        mi.rank_pair_interactions(X, y * 0.5, backend="cpu")
    with pytest.raises(ValueError, match="matching sample size"):
        mi.rank_pair_interactions(X, y[:-1], backend="cpu")
    with pytest.raises(ValueError, match="two columns"):
        mi.rank_pair_interactions(X[:, :1], y, backend="cpu")
    for bad in (0, 65537):
        with pytest.raises(ValueError, match="n_top"):
            mi.rank_pair_interactions(X, y, bad, backend="cpu")
    with pytest.raises(ValueError, match="score"):
        mi.rank_pair_interactions(X, y, score="sum", backend="cpu")
    with pytest.raises(ValueError, match="backend"):
        mi.rank_pair_interactions(X, y, backend="tpu")


def test_estimator_surface():
    from sklearn.base import clone
    from fastselect_amd import JMI, PairScreen
    (n, p, seed, a, b, states), _, _, _ = pairscan_np.PLANTED[0]
    X, y = pairscan_np.pure(n, p, seed, a, b, states)
    est = PairScreen(3, n_top=10, score="joint", backend="cpu", n_jobs=2)
    assert est.get_params() == {"n_features_to_select": 3, "n_top": 10, "score": "joint",
                                "backend": "cpu", "unit": "bit", "n_jobs": 2, "device": 0}
    est.set_params(n_features_to_select=2, score="gain")
    twin = clone(est).fit(X, y)
    est.fit(X, y)
    assert est.effective_backend_ == "cpu" and est.n_features_in_ == p
    assert est.top_pairs_.shape == (10, 2) and est.top_scores_.shape == (10,)
    assert est.relevance_scores_.shape == (p,) and est.interaction_scores_.shape == (p,)
    assert est.feature_importances_ is est.interaction_scores_
    want = np.argsort(-est.interaction_scores_, kind="stable")[:2]
    assert np.array_equal(est.top_features_, want) and est.top_features_.dtype == np.int32
    assert np.array_equal(twin.top_pairs_, est.top_pairs_)
    assert np.array_equal(est.transform(X), X[:, est.top_features_])
    assert est.fit_transform(X, y).shape == (n, 2)
    assert PairScreen.__module__ == "fastselect_amd"
    # the encoding is JMI.fit's: any values, by their sorted unique ones
    Xf = X * 0.5 - 1.0
    enc = PairScreen(2, n_top=10, backend="cpu").fit(Xf, y.astype(np.float64))
    assert np.array_equal(enc.top_pairs_, est.top_pairs_)
    assert np.array_equal(enc.top_scores_, est.top_scores_)
    assert np.array_equal(enc.relevance_scores_, JMI(1, backend="cpu").fit(Xf, y).relevance_scores_)


def test_estimator_in_a_pipeline_with_mdr():
    from sklearn.pipeline import Pipeline
    from fastselect_amd import MDR, PairScreen
    (n, p, seed, a, b, states), _, _, _ = pairscan_np.PLANTED[0]
    X, y = pairscan_np.pure(n, p, seed, a, b, states)
    pipe = Pipeline([("screen", PairScreen(4, backend="cpu")),
                     ("mdr", MDR(k=2, cv=3, backend="cpu"))])
    pipe.fit(X, y)
    kept = pipe.named_steps["screen"].top_features_
    assert {a, b} <= set(kept.tolist())
    best = pipe.named_steps["mdr"].best_interaction_
    assert {int(kept[f]) for f in best} == {a, b}


def test_estimator_rejections():
    from fastselect_amd import PairScreen
    X, y = mi_np.uniform(60, 5, 3, 7, 2)
    for k in (0, 6, -1):
        with pytest.raises(ValueError, match="n_features_to_select"):
            PairScreen(k, backend="cpu").fit(X, y)
    with pytest.raises(ValueError, match="score"):
        PairScreen(2, score="sum", backend="cpu").fit(X, y)
    with pytest.raises(ValueError, match="backend"):
        PairScreen(2, backend="tpu").fit(X, y)
    with pytest.raises(ValueError, match="unit"):
        PairScreen(2, unit="ban", backend="cpu").fit(X, y)
    for bad in (0, 65537):
        with pytest.raises(ValueError, match="n_top"):
            PairScreen(2, n_top=bad, backend="cpu").fit(X, y)
    with pytest.raises(ValueError, match="two features"):
        PairScreen(1, backend="cpu").fit(X[:, :1], y)
    with pytest.raises(ValueError, match="discretise"):
        PairScreen(2, backend="cpu").fit(np.arange(600.0).reshape(300, 2), np.arange(300) % 2)


def test_auto_takes_the_cpu_beyond_the_gpu_limits():
    from fastselect_amd import PairScreen
    from fastselect_amd import mutual_information as mi
    X33, y33 = mi_np.uniform(90, 3, 33, 33, 2)
    X33 = X33.copy()
    X33[:33, 0] = np.arange(33)              # one column takes all 33 values
    X5, y5 = mi_np.uniform(120, 4, 5, 34, 5)
    for X, y in ((X33, y33), (X5, y5)):
        est = PairScreen(2).fit(X, y)
        assert est.effective_backend_ == "cpu"
        pairs, sc, _, _ = mi.rank_pair_interactions(X, y)
        assert np.array_equal(pairs, est.top_pairs_) and np.array_equal(sc, est.top_scores_)
