"""The pair screen on the GPU (fs_pairscan.hip, k_pair_scan).

The identity that pins the kernel, without a tolerance: the list equals
pairscan_np.expected built from the GPU's own fs_jmi_rows at every anchor and
the GPU relevance, and feature_best the row maxima of that score matrix: the
same backend, the same expressions in the same order (k_pair_scan runs
k_jmi_row's epilogue), and the selection is exact.

Shapes are the smallest at which the tiled kernel can go wrong.  k_pair_scan
takes one workgroup per tile of T x T pairs of the upper triangle, T(SP) =
16 / NB columns a side with NB = ceil(states / 4): T = 16 at 3 states, 8 at 5,
5 at 10 (225 of 256 lanes), 2 at 32.  y is one more column of the planes, the
kernel stages 64 words (2048 samples) per chunk, and the class count C in 2..4
is a template parameter:

* 3 states: p = T - 1, T, T + 1 and 2T + 1 (15, 16, 17, 33): one ragged tile,
  one full tile, a second block of one column, three blocks; each with 2, 3 and
  4 classes;
* 5 states, 2 classes: p = 7, 8, 9, 17;
* 10 states x 2 classes at p = T + 1 = 6: idle lanes in every workgroup;
* 32 states x 4 classes at p = 2, 3 and 5, n = 257: every byte of the staging
  area and of the row buffer;
* n = 33, 64, 203, 2049 (one restage) and 4097 (two restages);
* the state counts of mi_np.geometry_dims (both ends of every NB) at n = 97 and
  257, 2 and 4 classes, p = T + 1;
* mixed columns with 4 classes, a one-class y (no scan), constant and duplicated
  columns (runs of exactly equal scores), all columns constant;
* routes, on 3 states at p = 4T + 3 = 67 (15 tiles): one tile a launch, four
  tiles a launch, a candidate buffer of one tile (pair_cap = 64 is raised to the
  256 pairs of a tile: launches are sized to the buffer, so by itself a small
  buffer gives many small launches and a rising threshold, never an overflow),
  and four tiles a launch into that buffer, where the first launch overflows
  and is run again in halves, twice; and on p = 1100 the product's own sizes
  with more than one launch.  Each route test first asserts by arithmetic that
  its shape takes the route.

Against the CPU backend the sorted score sequences agree position by position
within TOL = 1e-10 (test_jmi.py; each score moves by at most TOL, so each order
statistic does), and the pairs are equal wherever a score is more than 2 TOL
from both neighbours.
"""
import numpy as np
import pytest

import mi_np
import pairscan_np

pytestmark = pytest.mark.gpu

TOL = 1e-10
SCORES = ("joint", "gain")
THREADS = 256          # kPtThreads: the pairs of a tile at most, the buffer's floor


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
    for _p in (15, 16, 17, 33):
        SHAPES["s3_c%d_p%d" % (_c, _p)] = _u(65, _p, 3, 300 * _c + _p, _c)
for _p in (7, 8, 9, 17):
    SHAPES["s5_c2_p%d" % _p] = _u(65, _p, 5, 170 + _p, 2)
SHAPES["s10_c2_p6"] = _u(150, 6, 10, 181, 2)
for _p in (2, 3, 5):
    SHAPES["s32_c4_p%d" % _p] = _u(257, _p, 32, 190 + _p, 4)
SHAPES.update({
    "n33": mi_np.SHAPES["n33"],
    "n64": mi_np.SHAPES["n64"],
    "n203": mi_np.SHAPES["n203"],
    "n2049": mi_np.SHAPES["restage"],
    "n4097": mi_np.LONG["n4097"],
    "mixed_c4": mi_np.SHAPES["mixed"],
    "one_class": _one_class,
    "constant_pair": _constant_pair,
    "tied": pairscan_np.tied,
    "all_constant": pairscan_np.all_constant,
})
for _n, _s in sorted({(d[0], d[2]) for d in mi_np.geometry_dims()}):
    for _c in (2, 4):
        _p = mi_np.tile(_s) + 1
        SHAPES[mi_np.geometry_name(_n, _p, _s, classes=_c)] = mi_np.geometry_case(_n, _p, _s, _c)
SHAPES["route_p67"] = _u(65, 67, 3, 467, 2)

_DATA = {}


def _data(L, name):
    """(X, y, S, J of the GPU backend at every anchor, the GPU relevance)."""
    if name not in _DATA:
        X, y, S = SHAPES[name]()
        X = np.ascontiguousarray(X, dtype=np.uint8)
        y = np.ascontiguousarray(y, dtype=np.uint8)
        J = L.jmi_rows("gpu", X, y, S, np.arange(X.shape[1]))
        _, rel, _ = L.jmi_select("gpu", X, y, S, 1, want_rows=False)
        for a in (X, y, J, rel):
            a.setflags(write=False)
        _DATA[name] = (X, y, S, J, rel)
    return _DATA[name]


def _check(L, name, score, n_top, **kw):
    X, y, S, J, rel = _data(L, name)
    ws, wp, wbest = pairscan_np.expected(J, rel, score, n_top)
    grel, gs, gp, gbest = L.pair_screen("gpu", X, y, S, n_top=n_top, score=score, **kw)
    assert np.array_equal(grel, rel)
    assert np.array_equal(gs, ws), (name, score, n_top)
    assert np.array_equal(gp, wp), (name, score, n_top)
    assert np.array_equal(gbest, wbest), (name, score, n_top)
    return gs, gp


@pytest.mark.parametrize("name", sorted(n for n in SHAPES if n != "route_p67"))
def test_list_equals_jmi_rows(L, name):
    X, y, S, J, rel = _data(L, name)
    p = X.shape[1]
    total = p * (p - 1) // 2
    assert np.array_equal(J, J.T)
    assert np.array_equal(rel, L.mi_matrices("gpu", X, y, S)[0])
    for score in SCORES:
        for n_top in sorted({1, min(7, total), total, total + 5}):
            _check(L, name, score, n_top)
    # without feature_best: the same list
    a = L.pair_screen("gpu", X, y, S, n_top=total, want_feature_best=False)
    b = L.pair_screen("gpu", X, y, S, n_top=total)
    assert a[3] is None and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    timing = L.pair_screen_last_timing()
    assert len(timing) == 5 and all(t >= 0.0 for t in timing)
    if name in ("one_class", "all_constant"):
        assert not b[1].any() and not b[3].any()
        i, j = np.triu_indices(p, 1)
        assert np.array_equal(b[2], np.stack([i, j], axis=1))
    if name == "constant_pair":
        assert J[1, 3] == 0.0
    if name == "tied":
        assert J[0, 2] == J[0, 5] == J[0, 6]


# ---- routes ------------------------------------------------------------------
def tile_pairs(p, T):
    """The pairs i < j < p of every tile of the upper triangle, in tile order."""
    nb = -(-p // T)
    out = []
    for bi in range(nb):
        for bj in range(bi, nb):
            ri = min(T, p - bi * T)
            rj = min(T, p - bj * T)
            out.append(ri * (ri - 1) // 2 if bi == bj else ri * rj)
    return out


def first_launches(p, T, n_top, pair_tiles=0, pair_cap=0):
    """The launches up to the one that fills the list, as (first tile, tiles,
    overflows): before the list is full every pair of a launch is a candidate,
    so sizes and overflows follow from the hook values alone."""
    pairs = tile_pairs(p, T)
    cap = max(pair_cap if pair_cap > 0 else max(16384, 8 * n_top), THREADS)
    out, held, t0 = [], 0, 0
    while t0 < len(pairs) and held < n_top:
        per = min(pair_tiles if pair_tiles > 0 else cap // (T * T), len(pairs) - t0)
        todo = [(t0, per)]
        while todo:
            b0, cnt = todo.pop()
            over = sum(pairs[b0:b0 + cnt]) > cap
            out.append((b0, cnt, over))
            if over:
                todo += [(b0 + cnt // 2, cnt - cnt // 2), (b0, cnt // 2)]
            else:
                held += sum(pairs[b0:b0 + cnt])
        t0 += per
    return out, t0, len(pairs)


ROUTE_P, ROUTE_T = 67, 16


def test_route_one_launch(L):
    """The unhooked call: all 15 tiles in the first launch."""
    runs, done, tiles = first_launches(ROUTE_P, ROUTE_T, 100)
    assert tiles == 15 and runs == [(0, 15, False)] and done == tiles
    for score in SCORES:
        _check(L, "route_p67", score, 100)


@pytest.mark.parametrize("n_top", [1, 100, 2211 + 5])
@pytest.mark.parametrize("hooks", [{"pair_tiles": 1}, {"pair_tiles": 4}, {"pair_cap": 64},
                                   {"pair_tiles": 4, "pair_cap": 64}],
                         ids=["tiles1", "tiles4", "cap64", "tiles4_cap64"])
def test_routes(L, hooks, n_top):
    X, y, S, J, rel = _data(L, "route_p67")
    assert X.shape[1] == ROUTE_P and mi_np.tile(S) == ROUTE_T
    runs, done, tiles = first_launches(ROUTE_P, ROUTE_T, n_top, **hooks)
    assert tiles == 15
    if hooks == {"pair_tiles": 1}:
        assert [r[:2] for r in runs] == [(t, 1) for t in range(len(runs))]
        assert not any(r[2] for r in runs)
    elif hooks == {"pair_tiles": 4}:
        assert runs[0] == (0, 4, False)
        if n_top > 2211:
            assert [r[:2] for r in runs] == [(0, 4), (4, 4), (8, 4), (12, 3)]
    elif hooks == {"pair_cap": 64}:
        # a buffer of one tile: one tile a launch while every pair is admitted
        assert all(r[1] == 1 and not r[2] for r in runs)
    else:
        # 4 tiles (120 + 3 * 256 pairs) and then 2 (376) overflow 256 entries
        assert runs[:3] == [(0, 4, True), (0, 2, True), (0, 1, False)]
    if n_top <= 100:
        # the list is full after the first tile's 120 pairs: every later launch
        # runs under a threshold, which the later merges raise
        assert done < tiles and sum(tile_pairs(ROUTE_P, ROUTE_T)[:1]) >= n_top
    else:
        assert done == tiles     # never full: every launch admits every pair
    for score in SCORES:
        want = L.pair_screen("gpu", X, y, S, n_top=n_top, score=score)
        with L.test_hooks(**hooks):
            got = L.pair_screen("gpu", X, y, S, n_top=n_top, score=score)
            _check(L, "route_p67", score, n_top)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_route_product_sizes_with_a_threshold(L):
    """p = 1100 at 3 states: 69 blocks, 2415 tiles.  The first launch takes the
    64 tiles whose 16384 pairs at most fit the buffer and fills a list of 100;
    the rest runs under its threshold.  Checked against the all-anchors route."""
    p, n_top = 1100, 100
    runs, done, tiles = first_launches(p, 16, n_top)
    assert tiles == 2415 and runs == [(0, 64, False)] and done == 64
    X, y = mi_np.uniform(65, p, 3, 511, 2)
    J = L.jmi_rows("gpu", X, y, 3, np.arange(p))
    for score in SCORES:
        rel, gs, gp, gbest = L.pair_screen("gpu", X, y, 3, n_top=n_top, score=score)
        ws, wp, wbest = pairscan_np.expected(J, rel, score, n_top)
        assert np.array_equal(gs, ws) and np.array_equal(gp, wp)
        assert np.array_equal(gbest, wbest)
        with L.test_hooks(pair_tiles=700):
            again = L.pair_screen("gpu", X, y, 3, n_top=n_top, score=score)
        assert np.array_equal(again[1], gs) and np.array_equal(again[2], gp)
        assert np.array_equal(again[3], gbest)


# ---- against the CPU backend -------------------------------------------------
CPU_CASES = ["s3_c2_p33", "s3_c4_p17", "s5_c2_p17", "s10_c2_p6", "s32_c4_p5", "mixed_c4", "n4097",
             "tied", "route_p67"]


@pytest.mark.parametrize("name", CPU_CASES)
def test_against_the_cpu_backend(L, name):
    X, y, S, _, _ = _data(L, name)
    p = X.shape[1]
    total = p * (p - 1) // 2
    for score in SCORES:
        grel, gs, gp, gbest = L.pair_screen("gpu", X, y, S, n_top=total, score=score)
        crel, cs, cp, cbest = L.pair_screen("cpu", X, y, S, n_top=total, score=score)
        print(name, score, "scores", np.abs(gs - cs).max(), "best", np.abs(gbest - cbest).max())
        assert np.abs(grel - crel).max() <= TOL
        assert np.abs(gs - cs).max() <= TOL
        assert np.abs(gbest - cbest).max() <= TOL
        gap = np.abs(np.diff(cs))
        clear = np.concatenate(([True], gap > 2 * TOL)) & np.concatenate((gap > 2 * TOL, [True]))
        assert np.array_equal(gp[clear], cp[clear])


@pytest.mark.parametrize("case", pairscan_np.PLANTED)
def test_planted_pairs(L, case):
    from fastselect_amd import PairScreen
    from fastselect_amd import mutual_information as mi
    (n, p, seed, a, b, states), j_top, j_next, _ = case
    X, y = pairscan_np.pure(n, p, seed, a, b, states)
    lo, hi = min(a, b), max(a, b)
    for score in SCORES:
        g = L.pair_screen("gpu", X, y, states, n_top=3, score=score)
        c = L.pair_screen("cpu", X, y, states, n_top=3, score=score)
        assert g[2][0].tolist() == [lo, hi] == c[2][0].tolist()
        assert np.abs(g[1] - c[1]).max() <= TOL
        assert g[1][0] - g[1][1] > 0.4          # far from any tie
    est = PairScreen(n_features_to_select=2, backend="gpu").fit(X, y)
    auto = PairScreen(n_features_to_select=2).fit(X, y)
    assert est.effective_backend_ == "gpu" and auto.effective_backend_ == "gpu"
    assert set(est.top_features_.tolist()) == {a, b}
    assert np.array_equal(auto.top_pairs_, est.top_pairs_)
    pairs, sc, _, _ = mi.rank_pair_interactions(X, y, backend="gpu")
    assert np.array_equal(pairs, est.top_pairs_) and np.array_equal(sc, est.top_scores_)


def test_rejections(L):
    from fastselect_amd import PairScreen
    from fastselect_amd import mutual_information as mi
    X, y = mi_np.uniform(64, 5, 3, 42, 2)
    X = X.copy()
    X[63, 4] = 3
    with pytest.raises(ValueError, match=">= n_states"):
        L.pair_screen("gpu", X, y, 3)
    X[63, 4] = 0
    yb = y.copy()
    yb[10] = 3
    with pytest.raises(ValueError, match=">= n_states"):
        L.pair_screen("gpu", X, yb, 3)
    X[5, 1] = 200
    with pytest.raises(ValueError, match=">= n_states"):
        L.pair_screen("gpu", X, y, 3)
    X5, y5 = mi_np.uniform(120, 4, 5, 34, 5)
    with pytest.raises(ValueError, match="4 classes"):
        L.pair_screen("gpu", X5, y5, 5)
    with pytest.raises(RuntimeError, match="classes"):
        PairScreen(2, backend="gpu").fit(X5, y5)
    with pytest.raises(RuntimeError, match="classes"):
        mi.rank_pair_interactions(X5, y5, backend="gpu")
    assert PairScreen(2).fit(X5, y5).effective_backend_ == "cpu"
    X33, y33 = mi_np.uniform(90, 3, 33, 33, 2)
    with pytest.raises(ValueError, match="32 states"):
        L.pair_screen("gpu", X33, y33, 33)
    X33 = X33.copy()
    X33[:33, 0] = np.arange(33)              # one column takes all 33 values
    assert PairScreen(2).fit(X33, y33).effective_backend_ == "cpu"
    # the device still answers
    Xo, yo = mi_np.uniform(64, 5, 3, 42, 2)
    g = L.pair_screen("gpu", Xo, yo, 3, n_top=10)
    c = L.pair_screen("cpu", Xo, yo, 3, n_top=10)
    assert np.abs(g[1] - c[1]).max() <= TOL


def test_planes_that_cannot_be_allocated_are_out_of_memory(L):
    """2^31 - 1 samples x 2^20 columns: planes of 2^50 bytes.  The out-of-memory
    code on the size alone, before any array is read (the arrays are tiny)."""
    import ctypes
    lib = L.lib()
    u8p, f64p, i64p = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_double, ctypes.c_int64))
    x = np.zeros(16, np.uint8)
    r = np.zeros(4)
    t = np.zeros(4, np.int64)
    rc = lib.fs_pair_screen(L.BACKEND_GPU, 0, x.ctypes.data_as(u8p), x.ctypes.data_as(u8p),
                            2 ** 31 - 1, 1 << 20, 3, 0, 1, 4, 1, r.ctypes.data_as(f64p),
                            r.ctypes.data_as(f64p), t.ctypes.data_as(i64p),
                            t.ctypes.data_as(i64p), None)
    assert rc == L.FS_EOOM
