"""Pass 2 of the CPU backend, bit for bit, on grid data with caller-chosen
near / far decisions (tests/pass2_np.py explains why equality is owed).

Each run hands fs_plan_select a crafted rowstats vector (one threshold per
row) and fs_plan_pass2 crafted power-of-two counts, then asserts
``array_equal`` on the near counts select returns and on the float64 sums
pass 2 returns against the numpy restatement.  This pins the harness that
tests/test_gpu_pass2_exact.py runs on the GPU, and covers fs_cpu.cpp.
"""
import functools

import numpy as np
import pytest

import pass2_np as R

# n, p, trailing discrete columns, classes
SHAPES = [
    pytest.param(300, 40, 0, 2, id="n300-p40"),
    pytest.param(257, 70, 6, 3, id="n257-p70-d6-3cls"),
    pytest.param(130, 520, 20, 2, id="n130-p520-d20"),
    pytest.param(65, 8, 0, 2, id="n65-p8"),
]


@functools.lru_cache(maxsize=None)
def _case(n, p, nd, classes):
    pairs = tuple(R.slot_pairs(n))
    X, y, isd, recip = R.grid_data(n, p, nd, seed=n + p, classes=classes, pairs=pairs)
    D = R.distances(X, isd)
    return X, y, isd, recip, D, R.patterns(D, n, pairs)


def _plan(case, star, rank=0, world=1):
    from fastselect_amd import _lib
    X, y, isd, recip = case[:4]
    plan = _lib.Plan("cpu", X, y.astype(np.float64), recip, isd, use_star=star, rank=rank,
                     world=world)
    bufs = R.HostBufs(*X.shape)
    plan.pass1(bufs.ptr("rs"))  # the distances; its row moments are not used
    return plan, bufs, plan.calibration()["SC"]


def _check(name, got, want, bad):
    if not np.array_equal(got, want):
        k = np.flatnonzero(np.asarray(got) != np.asarray(want))
        bad.append(f"{name}: {k.size} differ, first at {k[0]}: {np.asarray(got)[k[0]]!r} != "
                   f"{np.asarray(want)[k[0]]!r}")


def test_restatement_agrees_with_the_definition():
    """The matrix-product forms of pass2_np against an n x n x p array."""
    for n, p, nd in ((65, 8, 0), (130, 30, 6), (40, 12, 12)):
        X, y, isd, _ = R.grid_data(n, p, nd, seed=1, pairs=R.slot_pairs(n))
        D = R.distances(X, isd)
        assert np.array_equal(D, R.distances_direct(X, isd))
        H, M = R.counts_pow2(n, tiny=True)
        for star in (False, True):
            e = R.expected(X, y, isd, R.patterns(D, n)["q40"], H, M, star, D=D)
            assert np.array_equal(e["sums"], R.weighted_sums_direct(X, isd, e["W32"]))
            assert e["weighted"] > 0 and np.any(e["sums"] != 0)


def test_slot_pairs_cover_the_weight_block():
    slots = [R.slot_of(i, j) for i, j in R.slot_pairs(700)]
    assert {s[3] for s in slots} >= {0, 63} and {s[2] for s in slots} == {0, 1}
    assert {s[4] for s in slots} >= {0, 15} and {s[5] for s in slots} >= {0, 7}
    assert any(s[0] == s[1] for s in slots) and any(s[0] != s[1] for s in slots)
    assert any(s[0] == s[1] == 5 for s in slots)  # the partial last row block


def test_feature_blocks_restate_the_layout():
    """The layouts the GPU tests rely on: which blocks are mixed."""
    assert R.feature_blocks(600, 100) == dict(
        PC=512, PW=640, sparse=[(8, "cont"), (4, "disc")],
        dense=["cont"] * 4 + ["disc"])
    assert R.feature_blocks(900, 200) == dict(
        PC=704, PW=960, sparse=[(8, "cont"), (8, "mixed")],
        dense=["cont"] * 5 + ["mixed", "disc", "disc"])
    assert R.feature_blocks(100, 40) == dict(PC=64, PW=128, sparse=[(4, "mixed")],
                                             dense=["mixed"])


@pytest.mark.parametrize("tiny", [False, True], ids=["pow2", "tinyH"])
@pytest.mark.parametrize("n,p,nd,classes", SHAPES)
@pytest.mark.parametrize("star", [False, True], ids=["multisurf", "star"])
def test_every_pattern_is_exact(star, n, p, nd, classes, tiny):
    case = _case(n, p, nd, classes)
    X, y, isd, _, D, pats = case
    H, M = R.counts_pow2(n, tiny)
    plan, bufs, SC = _plan(case, star)
    bad = []
    try:
        for name, thr in pats.items():
            e = R.expected(X, y, isd, thr, H, M, star, D=D)
            R.check_exactness(X, isd, D, thr, H, M, e["W32"])
            sel, sums = R.select_and_score(plan, bufs, thr, R.pack_counts(H, M), SC)
            assert plan.info()[2] == 0, f"{name}: refined pairs"
            _check(f"{name} hits", sel[:, 0], e["hits"], bad)
            _check(f"{name} misses", sel[:, 1], e["misses"], bad)
            _check(f"{name} sums", sums, e["sums"], bad)
            if name == "none" and not star:
                assert not np.any(sums != 0) and not np.any(np.signbit(sums))
    finally:
        plan.close()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("star", [False, True], ids=["multisurf", "star"])
def test_set_rows_parts_are_exact_and_add_up(star):
    case = _case(300, 40, 0, 2)
    X, y, isd, _, D, pats = case
    n = len(X)
    H, M = R.counts_pow2(n)
    plan, bufs, SC = _plan(case, star)
    try:
        for name in ("q40", "all", "row(64)"):
            thr = pats[name]
            total = np.zeros(X.shape[1])
            for rows in ((0, 64), (64, 200), (200, n)):
                plan.set_rows(*rows)
                e = R.expected(X, y, isd, thr, H, M, star, rows=rows, D=D)
                _, sums = R.select_and_score(plan, bufs, thr, R.pack_counts(H, M), SC)
                assert np.array_equal(sums, e["sums"]), (name, rows)
                total += sums
            whole = R.expected(X, y, isd, thr, H, M, star, D=D)["sums"]
            assert np.array_equal(total, whole), name
    finally:
        plan.close()


@pytest.mark.parametrize("star", [False, True], ids=["multisurf", "star"])
def test_two_ranks_add_up_exactly(star):
    case = _case(257, 70, 6, 3)
    X, y, isd, _, D, pats = case
    n = len(X)
    H, M = R.counts_pow2(n, tiny=True)
    ranks = [_plan(case, star, rank=r, world=2) for r in range(2)]
    try:
        for name in ("q40", "even", "all"):
            thr = pats[name]
            e = R.expected(X, y, isd, thr, H, M, star, D=D)
            got = [R.select_and_score(pl, b, thr, R.pack_counts(H, M), SC) for pl, b, SC in ranks]
            assert np.any(got[0][1] != 0) and np.any(got[1][1] != 0)
            assert np.array_equal(got[0][0][:, 0] + got[1][0][:, 0], e["hits"]), name
            assert np.array_equal(got[0][0][:, 1] + got[1][0][:, 1], e["misses"]), name
            assert np.array_equal(got[0][1] + got[1][1], e["sums"]), name
    finally:
        for pl, _, _ in ranks:
            pl.close()


@pytest.mark.parametrize("star", [False, True], ids=["surf", "surf-star"])
def test_surf_is_exact(star):
    """SURF's weights are +-1 and +-2: its sums are exact too; the thresholds
    are the row means the restatement computes (surf_expected)."""
    from fastselect_amd import _lib
    n, p = 257, 70
    X, y, isd, recip = R.grid_data(n, p, 6, seed=3)
    D = R.distances(X, isd)
    for rows in (None, (64, 200)):
        e = R.surf_expected(X, y, isd, star, rows=rows, D=D)
        plan = _lib.RowsPlan("cpu", "surf", X.astype(np.float64), y.astype(np.int32), recip, isd,
                             use_star=star, rows=rows)
        try:
            sums = np.full(p, np.nan)
            plan.score(sums.ctypes.data)
        finally:
            plan.close()
        assert np.any(e["sums"] != 0)
        assert np.array_equal(sums, e["sums"]), rows
