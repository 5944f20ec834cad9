"""Pass 2 on the GPU, bit for bit, on grid data with caller-chosen near / far
decisions (tests/pass2_np.py explains why equality is owed; the CPU
counterpart is tests/test_pass2_exact.py).

Every route of pass 2 -- k_weights_sparse3 + k_score_sparse3 with the
generated segment statement, the same with the plain-HIP walk, the dense
k_weights + k_score, and the sparse route under several segment lengths --
must return the numpy float64 sums exactly, so the routes also equal each
other exactly.  A test builds one plan and runs one pass 1, then one select
and one pass 2 per threshold pattern: the near counts of select, the sums of
pass 2 and (MultiSURF, sparse routes) fs_plan_weighted_pairs are compared
with ``array_equal`` / ``==``.
"""
import time

import numpy as np
import pytest

import pass2_np as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    from fastselect_amd import _lib
    assert _lib.device_count() >= 1, "no HIP device visible: GPU tests cannot run"
    yield
    # the n = 8200 matrices
    for cache in (_data_cache, _want_cache, _surf_data_cache, _surf_want_cache):
        cache.clear()


# (n, p, trailing discrete columns), and what tests/pass2_np.py::feature_blocks
# must say of the shape's sparse blocks (test_shapes_have_their_layouts)
SHAPES = {
    # one diagonal tile; half 1 holds a single real row; only the F = 4 block
    "n65-p8": ((65, 8, 0), [(4, "cont")]),
    # three row blocks, the last with one row; one F = 8 block plus the F = 4 tail
    "n257-p520": ((257, 520, 0), [(8, "cont"), (4, "cont")]),
    # a partial F = 8 block: lanes past PW, slack reads
    "n192-p800": ((192, 800, 0), [(8, "cont"), (8, "cont")]),
    # PC = 512: a continuous F = 8 block on the statement (12 padding columns)
    # beside an all-discrete F = 4 tail on the C++ loop; no block is mixed
    "n257-p600-d100": ((257, 600, 100), [(8, "cont"), (4, "disc")]),
    # PC = 704: block 0 on the statement, block 1 (512..959) mixed on the C++
    # loop -- lanes 0..47 of its first chunk continuous, the rest and the
    # second chunk discrete; the dense route is mixed at f0 = 640
    "n257-p900-d200": ((257, 900, 200), [(8, "cont"), (8, "mixed")]),
    # PC = 64 of PW = 128: a mixed F = 4 block, and the only dense block mixed
    "n257-p100-d40": ((257, 100, 40), [(4, "mixed")]),
    # all-discrete blocks
    "n140-p520-discrete": ((140, 520, 520), [(8, "disc"), (4, "disc")]),
    # six row blocks: segments of several tiles
    "n700-p520": ((700, 520, 0), [(8, "cont"), (4, "cont")]),
    # 65 column blocks: row block 0 has 65 tiles, a segment of 64 plus one of 1
    "n8200-p8": ((8200, 8, 0), [(4, "cont")]),
}
MIXED = ("n257-p900-d200", "n257-p100-d40")
BIG = "n8200-p8"
BIG_PATTERNS = ("all", "q40", "row(0)")
TINY_PATTERNS = ("all", "q40", "even", "row(63)")

# hooks set before the plan is created
ROUTES = {
    "sparse": dict(sparse=1),
    "generic": dict(sparse=1, pass2_generic=1),
    "dense": dict(sparse=0),
    "seg1": dict(sparse=1, seg_len=1),
    "seg3": dict(sparse=1, seg_len=3),
    "seg4": dict(sparse=1, seg_len=4),
    "seg100": dict(sparse=1, seg_len=100),
}
MODES = {"multisurf": (False, {}), "star-dense": (True, dict(star_split=0)),
         "star-split": (True, dict(star_split=1))}


def _routes(shape):
    """Every mode of a shape runs the same routes.  seg_len is the number of
    column blocks a segment of the sparse schedule may span
    (build_sparse_schedule), so with nb row blocks every seg_len >= nb gives
    the schedule of seg_len = nb, and the default at these sizes is 1
    (shard_segments; 5 at n = 8200).  One row block has no seg_len route; with
    two or three, seg3 and seg4 are run and put a row block's tiles in one
    segment, seg1 would repeat "sparse" and seg100 would repeat seg4; from six
    row blocks on all four differ and all four are run."""
    n = SHAPES[shape][0][0]
    nb = (n + R.TILE - 1) // R.TILE
    names = ["sparse", "generic", "dense"]
    if nb >= 2:
        names += ["seg3", "seg4"]
    if nb >= 6:
        names += ["seg1", "seg100"]
    return names


# MultiSURF* at n = 8200 is left out: what the shape adds is 65 column blocks
# (a capped segment of 64 tiles plus one of 1), which is the walk's and the
# reduction's business and the same for any weights, while a second float64
# restatement of 8200 x 8200 pairs would double the seconds the first case of
# that shape already takes.  The star modes run every route, all four seg_len
# among them, on the six-row-block shape.
CASES = [pytest.param(s, m, r, id=f"{s}-{m}-{r}")
         for s in SHAPES for m in MODES if not (s == BIG and m != "multisurf")
         for r in _routes(s)]


def test_shapes_have_their_layouts():
    """numpy only: each shape's feature blocks are what its comment claims,
    the mixed ones included (sparse: a block with continuous and discrete
    lanes on the C++ loop; dense: score_tiles<false, true, true>)."""
    for shape, ((n, p, nd), blocks) in SHAPES.items():
        lay = R.feature_blocks(p, nd)
        assert lay["sparse"] == blocks, (shape, lay)
        assert ("mixed" in lay["dense"]) == (shape in MIXED), (shape, lay)
    for shape in MIXED:
        n, p, nd = SHAPES[shape][0]
        lay = R.feature_blocks(p, nd)
        assert 0 < lay["PC"] < lay["PW"] and lay["PC"] % 128 != 0 and lay["PC"] % 256 != 0
    lay = R.feature_blocks(900, 200)
    assert lay["PC"] == 704 and lay["PC"] % 512 != 0 and lay["dense"][5] == "mixed"

_data_cache, _want_cache = {}, {}


def _case(shape):
    if shape not in _data_cache:
        n, p, nd = SHAPES[shape][0]
        pairs = tuple(R.slot_pairs(n))
        X, y, isd, recip = R.grid_data(n, p, nd, seed=n + p, pairs=pairs)
        D = R.distances(X, isd)
        pats = R.patterns(D, n, pairs)
        if shape == BIG:
            pats = {k: pats[k] for k in BIG_PATTERNS}
        _data_cache[shape] = (X, y, isd, recip, D, pats)
    return _data_cache[shape]


def _want(shape, name, star, tiny=False, rows=None):
    """The restatement of one (shape, pattern): computed once, with its
    preconditions checked, and shared by every route (matrices dropped)."""
    key = (shape, name, star, tiny, rows)
    if key not in _want_cache:
        X, y, isd, _, D, pats = _case(shape)
        H, M = R.counts_pow2(len(X), tiny)
        e = R.expected(X, y, isd, pats[name], H, M, star, rows=rows, D=D)
        R.check_exactness(X, isd, D, pats[name], H, M, e["W32"])
        _want_cache[key] = {k: e[k] for k in ("hits", "misses", "weighted", "sums")}
    return _want_cache[key]


def _plan(shape, star, rank=0, world=1):
    from fastselect_amd import _lib
    X, y, isd, recip = _case(shape)[:4]
    plan = _lib.Plan("gpu", X, y.astype(np.float64), recip, isd, use_star=star, rank=rank,
                     world=world)
    return plan, R.DevBufs(*X.shape)


def _pass1(plan, bufs):
    plan.pass1(bufs.ptr("rs"))  # the distances; its row moments are not used
    bufs.sync()
    cal = plan.calibration()
    assert not cal["q16"]
    return cal["SC"]


def _step(plan, bufs, shape, name, SC, tiny=False):
    n = bufs.n
    thr = _case(shape)[5][name]
    return R.select_and_score(plan, bufs, thr, R.pack_counts(*R.counts_pow2(n, tiny)), SC)


def _differ(label, got, want, bad):
    got, want = np.asarray(got), np.asarray(want)
    if not np.array_equal(got, want):
        k = np.flatnonzero(got != want)
        bad.append(f"{label}: {k.size} differ, first at {k[0]}: {got[k[0]]!r} != {want[k[0]]!r}")


@pytest.mark.parametrize("shape,mode,route", CASES)
def test_route_equals_numpy(hooks, shape, mode, route):
    star, mode_hooks = MODES[mode]
    for k, v in {**ROUTES[route], **mode_hooks}.items():
        hooks(k, v)
    t0 = time.perf_counter()
    pats = _case(shape)[5]
    # a stale weight slot would show in the first three; the rest in any order
    order = [k for k in ("all", "none", "row(63)", "row(0)") if k in pats]
    order += [k for k in pats if k not in order]
    counted = not star and ROUTES[route]["sparse"] == 1
    plan, bufs = _plan(shape, star)
    bad, refined = [], 0
    try:
        SC = _pass1(plan, bufs)
        for name in order:
            for tiny in (False, True) if name in TINY_PATTERNS and shape != BIG else (False,):
                want = _want(shape, name, star, tiny)
                sel, sums = _step(plan, bufs, shape, name, SC, tiny)
                refined += plan.info()[2]
                label = f"{name}{' tinyH' if tiny else ''}"
                _differ(f"{label} hits", sel[:, 0], want["hits"], bad)
                _differ(f"{label} misses", sel[:, 1], want["misses"], bad)
                _differ(f"{label} sums", sums, want["sums"], bad)
                if counted and plan.weighted_pairs() != want["weighted"]:
                    bad.append(f"{label}: weighted_pairs {plan.weighted_pairs()} != "
                               f"{want['weighted']}")
                if name == "none" and not star:
                    if np.any(sums != 0) or np.any(np.signbit(sums)):
                        bad.append("none: a score that is not +0.0")
                if name == "q40" and not tiny:  # a second step of the same pattern
                    _differ("q40 again", _step(plan, bufs, shape, name, SC)[1], sums, bad)
    finally:
        plan.close()
    print(f"{shape} {mode} {route}: {len(order)} patterns, {refined} refined pairs, "
          f"{time.perf_counter() - t0:.2f} s")
    assert not bad, "\n".join(bad)


SPLIT_PATTERNS = ("q40", "even", "all")


@pytest.mark.parametrize("mode", list(MODES))
def test_tile_shards_add_up(hooks, mode):
    """set_shard(r, 3) over the three shards of one plan: the near counts and
    the sums add up to the whole exactly."""
    shape = "n257-p520"
    star, mode_hooks = MODES[mode]
    for k, v in {"sparse": 1, **mode_hooks}.items():
        hooks(k, v)
    plan, bufs = _plan(shape, star)
    got = {k: [] for k in SPLIT_PATTERNS}
    try:
        for r in range(3):
            plan.set_shard(r, 3)
            SC = _pass1(plan, bufs)
            for name in SPLIT_PATTERNS:
                got[name].append(_step(plan, bufs, shape, name, SC, tiny=True))
    finally:
        plan.close()
    for name, parts in got.items():
        want = _want(shape, name, star, True)
        assert all(np.any(s != 0) for _, s in parts)
        assert np.array_equal(sum(c[:, 0] for c, _ in parts), want["hits"]), name
        assert np.array_equal(sum(c[:, 1] for c, _ in parts), want["misses"]), name
        assert np.array_equal(sum(s for _, s in parts), want["sums"]), name


@pytest.mark.parametrize("mode", list(MODES))
def test_two_ranks_add_up(hooks, mode):
    shape = "n257-p900-d200"
    star, mode_hooks = MODES[mode]
    for k, v in {"sparse": 1, **mode_hooks}.items():
        hooks(k, v)
    got = {k: [] for k in SPLIT_PATTERNS}
    for r in range(2):
        plan, bufs = _plan(shape, star, rank=r, world=2)
        try:
            SC = _pass1(plan, bufs)
            for name in SPLIT_PATTERNS:
                got[name].append(_step(plan, bufs, shape, name, SC))
        finally:
            plan.close()
    for name, parts in got.items():
        want = _want(shape, name, star)
        assert all(np.any(s != 0) for _, s in parts)
        assert np.array_equal(parts[0][0][:, 0] + parts[1][0][:, 0], want["hits"]), name
        assert np.array_equal(parts[0][0][:, 1] + parts[1][0][:, 1], want["misses"]), name
        assert np.array_equal(parts[0][1] + parts[1][1], want["sums"]), name


@pytest.mark.parametrize("route", ["sparse", "dense"])
@pytest.mark.parametrize("mode", list(MODES))
def test_set_rows_parts_are_exact_and_add_up(hooks, mode, route):
    shape = "n257-p520"
    star, mode_hooks = MODES[mode]
    for k, v in {**ROUTES[route], **mode_hooks}.items():
        hooks(k, v)
    n = SHAPES[shape][0][0]
    plan, bufs = _plan(shape, star)
    bad = []
    try:
        SC = _pass1(plan, bufs)
        for name in SPLIT_PATTERNS + ("row(64)",):
            total = np.zeros(bufs.p)
            for rows in ((0, 64), (64, 200), (200, n)):
                plan.set_rows(*rows)
                want = _want(shape, name, star, rows=rows)
                sums = _step(plan, bufs, shape, name, SC)[1]
                _differ(f"{name} rows {rows}", sums, want["sums"], bad)
                if not star and route == "sparse" and plan.weighted_pairs() != want["weighted"]:
                    bad.append(f"{name} rows {rows}: weighted_pairs")
                total += sums
            _differ(f"{name} parts", total, _want(shape, name, star)["sums"], bad)
    finally:
        plan.close()
    assert not bad, "\n".join(bad)


# ---- SURF / SURF* ---------------------------------------------------------------

# seeds at which no distance lies within SURF_MARGIN of its row's mean
# (surf_expected asserts it)
SURF_SHAPES = {"n257-p520": (257, 520, 4), "n700-p520": (700, 520, 1202)}
SURF_ROUTES = {
    "sparse": dict(sparse=1),
    "generic": dict(sparse=1, pass2_generic=1),
    "dense": dict(sparse=0),
    "seg4": dict(sparse=1, seg_len=4),
    "f64": dict(sparse=1, surf_f64=1),
    "int": dict(sparse=1, surf_f64=0),
    "dense-int": dict(sparse=0, surf_f64=0),
}
_surf_data_cache, _surf_want_cache = {}, {}


def _surf_case(shape):
    if shape not in _surf_data_cache:
        n, p, seed = SURF_SHAPES[shape]
        X, y, isd, recip = R.grid_data(n, p, 0, seed=seed)
        _surf_data_cache[shape] = (X.astype(np.float64), y.astype(np.int32), isd, recip,
                                   R.distances(X, isd))
    return _surf_data_cache[shape]


def _surf_want(shape, star, rows):
    key = (shape, star, rows)
    if key not in _surf_want_cache:
        X, y, isd, _, D = _surf_case(shape)
        e = R.surf_expected(X, y, isd, star, rows=rows, D=D)
        assert np.any(e["sums"] != 0)
        _surf_want_cache[key] = e["sums"]
    return _surf_want_cache[key]


@pytest.mark.parametrize("route", list(SURF_ROUTES))
@pytest.mark.parametrize("star", [False, True], ids=["surf", "surf-star"])
@pytest.mark.parametrize("shape", list(SURF_SHAPES))
def test_surf_route_equals_numpy(hooks, shape, star, route):
    import torch

    from fastselect_amd import _lib
    for k, v in SURF_ROUTES[route].items():
        hooks(k, v)
    bad = []
    for rows in (None, (64, 200)):
        X, y, isd, recip, _ = _surf_case(shape)
        want = _surf_want(shape, star, rows)
        plan = _lib.RowsPlan("gpu", "surf", X, y, recip, isd, use_star=star, rows=rows)
        try:
            sums = torch.full((X.shape[1],), float("nan"), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            plan.score(sums.data_ptr())
            torch.cuda.synchronize()
            if "surf_f64" in SURF_ROUTES[route]:
                assert plan.calibration()["surf_f64"] == bool(SURF_ROUTES[route]["surf_f64"])
        finally:
            plan.close()
        _differ(f"rows {rows}", sums.cpu().numpy(), want, bad)
    assert not bad, "\n".join(bad)
