"""RReliefF on the CPU backend and at the ABI (cpu::rrelieff_sums,
fs_plan_score_targets, fs_rrelieff_scores, fs_rrelieff_score, the RReliefF
estimator) against the float64 numpy model (rrelieff_np.py).

The CPU backend sums the reference's float32 diffs (widened to float64) times
the float64 dy over the plan's neighbour lists; the model sums the same terms
in another order.  A sum has at most n k = 3000 non-negative terms here, so
the two differ by at most 3000 * 1.1e-16 = 3.3e-13 relative: the bar is 1e-12,
for the order alone, and W is held to that bar propagated through the
epilogue (rrelieff_np.w_tolerance) plus the library's one float32 rounding of
W (2^-24 |W|).  Row ranges regroup the plan's own terms and are held to the
same 1e-12.
"""
import numpy as np
import pytest

import rrelieff_np as R
import stir_np
import stir_relieff_np as M

from fastselect_amd import RReliefF, TuRF, _lib as L

TOL = 1e-12
N_TARGETS = 17
_CACHE = {}

# name -> (n, continuous columns, discrete columns, k): the shapes of
# tests/test_gpu_stir_relieff.py (the three-class case with its y ignored)
SHAPES = {
    "mixed": (300, 20, 20, 3),
    "n130-p270": (130, 200, 70, 10),
    "discrete-p64": (130, 0, 64, 5),
    "continuous-p64": (130, 64, 0, 1),
    "three-class": (300, 20, 20, 5),
}


def preprocess(x):
    """(recip f32, is_discrete) as RReliefF.fit and ReliefF.fit derive them."""
    return M.preprocess(x, np.zeros(x.shape[0]))[1:3]


def make_targets(x, n_targets=N_TARGETS, seed=7):
    """(n_targets, n) float64: a target planted on two columns, permutations
    of it, plain noise, and one with many equal values (dy = 0 pairs)."""
    rng = np.random.default_rng(seed)
    n, p = x.shape
    t0 = x[:, 0].astype(np.float64) + 0.5 * (x[:, p - 1] > np.median(x[:, p - 1])) \
        + 0.3 * rng.standard_normal(n)
    t = np.empty((n_targets, n))
    t[0] = t0
    for b in range(1, n_targets):
        t[b] = rng.permutation(t0) if b % 2 else 5.0 * rng.standard_normal(n) - 3.0
    t[n_targets - 1] = rng.integers(0, 4, n)
    return t


def plan_targets(backend, x, recip, isd, k, targets, rows=None, feat=None, n_jobs=-1,
                 repeat=False, more=()):
    """One resident one-class plan, one ``score_targets`` call (two with
    ``repeat``).  Returns a dict: s_a (n_kept), s_ca (B, n_kept), s_c (B), m
    (rows * k), sel_ms / upd_ms, again (the second call's triple) and more
    (the triples of further calls on the same plan, one per entry of
    ``more``)."""
    targets = np.atleast_2d(targets)
    pl = L.RowsPlan(backend, "relieff", x, np.zeros(x.shape[0], np.int32), recip, isd, k=k,
                    class_probs=np.ones(1, np.float32), rows=rows, n_jobs=n_jobs)
    try:
        if feat is not None:
            pl.set_features(feat)
        nk = pl.n_kept

        def call(t):
            t = np.atleast_2d(t)
            B = t.shape[0]
            size = nk + B * nk + B
            if backend == "gpu":
                import torch
                buf = torch.empty(size, dtype=torch.float64, device="cuda")
                torch.cuda.synchronize()  # the plan runs on a stream of its own
                p0 = buf.data_ptr()
            else:
                buf = np.zeros(size)
                p0 = buf.ctypes.data
            pl.score_targets(t, p0, p0 + 8 * nk, p0 + 8 * (nk + B * nk))
            h = buf.cpu().numpy() if backend == "gpu" else buf
            return h[:nk].copy(), h[nk:nk + B * nk].reshape(B, nk).copy(), h[nk + B * nk:].copy()

        first = call(targets)
        again = call(targets) if repeat else None
        ms = (pl.targets_kernel_ms(0), pl.targets_kernel_ms(1))
        extra = [call(t) for t in more]
    finally:
        pl.close()
    lo, hi = (0, x.shape[0]) if rows is None else rows
    return {"s_a": first[0], "s_ca": first[1], "s_c": first[2], "m": (hi - lo) * k,
            "sel_ms": ms[0], "upd_ms": ms[1], "again": again, "more": extra}


def rel_err(a, ref):
    return float(np.max(np.abs(a - ref) / np.abs(ref)))


def case(name, oracle):
    """(x, recip, isd, k, targets, model (S_A, S_CA, S_C, M)), once per session."""
    if name not in _CACHE:
        n, pc, pd, k = SHAPES[name]
        x = M.three_class_case()[0] if name == "three-class" else stir_np.mixed_case(n, pc, pd)[0]
        recip, isd = preprocess(x)
        assert int(isd.sum()) == pd
        argsort = oracle.numba_argsort if name == "discrete-p64" else None
        targets = make_targets(x)
        _CACHE[name] = (x, recip, isd, k, targets,
                        R.sums(x, targets, recip, isd, k, argsort=argsort))
    return _CACHE[name]


def whole(name, oracle, backend="cpu"):
    if ("whole", backend, name) not in _CACHE:
        x, recip, isd, k, targets, _ = case(name, oracle)
        _CACHE["whole", backend, name] = plan_targets(backend, x, recip, isd, k, targets,
                                                      repeat=True)
    return _CACHE["whole", backend, name]


def check_against_model(r, model, sum_tol, label):
    m_a, m_ca, m_c, m_m = model
    assert r["m"] == m_m
    assert np.all(m_a > 0) and np.all(m_ca > 0) and np.all(m_c > 0)
    errs = (rel_err(r["s_a"], m_a), rel_err(r["s_ca"], m_ca), rel_err(r["s_c"], m_c))
    print(f"{label}: max relative error of S_A {errs[0]:.3e}, S_CA {errs[1]:.3e}, "
          f"S_C {errs[2]:.3e}")
    assert max(errs) <= sum_tol
    w = L.rrelieff_scores(r["s_a"], r["s_ca"], r["s_c"], r["m"])
    m_w = R.weights(*model)
    assert w.dtype == np.float32 and w.shape == m_w.shape
    tol = R.w_tolerance(m_a, m_ca, m_c, m_m, sum_tol) + 2.0 ** -24 * np.abs(m_w)
    print(f"{label}: max |W - model| / tolerance {np.max(np.abs(w - m_w) / tol):.3e}")
    assert np.all(np.abs(w - m_w) <= tol)


@pytest.mark.parametrize("name", list(SHAPES))
def test_sums_counts_and_w_match_the_model(name, oracle):
    x, recip, isd, k, targets, model = case(name, oracle)
    r = whole(name, oracle)
    assert r["m"] == x.shape[0] * k
    check_against_model(r, model, TOL, name)
    assert (r["sel_ms"], r["upd_ms"]) == (-1.0, -1.0)  # a CPU plan has no kernel time
    for a, b in zip(r["again"], (r["s_a"], r["s_ca"], r["s_c"])):
        assert np.array_equal(a, b)


def test_discrete_case_has_ties_at_the_kth_key(oracle):
    x, recip, isd, k, targets, model = case("discrete-p64", oracle)
    stable = R.sums(x, targets[:1], recip, isd, k)
    assert not np.array_equal(stable[0], model[0]), "no tie at a k-th key: the case checks nothing"


def test_a_case_worked_by_hand():
    """n = 4, p = 1, k = 1.  x = (0, 1, 3, 8), range 8, so the scaled values
    are 0, 1/8, 3/8, 1 (exact in float32) and the nearest neighbours are
    0 -> 1 (d = 1/8), 1 -> 0 (1/8; its other candidate, 3, is 2/8 away),
    3 -> 1 (2/8; 8 is 5/8 away) and 8 -> 3 (5/8): S_A = 9/8, M = 4.
    t = (0, 2, 3, 10), range 10: u = (0, .2, .3, 1), so dy is .2, .2, .1, .7
    over those pairs: S_C = 1.2 and S_CA = (.2 + .2 + .1 * 2 + .7 * 5) / 8 =
    4.1 / 8 = 0.5125.  W = 0.5125 / 1.2 - (1.125 - 0.5125) / (4 - 1.2) =
    0.4270833... - 0.21875 = 0.2083333..."""
    x = np.array([[0.0], [1.0], [3.0], [8.0]], dtype=np.float32)
    t = np.array([0.0, 2.0, 3.0, 10.0])
    recip, isd = np.array([1.0 / 8.0], np.float32), np.zeros(1, bool)
    r = plan_targets("cpu", x, recip, isd, 1, t)
    assert r["m"] == 4
    np.testing.assert_allclose(r["s_a"], [9.0 / 8.0], rtol=1e-15, atol=0)
    np.testing.assert_allclose(r["s_c"], [1.2], rtol=1e-15, atol=0)
    np.testing.assert_allclose(r["s_ca"], [[0.5125]], rtol=1e-15, atol=0)
    w = L.rrelieff_scores(r["s_a"], r["s_ca"], r["s_c"], 4)
    assert w[0, 0] == np.float32(0.5125 / 1.2 - 0.6125 / 2.8)
    assert abs(float(w[0, 0]) - 0.20833333) < 1e-7
    assert np.array_equal(L.rrelieff_score("cpu", x, t, recip, isd, 1), w)


def test_each_row_of_a_batch_has_the_bits_of_its_own_call(oracle):
    x, recip, isd, k, targets, _ = case("mixed", oracle)
    nine = plan_targets("cpu", x, recip, isd, k, targets[:9])
    for b in range(9):
        one = plan_targets("cpu", x, recip, isd, k, targets[b])
        assert np.array_equal(one["s_ca"][0], nine["s_ca"][b]), b
        assert one["s_c"][0] == nine["s_c"][b], b
        assert np.array_equal(one["s_a"], nine["s_a"]), b
    full = whole("mixed", oracle)  # 17 targets: two blocks of the CPU walk
    assert np.array_equal(full["s_ca"][:9], nine["s_ca"])
    assert np.array_equal(full["s_c"][:9], nine["s_c"])
    assert np.array_equal(full["s_a"], nine["s_a"])


def test_thread_count_does_not_change_the_bits(oracle):
    x, recip, isd, k, targets, _ = case("mixed", oracle)
    one = plan_targets("cpu", x, recip, isd, k, targets[:9], n_jobs=1)
    many = plan_targets("cpu", x, recip, isd, k, targets[:9], n_jobs=16)
    for q in ("s_a", "s_ca", "s_c"):
        assert np.array_equal(one[q], many[q]), q


def test_row_ranges_add_up(oracle):
    x, recip, isd, k, targets, _ = case("mixed", oracle)
    ref = whole("mixed", oracle)
    parts = [plan_targets("cpu", x, recip, isd, k, targets, rows=rg)
             for rg in ((0, 100), (100, 300))]
    assert sum(p["m"] for p in parts) == ref["m"]
    for q in ("s_a", "s_ca", "s_c"):
        assert all(np.all(p[q] > 0) for p in parts)
        np.testing.assert_allclose(sum(p[q] for p in parts), ref[q], rtol=TOL, atol=0)
    # a range is the model's range: a pair belongs to its focal sample, and u
    # is scaled by the whole target's range
    m = R.sums(x, targets, recip, isd, k, rows=(0, 100))
    check_against_model(parts[0], m, TOL, "rows [0, 100)")
    e = plan_targets("cpu", x, recip, isd, k, targets, rows=(128, 128))
    assert e["m"] == 0 and not e["s_a"].any() and not e["s_ca"].any() and not e["s_c"].any()


def test_feature_subset_of_both_kinds(oracle):
    x, recip, isd, k, targets, _ = case("mixed", oracle)
    feat = np.array([1, 3, 7, 19, 22, 25, 30, 38])
    assert isd[feat].any() and not isd[feat].all()
    r = plan_targets("cpu", x, recip, isd, k, targets[:3], feat=feat)
    m = R.sums(np.ascontiguousarray(x[:, feat]), targets[:3], recip[feat], isd[feat], k)
    assert r["s_a"].shape == (feat.size,) and r["s_ca"].shape == (3, feat.size)
    check_against_model(r, m, TOL, "subset")


def test_constant_target_gives_zeros(oracle):
    x, recip, isd, k, targets, _ = case("mixed", oracle)
    t = np.stack([np.full(x.shape[0], 4.25), targets[0]])
    r = plan_targets("cpu", x, recip, isd, k, t)
    assert r["s_c"][0] == 0.0 and not r["s_ca"][0].any() and r["s_a"].all()
    w = L.rrelieff_scores(r["s_a"], r["s_ca"], r["s_c"], r["m"])
    assert not w[0].any() and w[1].any()
    # S_C == M: zeros too
    assert not L.rrelieff_scores(r["s_a"], r["s_ca"][1:], [float(r["m"])], r["m"]).any()
    assert not L.rrelieff_score("cpu", x, t[0], recip, isd, k).any()
    est = RReliefF(n_features_to_select=5, n_neighbors=k, backend="cpu").fit(x, t[0])
    assert est.feature_importances_.dtype == np.float32 and not est.feature_importances_.any()
    assert est.top_features_.tolist() == [0, 1, 2, 3, 4] and est.n_features_in_ == 40
    with pytest.raises(ValueError, match="constant"):
        RReliefF(backend="cpu").permutation_test(x, t[0], n_permutations=3)


def refusal_cases(backend, x, recip, isd, k, targets, bufs):
    """Every refusal of fs_plan_score_targets: FS_EINVAL, fs_last_error says
    why, the buffers keep their sentinel.  ``bufs``: (pointers of s_a, s_ca,
    s_c, a callable returning the three buffers' host copies)."""
    pa, pca, pc, snapshot = bufs
    n = x.shape[0]
    lib = L.lib()
    before = [b.copy() for b in snapshot()]
    zero = np.zeros(n, np.int32)
    one = np.ones(1, np.float32)
    t = np.ascontiguousarray(targets[:2])
    tp = t.ctypes.data_as(L._f64p)

    def refused(plan, tptr, B, a, ca, c, match):
        rc = lib.fs_plan_score_targets(plan._h, tptr, B, L._vp(a or None), L._vp(ca or None),
                                       L._vp(c or None))
        assert rc == L.FS_EINVAL, match
        assert match in lib.fs_last_error().decode(), lib.fs_last_error()
        for got, want in zip(snapshot(), before):
            assert np.array_equal(got, want), match

    ok = L.RowsPlan(backend, "relieff", x, zero, recip, isd, k=k, class_probs=one)
    try:
        refused(ok, None, 2, pa, pca, pc, "NULL")
        refused(ok, tp, 2, 0, pca, pc, "NULL")
        refused(ok, tp, 2, pa, 0, pc, "NULL")
        refused(ok, tp, 2, pa, pca, 0, "NULL")
        refused(ok, tp, 0, pa, pca, pc, "B < 1")
        for bad in (np.nan, np.inf, -np.inf):
            tb = t.copy()
            tb[1, n - 1] = bad
            refused(ok, tb.ctypes.data_as(L._f64p), 2, pa, pca, pc, "non-finite")
    finally:
        ok.close()
    assert lib.fs_plan_score_targets(None, tp, 2, L._vp(pa), L._vp(pca), L._vp(pc)) == L.FS_EINVAL
    y2 = (np.arange(n) % 2).astype(np.int32)
    two = L.RowsPlan(backend, "relieff", x, y2, recip, isd, k=k,
                     class_probs=np.array([0.5, 0.5], np.float32))
    try:
        refused(two, tp, 2, pa, pca, pc, "more than one class")
    finally:
        two.close()
    surf = L.RowsPlan(backend, "surf", x.astype(np.float64), y2, recip, isd)
    try:
        refused(surf, tp, 2, pa, pca, pc, "SURF or MultiSURF")
    finally:
        surf.close()
    ms = L.Plan(backend, x, y2.astype(np.float64), recip, isd)
    try:
        refused(ms, tp, 2, pa, pca, pc, "SURF or MultiSURF")
    finally:
        ms.close()
    with L.accumulation("reference"):
        ref = L.RowsPlan(backend, "relieff", x, zero, recip, isd, k=k, class_probs=one)
    try:
        refused(ref, tp, 2, pa, pca, pc, "reference-order")
    finally:
        ref.close()
    for bad_k in (0, n):
        pl = L.RowsPlan(backend, "relieff", x, zero, recip, isd, k=bad_k, class_probs=one)
        try:
            refused(pl, tp, 2, pa, pca, pc, "1 <= k <= n - 1")
        finally:
            pl.close()


def test_refusals(oracle):
    x, recip, isd, k, targets, _ = case("mixed", oracle)
    p = x.shape[1]
    a, ca, c = np.full(p, -7.0), np.full(2 * p, -7.0), np.full(2, -7.0)
    refusal_cases("cpu", x, recip, isd, k, targets,
                  (a.ctypes.data, ca.ctypes.data, c.ctypes.data, lambda: (a, ca, c)))
    lib = L.lib()
    out = np.full(p, -7.0, np.float32)
    assert lib.fs_rrelieff_scores(None, None, 1.0, 2.0, p, out.ctypes.data_as(L._f32p)) \
        == L.FS_EINVAL
    with pytest.raises(ValueError, match="1 <= k <= n - 1"):
        L.rrelieff_score("cpu", x, targets[0], recip, isd, x.shape[0])
    with pytest.raises(ValueError, match="non-finite"):
        L.rrelieff_score("cpu", x, np.where(np.arange(300) == 5, np.nan, targets[0]), recip,
                         isd, k)
    with pytest.raises(ValueError, match="shape"):
        L.rrelieff_score("cpu", x, targets[0][:-1], recip, isd, k)


def planted():
    """X of stir_np.mixed_case(300, 20, 20); y = x[:, 3] + 0.5 (x[:, 25] == 2)
    + 0.3 N(0, 1), seed 0."""
    x = stir_np.mixed_case(300, 20, 20)[0]
    y = x[:, 3] + 0.5 * (x[:, 25] == 2) + 0.3 * np.random.default_rng(0).standard_normal(300)
    return x, y.astype(np.float64)


def planted_model():
    if "planted" not in _CACHE:
        x, y = planted()
        recip, isd = preprocess(x)
        _CACHE["planted"] = R.sums(x, y, recip, isd, 10)
    return _CACHE["planted"]


def test_estimator_surface():
    from sklearn.base import clone
    from sklearn.linear_model import LinearRegression
    from sklearn.pipeline import Pipeline
    x, y = planted()
    est = RReliefF(n_features_to_select=2, n_neighbors=10, backend="cpu")
    assert est.get_params() == {"n_features_to_select": 2, "discrete_limit": 10,
                                "n_neighbors": 10, "backend": "cpu", "verbose": False,
                                "n_jobs": -1}
    assert RReliefF().get_params()["n_neighbors"] == 10
    twin = clone(est)
    assert twin is not est and twin.get_params() == est.get_params()
    est.fit(x, y)
    model = planted_model()
    m_w = R.weights(*model)[0]
    tol = R.w_tolerance(*model, TOL)[0] + 2.0 ** -24 * np.abs(m_w)
    assert est.feature_importances_.dtype == np.float32
    assert np.all(np.abs(est.feature_importances_ - m_w) <= tol)
    assert set(est.top_features_.tolist()) == {3, 25}
    assert est.n_features_in_ == 40 and est.effective_backend_ == "cpu"
    assert np.array_equal(est.is_discrete_, np.arange(40) >= 20)
    assert np.array_equal(est.transform(x), x[:, est.top_features_])
    assert np.array_equal(twin.fit_transform(x, y), x[:, est.top_features_])
    assert type(est).__module__ == "fastselect_amd"
    pipe = Pipeline([("select", RReliefF(n_features_to_select=2, backend="cpu")),
                     ("fit", LinearRegression())]).fit(x, y)
    assert pipe.named_steps["fit"].coef_.shape == (2,)
    assert pipe.score(x, y) > 0.3
    for bad in (0, 300):
        with pytest.raises(ValueError, match="n_neighbors"):
            RReliefF(n_neighbors=bad, backend="cpu").fit(x, y)
    with pytest.raises(ValueError, match="backend"):
        RReliefF(backend="tpu").fit(x, y)
    with pytest.raises(ValueError, match="NaN"):
        RReliefF(backend="cpu").fit(x, np.where(np.arange(300) == 1, np.nan, y))


class RefitOnly(RReliefF):
    """RReliefF without the resident scorer: TuRF refits on X[:, active]."""
    _resident_scorer = None


def test_turf_resident_equals_refit():
    x, y = planted()
    kw = dict(n_features_to_select=2, n_neighbors=10, backend="cpu")
    a = TuRF(RReliefF(**kw), n_features_to_select=6, pct_remove=0.3).fit(x, y)
    b = TuRF(RefitOnly(**kw), n_features_to_select=6, pct_remove=0.3).fit(x, y)
    assert np.array_equal(a.top_features_, b.top_features_)
    assert {3, 25} <= set(a.top_features_.tolist())
    assert np.array_equal(a.feature_importances_, b.feature_importances_)
    assert a.feature_importances_.any()


def test_planted_case_and_its_permutation_test():
    """Measured with this file's model (float32 keys, k = 10): the top scores
    are 0.0518 (feature 25) and 0.0455 (feature 3), the next 0.0165
    (feature 38); over 99 permutations (random_state = 0) the null maxima lie
    between 0.0116 and 0.0386, both planted features have p = 0.01 on both
    p-values, and the smallest max-T p among the 38 noise features is 0.83."""
    x, y = planted()
    m_w = R.weights(*planted_model())[0]
    order = np.argsort(m_w)[::-1]
    assert set(order[:2].tolist()) == {3, 25}  # on the model first
    print(f"model: top scores {m_w[order[:3]]} at {order[:3]}")
    est = RReliefF(n_features_to_select=2, n_neighbors=10, backend="cpu")
    est.permutation_test(x, y, n_permutations=99, random_state=0)
    fit = RReliefF(n_features_to_select=2, n_neighbors=10, backend="cpu").fit(x, y)
    assert np.array_equal(est.feature_importances_, fit.feature_importances_)
    assert np.array_equal(est.top_features_, fit.top_features_)
    assert set(est.top_features_.tolist()) == {3, 25}
    assert est.n_permutations_ == 99 and not hasattr(est, "null_scores_")
    assert est.p_values_.shape == est.p_values_maxT_.shape == (40,)
    assert est.null_max_scores_.shape == (99,)
    assert est.null_mean_.shape == est.null_std_.shape == (40,)
    noise = np.setdiff1d(np.arange(40), [3, 25])
    print(f"null maxima {est.null_max_scores_.min():.4f} .. {est.null_max_scores_.max():.4f}, "
          f"smallest noise max-T p {est.p_values_maxT_[noise].min():.2f}")
    assert est.p_values_[[3, 25]].tolist() == [0.01, 0.01]
    assert est.p_values_maxT_[[3, 25]].tolist() == [0.01, 0.01]
    assert est.p_values_maxT_[noise].min() >= 0.2
    assert np.all(est.p_values_maxT_ >= est.p_values_)
    # the null is the one-shot call's rows, and row 0 is the fit
    kept = RReliefF(n_features_to_select=2, n_neighbors=10, backend="cpu")
    kept.permutation_test(x, y, n_permutations=99, random_state=0, keep_null=True)
    rng = np.random.default_rng(0)
    t = np.stack([y] + [rng.permutation(y) for _ in range(99)])
    recip, isd = preprocess(x)
    direct = L.rrelieff_score("cpu", x, t, recip, isd, 10)
    assert np.array_equal(direct[0], est.feature_importances_)
    assert np.array_equal(kept.null_scores_, direct[1:].astype(np.float64))
    assert np.array_equal(kept.null_max_scores_, direct[1:].max(axis=1).astype(np.float64))
    assert np.array_equal(kept.p_values_, est.p_values_)
    np.testing.assert_allclose(kept.null_mean_, direct[1:].astype(np.float64).mean(axis=0))
    np.testing.assert_allclose(kept.null_std_, direct[1:].astype(np.float64).std(axis=0))
    with pytest.raises(ValueError, match="n_permutations"):
        RReliefF(backend="cpu").permutation_test(x, y, n_permutations=0)
