"""STIR for ReliefF on the CPU backend (cpu::relieff_stir, fs_plan_score_stir,
ReliefF.stir_test) against the float64 numpy model (stir_relieff_np.py).

The CPU backend sums the reference's float32 diffs (widened to float64) over
the plan's neighbour lists, the model sums the same terms in another order.
A sum has at most n k (C - 1) = 6000 non-negative terms here, so the two
differ by at most 6000 * 1.1e-16 = 6.7e-13 relative: the bar is 1e-12, for
the order alone.  Row ranges regroup the plan's own terms and are held to the
same 1e-12; counts are integers and equal.  Nothing here asserts calibration.
"""
import numpy as np
import pytest

import stir_np
import stir_relieff_np as M

from fastselect_amd import ReliefF, _lib as L

TOL = 1e-12
_CACHE = {}


def plan_stir(backend, x, y_enc, recip, isd, probs, k, rows=None, feat=None, n_jobs=-1,
              accumulation="fast", algo="relieff"):
    """One resident plan; score, score_stir twice, score.  Returns a dict:
    before / after (``score``'s sums), sums (``score_stir``'s score sums),
    stir (4, n_kept), n_hit, n_miss, and again (the second call's (sums,
    stir, n_hit, n_miss))."""
    with L.accumulation(accumulation):
        pl = L.RowsPlan(backend, algo, x, y_enc, recip, isd, k=k, class_probs=probs, rows=rows,
                        n_jobs=n_jobs)
    try:
        if feat is not None:
            pl.set_features(feat)
        nk = pl.n_kept
        if backend == "gpu":
            import torch
            bufs = [torch.empty(m, dtype=torch.float64, device="cuda")
                    for m in (nk, nk, 4 * nk, 2, nk, 4 * nk, 2, nk)]
            torch.cuda.synchronize()  # the plan runs on a stream of its own
            ptr = [b.data_ptr() for b in bufs]
        else:
            bufs = [np.zeros(m) for m in (nk, nk, 4 * nk, 2, nk, 4 * nk, 2, nk)]
            ptr = [b.ctypes.data for b in bufs]
        pl.score(ptr[0])
        pl.score_stir(ptr[1], ptr[2], ptr[3])
        pl.score_stir(ptr[4], ptr[5], ptr[6])
        pl.score(ptr[7])
        ms = pl.stir_kernel_ms(2)
        h = [b.cpu().numpy() if backend == "gpu" else b for b in bufs]
    finally:
        pl.close()
    assert h[3][0] == int(h[3][0]) and h[3][1] == int(h[3][1])
    return {"before": h[0], "sums": h[1], "stir": h[2].reshape(4, nk), "n_hit": int(h[3][0]),
            "n_miss": int(h[3][1]), "after": h[7], "kernel_ms": ms,
            "again": (h[4], h[5].reshape(4, nk), int(h[6][0]), int(h[6][1]))}


def rel_err(a, ref):
    return float(np.max(np.abs(a - ref) / np.abs(ref)))


def mixed():
    """(x, y_enc, recip, isd, probs), once per session."""
    if "mixed" not in _CACHE:
        x, y = stir_np.mixed_case(300, 20, 20)
        _CACHE["mixed"] = (x,) + M.preprocess(x, y)
    return _CACHE["mixed"]


def mixed_model(k):
    if ("model", k) not in _CACHE:
        x, y_enc, recip, isd, _ = mixed()
        _CACHE["model", k] = M.stir_sums(x, y_enc, recip, isd, k)
    return _CACHE["model", k]


def mixed_whole(k):
    if ("whole", k) not in _CACHE:
        _CACHE["whole", k] = plan_stir("cpu", *mixed(), k)
    return _CACHE["whole", k]


def three_class():
    if "three" not in _CACHE:
        x, y = M.three_class_case()
        _CACHE["three"] = (x,) + M.preprocess(x, y)
    return _CACHE["three"]


def discrete(oracle):
    """All-discrete columns in {0, 1, 2}: the keys are small integers, so
    nearly every row ties at its k-th key and numba's order decides."""
    if "discrete" not in _CACHE:
        x, y = stir_np.mixed_case(130, 0, 64)
        pre = M.preprocess(x, y)
        assert pre[2].all() and np.bincount(pre[0]).min() > 5
        k = 5
        _CACHE["discrete"] = (x,) + pre + (k, M.stir_sums(x, pre[0], pre[1], pre[2], k,
                                                         argsort=oracle.numba_argsort))
    return _CACHE["discrete"]


@pytest.mark.parametrize("k", [3, 10])
def test_sums_and_counts_match_the_model(k):
    m_sums, m_h, m_m = mixed_model(k)
    r = mixed_whole(k)
    assert (r["n_hit"], r["n_miss"]) == (m_h, m_m) == (300 * k, 300 * k)
    assert np.all(m_sums > 0)
    err = rel_err(r["stir"], m_sums)
    print(f"k = {k}: max relative error of the four sums {err:.3e}")
    assert err <= TOL


def test_three_classes_with_a_small_class():
    """Class 2 has 4 members and k = 5: a class-2 focal row has 3 hits (its
    self-hit of the score is no pair), every other row 4 misses of class 2;
    M pools both other classes."""
    x, y_enc, recip, isd, probs = three_class()
    k = 5
    assert np.bincount(y_enc).tolist()[2] == 4 and np.bincount(y_enc)[:2].min() > k
    m_sums, m_h, m_m = M.stir_sums(x, y_enc, recip, isd, k)
    assert m_h == 296 * k + 4 * 3
    assert m_m == 296 * (k + 4) + 4 * (2 * k)
    r = plan_stir("cpu", x, y_enc, recip, isd, probs, k)
    assert (r["n_hit"], r["n_miss"]) == (m_h, m_m)
    assert np.all(m_sums > 0)
    err = rel_err(r["stir"], m_sums)
    print(f"three classes: max relative error {err:.3e}")
    assert err <= TOL
    # the four class-2 rows alone: 3 hits each
    r2 = plan_stir("cpu", x, y_enc, recip, isd, probs, k, rows=(7, 8))
    assert y_enc[7] == 2 and (r2["n_hit"], r2["n_miss"]) == (3, 2 * k)


def test_discrete_columns_with_ties_at_the_kth_key(oracle):
    x, y_enc, recip, isd, probs, k, (m_sums, m_h, m_m) = discrete(oracle)
    stable = M.stir_sums(x, y_enc, recip, isd, k)[0]
    assert not np.array_equal(stable, m_sums), "no tie at a k-th key: the case checks nothing"
    r = plan_stir("cpu", x, y_enc, recip, isd, probs, k)
    assert (r["n_hit"], r["n_miss"]) == (m_h, m_m) == (130 * k, 130 * k)
    assert np.all(m_sums > 0)
    assert rel_err(r["stir"], m_sums) <= TOL
    assert np.array_equal(r["stir"][1], r["stir"][0]) and np.array_equal(r["stir"][3], r["stir"][2])


def test_row_ranges_add_up_and_n_jobs_does_not_matter():
    args = mixed()
    k = 3
    whole = mixed_whole(k)
    parts = [plan_stir("cpu", *args, k, rows=rg) for rg in ((0, 77), (77, 128), (128, 300))]
    assert sum(p["n_hit"] for p in parts) == whole["n_hit"]
    assert sum(p["n_miss"] for p in parts) == whole["n_miss"]
    assert all(np.all(p["stir"] > 0) for p in parts)
    np.testing.assert_allclose(sum(p["stir"] for p in parts), whole["stir"], rtol=TOL, atol=0)
    # a range is the model's range: a pair belongs to its focal sample
    m = M.stir_sums(*args[:4], k, rows=(77, 128))
    assert (parts[1]["n_hit"], parts[1]["n_miss"]) == m[1:]
    assert rel_err(parts[1]["stir"], m[0]) <= TOL
    # an empty range: zeros
    e = plan_stir("cpu", *args, k, rows=(128, 128))
    assert (e["n_hit"], e["n_miss"]) == (0, 0) and not e["stir"].any() and not e["sums"].any()
    ref = plan_stir("cpu", *args, k, n_jobs=1)
    for nj in (3, 16):
        got = plan_stir("cpu", *args, k, n_jobs=nj)
        assert np.array_equal(got["stir"], ref["stir"])
        assert (got["n_hit"], got["n_miss"]) == (ref["n_hit"], ref["n_miss"])


@pytest.mark.parametrize("accumulation", ["fast", "reference"])
def test_score_bits_are_scores(accumulation):
    r = plan_stir("cpu", *mixed(), 3, accumulation=accumulation)
    assert r["before"].any()
    assert np.array_equal(r["sums"], r["before"]) and np.array_equal(r["after"], r["before"])
    s2, t2, h2, m2 = r["again"]
    assert np.array_equal(s2, r["before"]) and np.array_equal(t2, r["stir"])
    assert (h2, m2) == (r["n_hit"], r["n_miss"])
    assert r["kernel_ms"] == -1.0  # a CPU plan has no kernel time
    # the neighbour sets do not depend on the accumulation mode
    np.testing.assert_allclose(r["stir"], mixed_whole(3)["stir"], rtol=TOL, atol=0)


def test_feature_subset_is_its_own_model():
    x, y_enc, recip, isd, probs = mixed()
    feat = np.array([1, 3, 7, 19, 22, 25, 30, 38])
    r = plan_stir("cpu", x, y_enc, recip, isd, probs, 3, feat=feat)
    m_sums, m_h, m_m = M.stir_sums(np.ascontiguousarray(x[:, feat]), y_enc, recip[feat],
                                   isd[feat], 3)
    assert r["stir"].shape == (4, feat.size) and (r["n_hit"], r["n_miss"]) == (m_h, m_m)
    assert np.all(m_sums > 0)
    assert rel_err(r["stir"], m_sums) <= TOL
    assert np.array_equal(r["sums"], r["before"])


def test_refusals():
    x, y_enc, recip, isd, probs = mixed()
    n, p = x.shape
    s, t, c = np.zeros(p), np.zeros(4 * p), np.zeros(2)
    surf = L.RowsPlan("cpu", "surf", x.astype(np.float64), y_enc, recip, isd)
    try:
        with pytest.raises(RuntimeError, match="SURF"):   # FS_ENOTSUP
            surf.score_stir(s.ctypes.data, t.ctypes.data, c.ctypes.data)
    finally:
        surf.close()
    ms = L.Plan("cpu", x, y_enc.astype(np.float64), recip, isd)
    try:
        with pytest.raises(ValueError, match="fs_plan_stir"):
            L.check(L.lib().fs_plan_score_stir(ms._h, s.ctypes.data, t.ctypes.data,
                                               c.ctypes.data))
    finally:
        ms.close()
    rf = L.RowsPlan("cpu", "relieff", x, y_enc, recip, isd, k=3, class_probs=probs)
    try:
        for ptrs in ((0, t.ctypes.data, c.ctypes.data), (s.ctypes.data, 0, c.ctypes.data),
                     (s.ctypes.data, t.ctypes.data, 0)):
            with pytest.raises(ValueError, match="NULL"):
                rf.score_stir(*ptrs)
        # fs_plan_stir keeps refusing ReliefF plans
        with pytest.raises(ValueError, match="MultiSURF plans"):
            rf.stir(t.ctypes.data)
    finally:
        rf.close()


def test_estimator_on_the_mixed_case():
    x, y = stir_np.mixed_case(300, 20, 20)
    k = 10
    m_sums, m_h, m_m = mixed_model(k)
    m_hm, m_mm, m_t, m_df, m_p = M.statistics(m_sums, m_h, m_m)
    # the planted pair on the model first: a failure here is the data's
    assert set(np.argsort(m_p)[:2].tolist()) == {3, 25}
    est = ReliefF(n_features_to_select=2, n_neighbors=k, backend="cpu").stir_test(x, y)
    assert (est.stir_n_hit_pairs_, est.stir_n_miss_pairs_) == (m_h, m_m)
    assert est.stir_df_ == m_df == m_h + m_m - 2
    assert np.all(np.abs(est.stir_t_ - m_t) <= M.t_tolerance(m_sums, m_h, m_m, 1e-9))
    np.testing.assert_allclose(est.stir_hit_mean_, m_hm, rtol=1e-9, atol=0)
    np.testing.assert_allclose(est.stir_miss_mean_, m_mm, rtol=1e-9, atol=0)
    # p-values: the model's epilogue on the plan's own sums (the estimator's
    # plan is mixed_whole's).  t agrees to a few ulp (the same float64
    # formula); p = sf(t) moves by about t^2 of t's relative error, and
    # t <= 40 here: 1600 * 1e-15 = 1.6e-12, so 1e-10.
    w = mixed_whole(k)
    _, _, w_t, _, w_p = M.statistics(w["stir"], w["n_hit"], w["n_miss"])
    assert np.max(np.abs(w_t)) <= 40
    np.testing.assert_allclose(est.stir_t_, w_t, rtol=1e-12, atol=0)
    np.testing.assert_allclose(est.stir_p_values_, w_p, rtol=1e-10, atol=0)
    assert np.all((est.stir_p_values_ >= 0) & (est.stir_p_values_ <= 1))
    assert set(np.argsort(est.stir_p_values_)[:2].tolist()) == {3, 25}
    assert np.array_equal(est.stir_p_adjusted_, stir_np.benjamini_hochberg(est.stir_p_values_))
    # the fit attributes are the resident refit's, bit for bit
    ref = ReliefF(n_features_to_select=2, n_neighbors=k, backend="cpu")
    scorer = ref._resident_scorer(x, y)
    try:
        scorer.refit(np.arange(x.shape[1]))
    finally:
        scorer.close()
    assert np.array_equal(est.feature_importances_, ref.feature_importances_)
    assert est.feature_importances_.dtype == np.float32
    assert np.array_equal(est.top_features_, ref.top_features_)
    assert np.array_equal(est.is_discrete_, ref.is_discrete_)
    assert est.n_features_in_ == ref.n_features_in_ == 40
    assert est.effective_backend_ == "cpu" and est.devices_ is None
    bon = ReliefF(n_neighbors=k, backend="cpu").stir_test(x, y, adjust="bonferroni")
    assert np.array_equal(bon.stir_p_adjusted_, np.minimum(bon.stir_p_values_ * 40, 1.0))
    raw = ReliefF(n_neighbors=k, backend="cpu").stir_test(x, y, adjust=None)
    assert np.array_equal(raw.stir_p_adjusted_, raw.stir_p_values_)
    with pytest.raises(ValueError, match="adjust"):
        ReliefF(backend="cpu").stir_test(x, y, adjust="holm")
    slow = ReliefF(n_neighbors=k, backend="cpu", accumulation="reference").stir_test(x, y)
    np.testing.assert_allclose(slow.stir_t_, est.stir_t_, rtol=1e-12, atol=0)


def test_too_few_pairs_and_a_single_class():
    x, y = stir_np.mixed_case(300, 20, 20)
    with pytest.raises(ValueError, match="single class"):
        ReliefF(backend="cpu").stir_test(x, np.zeros(x.shape[0]))
    # two samples: one hit-less row each, |H| = 0
    with pytest.raises(ValueError, match="fewer than 2"), \
            pytest.warns(UserWarning, match="smallest class size"):
        ReliefF(backend="cpu", n_neighbors=1).stir_test(x[:2], np.array([0.0, 1.0]))
