"""STIR on the CPU backend (fs_stir_cpu.cpp, fs_stir.h, MultiSURF.stir_test)
against the float64 numpy model (stir_np.py).

The CPU backend sums the reference's float32 diffs (widened to float64) over
the plan's near pairs, the model sums the same terms in another order: with
at most 14474 non-negative terms per sum the two differ by at most
14474 * 1.1e-16 = 1.6e-12 relative, so 1e-10 leaves room only for the order.
Sums that only regroup the plan's own terms (ranks, row ranges) are held to
1e-12.  Nothing here asserts calibration: on the mixed case the 38 noise
features have a median p of 0.73 but a smallest p of 6.8e-7.
"""
import numpy as np
import pytest

import stir_np
from conftest import scale_rel_err

from fastselect_amd import MultiSURF, MultiSURFstar, _lib as L
from fastselect_amd.MultiSURF import adjust_p_values, stir_p_values

_CACHE = {}


def mixed():
    """(x, y, recip, isd, model sums, |H|, |M|, model counts), once per session."""
    if "mixed" not in _CACHE:
        x, y = stir_np.mixed_case()
        recip, isd = stir_np.preprocess(x)
        _CACHE["mixed"] = (x, y, recip, isd) + stir_np.stir_sums(x, y, recip, isd)
    return _CACHE["mixed"]


def plan_sums(x, y, recip, isd, feat=None, rows=None, n_jobs=-1):
    """(sums[4, k], counts[n, 2]) of one world-1 CPU plan."""
    n = x.shape[0]
    pl = L.Plan("cpu", x, y, recip, isd, feat_idx=feat, n_jobs=n_jobs)
    try:
        rs, cn = np.zeros(3 * n), np.zeros(2 * n)
        pl.pass1(rs.ctypes.data)
        pl.select(rs.ctypes.data, cn.ctypes.data)
        if rows is not None:
            pl.set_rows(*rows)
        s = np.zeros(4 * pl.n_kept)
        pl.stir(s.ctypes.data)
        return s.reshape(4, -1), cn.reshape(n, 2)
    finally:
        pl.close()


def whole():
    if "whole" not in _CACHE:
        x, y, recip, isd = mixed()[:4]
        _CACHE["whole"] = plan_sums(x, y, recip, isd)
    return _CACHE["whole"]


def test_sums_match_the_model():
    m_sums, m_h, m_m, m_counts = mixed()[4:]
    s, cn = whole()
    assert np.array_equal(cn.astype(np.int64), m_counts)
    np.testing.assert_allclose(s, m_sums, rtol=1e-10, atol=0)
    assert np.all(s > 0)


def test_pair_counts_are_the_models_integers():
    _, m_h, m_m, _ = mixed()[4:]
    _, cn = whole()
    assert (m_h, m_m) == (14474, 13046)
    assert (int(cn[:, 0].sum()), int(cn[:, 1].sum())) == (14474, 13046)


def test_same_bits_for_every_n_jobs():
    x, y, recip, isd = mixed()[:4]
    ref = plan_sums(x, y, recip, isd, n_jobs=1)[0]
    for nj in (3, 16):
        assert np.array_equal(plan_sums(x, y, recip, isd, n_jobs=nj)[0], ref)


def test_two_ranks_add_up():
    x, y, recip, isd = mixed()[:4]
    n = x.shape[0]
    plans = [L.Plan("cpu", x, y, recip, isd, rank=r, world=2) for r in range(2)]
    try:
        rs = [np.zeros(3 * n) for _ in plans]
        for pl, r in zip(plans, rs):
            pl.pass1(r.ctypes.data)
        rs_all = rs[0] + rs[1]
        cn = [np.zeros(2 * n) for _ in plans]
        for pl, c in zip(plans, cn):
            pl.select(rs_all.ctypes.data, c.ctypes.data)
        parts = [np.zeros(4 * x.shape[1]) for _ in plans]
        for pl, s in zip(plans, parts):
            pl.stir(s.ctypes.data)
    finally:
        for pl in plans:
            pl.close()
    s, c1 = whole()
    assert np.array_equal((cn[0] + cn[1]).reshape(n, 2), c1)
    assert np.all(parts[0] > 0) and np.all(parts[1] > 0)
    np.testing.assert_allclose((parts[0] + parts[1]).reshape(4, -1), s, rtol=1e-12, atol=0)


def test_row_ranges_add_up():
    x, y, recip, isd = mixed()[:4]
    a = plan_sums(x, y, recip, isd, rows=(0, 150))[0]
    b = plan_sums(x, y, recip, isd, rows=(150, 300))[0]
    np.testing.assert_allclose(a + b, whole()[0], rtol=1e-12, atol=0)
    # a half is the model's half: a pair side counts for its own focal sample
    m = stir_np.stir_sums(*mixed()[:4], rows=(0, 150))[0]
    np.testing.assert_allclose(a, m, rtol=1e-10, atol=0)


def test_feature_subset_is_its_own_model():
    x, y, recip, isd = mixed()[:4]
    feat = np.array([1, 3, 7, 19, 22, 25, 30, 38])
    n = x.shape[0]
    pl = L.Plan("cpu", x, y, recip, isd)
    try:
        pl.set_features(feat)
        rs, cn = np.zeros(3 * n), np.zeros(2 * n)
        pl.pass1(rs.ctypes.data)
        pl.select(rs.ctypes.data, cn.ctypes.data)
        s = np.zeros(4 * feat.size)
        pl.stir(s.ctypes.data)
    finally:
        pl.close()
    m_sums, m_h, m_m, m_counts = stir_np.stir_sums(np.ascontiguousarray(x[:, feat]), y,
                                                   recip[feat], isd[feat])
    assert np.array_equal(cn.reshape(n, 2).astype(np.int64), m_counts)
    np.testing.assert_allclose(s.reshape(4, -1), m_sums, rtol=1e-10, atol=0)


def test_statistics_match_the_models_epilogue():
    """The mixed case with a constant column (every diff 0: t = 0, p = 1) and
    a discrete column equal to y (every hit diff 0, every miss diff 1:
    sp == 0, t = +inf, p = 0)."""
    x, y = stir_np.mixed_case()
    x[:, 10] = 0.25
    x[:, 30] = y
    recip, isd = stir_np.preprocess(x)
    s, cn = plan_sums(x, y, recip, isd)
    nh, nm = cn[:, 0].sum(), cn[:, 1].sum()
    hm, mm, t, df, sp = L.stir_statistics_ex(s, nh, nm)
    assert sp[10] == 0.0 and sp[30] == 0.0 and np.count_nonzero(sp == 0.0) == 2
    p = stir_p_values(t, df, sp)
    m_hm, m_mm, m_t, m_df, m_p = stir_np.statistics(s, nh, nm)
    assert df == m_df == nh + nm - 2
    np.testing.assert_allclose(hm, m_hm, rtol=1e-12, atol=0)
    np.testing.assert_allclose(mm, m_mm, rtol=1e-12, atol=0)
    fin = np.isfinite(m_t)
    assert np.array_equal(fin, np.isfinite(t))
    np.testing.assert_allclose(t[fin], m_t[fin], rtol=1e-12, atol=0)
    np.testing.assert_allclose(p, m_p, rtol=1e-12, atol=0)
    assert t[10] == 0.0 and p[10] == 1.0
    assert t[30] == np.inf and p[30] == 0.0
    assert np.all((p >= 0) & (p <= 1))


def test_stir_test_on_the_mixed_case():
    """feature_importances_ of stir_test (one resident step) against fit's
    (the one-shot call): equality is expected and was seen (max difference
    0.0 on the CPU backend); the bar is the project's 1e-5."""
    x, y = stir_np.mixed_case()
    est = MultiSURF(n_features_to_select=2, backend="cpu").stir_test(x, y)
    m_sums, m_h, m_m, _ = mixed()[4:]
    _, _, m_t, m_df, m_p = stir_np.statistics(m_sums, m_h, m_m)
    assert set(np.argsort(est.stir_t_)[-2:].tolist()) == {3, 25}
    assert est.stir_p_values_[3] < 1e-6 and est.stir_p_values_[25] < 1e-6
    assert (est.stir_n_hit_pairs_, est.stir_n_miss_pairs_) == (14474, 13046)
    assert est.stir_df_ == 14474 + 13046 - 2
    assert np.all(np.abs(est.stir_t_ - m_t) <= stir_np.t_tolerance(m_sums, m_h, m_m, 1e-10))
    np.testing.assert_allclose(est.stir_hit_mean_, m_sums[0] / m_h, rtol=1e-10, atol=0)
    np.testing.assert_allclose(est.stir_miss_mean_, m_sums[2] / m_m, rtol=1e-10, atol=0)
    assert np.array_equal(est.stir_p_adjusted_, stir_np.benjamini_hochberg(est.stir_p_values_))
    assert set(est.top_features_.tolist()) == {3, 25}
    fit = MultiSURF(n_features_to_select=2, backend="cpu").fit(x, y)
    diff = scale_rel_err(est.feature_importances_, fit.feature_importances_)
    print(f"stir_test vs fit feature_importances_: scale-relative {diff:.3e}")
    assert diff <= 1e-5
    assert np.array_equal(est.top_features_, fit.top_features_)
    assert np.array_equal(est.is_discrete_, fit.is_discrete_)
    assert est.n_features_in_ == fit.n_features_in_ == 40
    bon = MultiSURF(backend="cpu").stir_test(x, y, adjust="bonferroni")
    assert np.array_equal(bon.stir_p_adjusted_, np.minimum(bon.stir_p_values_ * 40, 1.0))
    raw = MultiSURF(backend="cpu").stir_test(x, y, adjust=None)
    assert np.array_equal(raw.stir_p_adjusted_, raw.stir_p_values_)


def test_benjamini_hochberg_by_hand():
    # sorted 0.005, 0.01, 0.03, 0.04, 0.5 -> p m / rank = 0.025, 0.025, 0.05,
    # 0.05, 0.5, already monotone
    p = np.array([0.01, 0.04, 0.03, 0.005, 0.5])
    np.testing.assert_allclose(adjust_p_values(p, "fdr_bh"), [0.025, 0.05, 0.05, 0.025, 0.5],
                               rtol=1e-15)
    # 0.01, 0.02, 0.021, 0.9, 0.95 -> 0.05, 0.05, 0.035, 1.125, 0.95: the step-up
    # takes the smaller value above (0.035 twice) and caps at 1 (0.95 twice)
    q = np.array([0.95, 0.021, 0.01, 0.9, 0.02])
    np.testing.assert_allclose(adjust_p_values(q, "fdr_bh"), [0.95, 0.035, 0.035, 0.95, 0.035],
                               rtol=1e-15)
    with pytest.raises(ValueError):
        adjust_p_values(p, "holm")


def test_refusals():
    x, y, recip, isd = mixed()[:4]
    n, p = x.shape
    rs, cn, s = np.zeros(3 * n), np.zeros(2 * n), np.zeros(4 * p)
    pl = L.Plan("cpu", x, y, recip, isd, use_star=True)
    try:
        pl.pass1(rs.ctypes.data)
        pl.select(rs.ctypes.data, cn.ctypes.data)
        with pytest.raises(RuntimeError, match="MultiSURF\\*"):   # FS_ENOTSUP
            pl.stir(s.ctypes.data)
    finally:
        pl.close()
    pl = L.Plan("cpu", x, y, recip, isd)
    try:
        with pytest.raises(ValueError, match="fs_plan_select"):
            pl.stir(s.ctypes.data)
        pl.pass1(rs.ctypes.data)
        with pytest.raises(ValueError, match="fs_plan_select"):
            pl.stir(s.ctypes.data)
        pl.select(rs.ctypes.data, cn.ctypes.data)
        pl.stir(s.ctypes.data)
        pl.set_features(np.arange(5))
        with pytest.raises(ValueError, match="fs_plan_select"):
            pl.stir(s.ctypes.data)
        pl.set_features(None)
        pl.pass1(rs.ctypes.data)
        pl.select(rs.ctypes.data, cn.ctypes.data)
        pl.set_shard(0, 2)
        with pytest.raises(ValueError, match="fs_plan_select"):
            pl.stir(s.ctypes.data)
    finally:
        pl.close()
    yi = y.astype(np.int32)
    for rows in (L.RowsPlan("cpu", "relieff", x, yi, recip, isd, k=3,
                            class_probs=np.bincount(yi) / n),
                 L.RowsPlan("cpu", "surf", x.astype(np.float64), yi, recip, isd)):
        try:
            with pytest.raises(ValueError, match="MultiSURF plans"):
                rows.stir(s.ctypes.data)
        finally:
            rows.close()
    for est in (MultiSURF(backend="cpu", use_star=True), MultiSURFstar(backend="cpu")):
        with pytest.raises(ValueError, match="MultiSURF\\*"):
            est.stir_test(x, y)
    with pytest.raises(ValueError, match="adjust"):
        MultiSURF(backend="cpu").stir_test(x, y, adjust="holm")


def test_stir_needs_a_step_on_the_current_features():
    """With several tile shards stir() recomputes each shard's decisions from
    the last step's row statistics: after set_features those belong to
    another feature set, so it is refused until the next step()."""
    from fastselect_amd.parallel import ShardedMultiSURF
    x, y, recip, isd = mixed()[:4]
    for shards in (1, 2):
        job = ShardedMultiSURF(x, y, recip, isd, backend="cpu", shard=False, shards=shards)
        try:
            with pytest.raises(ValueError, match="step"):
                job.stir()
            job.step()
            whole_sums = job.stir()[0].numpy().copy()
            np.testing.assert_allclose(whole_sums, whole()[0], rtol=1e-12, atol=0)
            feat = np.array([1, 3, 22, 25])
            job.set_features(feat)
            with pytest.raises(ValueError, match="step"):
                job.stir()
            job.step()
            sub, nh, nm = job.stir()
            m = stir_np.stir_sums(np.ascontiguousarray(x[:, feat]), y, recip[feat], isd[feat])
            assert (nh, nm) == (m[1], m[2])
            np.testing.assert_allclose(sub.numpy(), m[0], rtol=1e-10, atol=0)
        finally:
            job.close()


def test_too_few_pairs_is_a_value_error():
    x, y = stir_np.mixed_case()
    sums = np.ones((4, 3))
    for nh, nm in ((1, 100), (100, 1), (0, 0)):
        with pytest.raises(ValueError, match="fewer than 2"):
            L.stir_statistics(sums, nh, nm)
    # one class: no near misses at all
    with pytest.raises(ValueError, match="fewer than 2"):
        MultiSURF(backend="cpu").stir_test(x, np.zeros(x.shape[0]))
