"""RReliefF on the GPU (fs_rrelieff.hip: k_rrf_update and k_rrf_sc inside
fs_plan_score_targets, on the lists of a one-class ReliefF plan) against the
float64 numpy model (rrelieff_np.py) and against itself.

The first test pins the one-class selection on the device: S_A and S_C
against the model, whose lists are the k nearest of all in the reference's
float32 keys and numba's tie order.

Sum bar.  The argument of tests/test_gpu_stir_relieff.py: every term of S_A,
S_CA and S_C is non-negative, so nothing cancels and the relative error of a
sum is bounded by that of its terms.  A diff is |a - b| of two float32 pass-2
operands, each rounded once (~6e-8 of the feature's range), widened to
float64 before it is multiplied by the float64 dy and summed; S_C has
float64 terms only.  The assertion is the project's parity bar, 1e-5, on
every entry (the error seen is printed), and W is held to that bar
propagated through the epilogue (rrelieff_np.w_tolerance).  Sums that regroup
the device's own float64 terms (row ranges) are held to 1e-12.  Rows of a
batch against their own B = 1 call, S_A across batch sizes and a repeated
call are compared bit for bit.
"""
import numpy as np
import pytest

import rrelieff_np as R
from test_rrelieff import (SHAPES, case, check_against_model, plan_targets, planted,
                           planted_model, refusal_cases, whole)

pytestmark = pytest.mark.gpu

SUM_TOL = 1e-5
ADD_TOL = 1e-12


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    from fastselect_amd import _lib
    assert _lib.device_count() >= 1, "no HIP device visible: GPU tests cannot run"


@pytest.mark.parametrize("name", list(SHAPES))
def test_one_class_lists_s_a_and_s_c_match_the_model(name, oracle):
    """S_A and S_C do not weigh a feature by the target (S_A) or a target by a
    feature (S_C): they pin the neighbour lists of the one-class selection."""
    x, recip, isd, k, targets, (m_a, m_ca, m_c, m_m) = case(name, oracle)
    r = whole(name, oracle, "gpu")
    assert r["m"] == m_m == x.shape[0] * k
    ea = float(np.max(np.abs(r["s_a"] - m_a) / m_a))
    ec = float(np.max(np.abs(r["s_c"] - m_c) / m_c))
    print(f"{name}: max relative error of S_A {ea:.3e}, of S_C {ec:.3e}")
    assert ea <= SUM_TOL and ec <= SUM_TOL


@pytest.mark.parametrize("name", list(SHAPES))
def test_sums_and_w_match_the_model(name, oracle):
    x, recip, isd, k, targets, model = case(name, oracle)
    r = whole(name, oracle, "gpu")
    m_a, m_ca, m_c, m_m = model
    assert np.all(m_a > 0) and np.all(m_ca > 0) and np.all(m_c > 0)
    errs = [float(np.max(np.abs(r[q] - m) / m))
            for q, m in (("s_a", m_a), ("s_ca", m_ca), ("s_c", m_c))]
    print(f"{name}: max relative error of S_A {errs[0]:.3e}, S_CA {errs[1]:.3e}, "
          f"S_C {errs[2]:.3e}; selection {r['sel_ms']:.3f} ms, k_rrf_update "
          f"{r['upd_ms']:.3f} ms over 3 chunks")
    assert max(errs) <= SUM_TOL
    from fastselect_amd import _lib as L
    w = L.rrelieff_scores(r["s_a"], r["s_ca"], r["s_c"], r["m"])
    m_w = R.weights(*model)
    tol = R.w_tolerance(m_a, m_ca, m_c, m_m, SUM_TOL)
    print(f"{name}: max |W - model| / tolerance {np.max(np.abs(w - m_w) / tol):.3e}")
    assert np.all(np.abs(w - m_w) <= tol)
    assert r["sel_ms"] > 0 and r["upd_ms"] > 0
    # a repeated call gives the same bits
    for a, b in zip(r["again"], (r["s_a"], r["s_ca"], r["s_c"])):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", list(SHAPES))
def test_batch_rows_have_the_bits_of_their_own_call(name, oracle):
    """B = 1 (the width-1 kernel), 8 (a full chunk), 9 (a chunk and a single
    target at width 1) and 17 (two chunks and a single one); B = 12 and 3 add
    ragged chunks of 4 and 3 at width 8."""
    x, recip, isd, k, targets, _ = case(name, oracle)
    full = whole(name, oracle, "gpu")  # B = 17
    sizes = (8, 9, 17, 12, 3)
    # one plan: the 17 single calls, then every batch size twice
    batches = [targets[b] for b in range(17)] + [targets[:B] for B in sizes for _ in range(2)]
    r = plan_targets("gpu", x, recip, isd, k, targets[0], more=batches)
    ones, rest = r["more"][:17], r["more"][17:]
    assert np.array_equal(r["s_ca"], ones[0][1])
    for b, (s_a, s_ca, s_c) in enumerate(ones):
        assert s_ca.shape == (1, x.shape[1]) and s_c.shape == (1,)
        assert np.array_equal(s_a, full["s_a"]), b
        # another plan's call of all 17
        assert np.array_equal(s_ca[0], full["s_ca"][b]) and s_c[0] == full["s_c"][b], b
    for q, B in enumerate(sizes):
        (s_a, s_ca, s_c), twice = rest[2 * q], rest[2 * q + 1]
        assert s_ca.shape == (B, x.shape[1]) and s_c.shape == (B,)
        assert np.array_equal(s_a, full["s_a"]), B
        for b in range(B):
            assert np.array_equal(s_ca[b], ones[b][1][0]), (B, b)
            assert s_c[b] == ones[b][2][0], (B, b)
        for a, c in zip(twice, (s_a, s_ca, s_c)):
            assert np.array_equal(a, c), B


def test_row_ranges_add_up(oracle):
    x, recip, isd, k, targets, _ = case("mixed", oracle)
    ref = whole("mixed", oracle, "gpu")
    parts = [plan_targets("gpu", x, recip, isd, k, targets, rows=rg)
             for rg in ((0, 100), (100, 300))]
    assert sum(p["m"] for p in parts) == ref["m"]
    for q in ("s_a", "s_ca", "s_c"):
        assert all(np.all(p[q] > 0) for p in parts)
        np.testing.assert_allclose(sum(p[q] for p in parts), ref[q], rtol=ADD_TOL, atol=0)
    m = R.sums(x, targets, recip, isd, k, rows=(100, 300))
    check_against_model(parts[1], m, SUM_TOL, "rows [100, 300)")
    e = plan_targets("gpu", x, recip, isd, k, targets, rows=(128, 128))
    assert e["m"] == 0 and not e["s_a"].any() and not e["s_ca"].any() and not e["s_c"].any()


def test_feature_subset_of_both_kinds(oracle):
    x, recip, isd, k, targets, _ = case("mixed", oracle)
    feat = np.array([1, 3, 7, 19, 22, 25, 30, 38])
    r = plan_targets("gpu", x, recip, isd, k, targets[:9], feat=feat)
    m = R.sums(np.ascontiguousarray(x[:, feat]), targets[:9], recip[feat], isd[feat], k)
    assert r["s_a"].shape == (feat.size,) and r["s_ca"].shape == (9, feat.size)
    check_against_model(r, m, SUM_TOL, "subset")
    assert r["upd_ms"] > 0


def test_constant_target_and_one_shot(oracle):
    from fastselect_amd import _lib as L
    x, recip, isd, k, targets, model = case("mixed", oracle)
    t = np.stack([np.full(x.shape[0], 4.25), targets[0]])
    r = plan_targets("gpu", x, recip, isd, k, t)
    assert r["s_c"][0] == 0.0 and not r["s_ca"][0].any() and r["s_a"].all()
    w = L.rrelieff_score("gpu", x, t, recip, isd, k)
    assert w.shape == (2, x.shape[1]) and not w[0].any()
    assert np.array_equal(w, L.rrelieff_scores(r["s_a"], r["s_ca"], r["s_c"], r["m"]))
    m_a, m_ca, m_c, m_m = model
    tol = R.w_tolerance(m_a, m_ca[:1], m_c[:1], m_m, SUM_TOL)[0]
    assert np.all(np.abs(w[1] - R.weights(m_a, m_ca[:1], m_c[:1], m_m)[0]) <= tol)


def test_estimator_and_permutation_test_against_the_cpu_backend():
    from fastselect_amd import RReliefF, TuRF
    x, y = planted()
    model = planted_model()
    m_w = R.weights(*model)[0]
    assert set(np.argsort(m_w)[::-1][:2].tolist()) == {3, 25}  # on the model first
    tol = R.w_tolerance(*model, SUM_TOL)[0]
    kw = dict(n_features_to_select=2, n_neighbors=10)
    gpu = RReliefF(backend="gpu", **kw).fit(x, y)
    cpu = RReliefF(backend="cpu", **kw).fit(x, y)
    assert gpu.effective_backend_ == "gpu" and cpu.effective_backend_ == "cpu"
    assert gpu.feature_importances_.dtype == np.float32 and gpu.n_features_in_ == 40
    assert np.array_equal(gpu.top_features_, cpu.top_features_)
    assert np.array_equal(gpu.is_discrete_, cpu.is_discrete_)
    for est in (gpu, cpu):
        print(f"{est.effective_backend_}: max |W - model| / tolerance "
              f"{np.max(np.abs(est.feature_importances_ - m_w) / tol):.3e}")
        assert np.all(np.abs(est.feature_importances_ - m_w) <= tol)
    gp = RReliefF(backend="gpu", **kw).permutation_test(x, y, n_permutations=99, random_state=0,
                                                        keep_null=True)
    cp = RReliefF(backend="cpu", **kw).permutation_test(x, y, n_permutations=99, random_state=0,
                                                        keep_null=True)
    assert np.array_equal(gp.feature_importances_, gpu.feature_importances_)
    assert np.array_equal(gp.top_features_, cp.top_features_)
    print(f"max |null GPU - null CPU| {np.max(np.abs(gp.null_scores_ - cp.null_scores_)):.3e}")
    assert np.array_equal(gp.p_values_, cp.p_values_)
    assert np.array_equal(gp.p_values_maxT_, cp.p_values_maxT_)
    assert gp.p_values_[[3, 25]].tolist() == [0.01, 0.01]
    assert gp.p_values_maxT_[[3, 25]].tolist() == [0.01, 0.01]
    assert np.delete(gp.p_values_maxT_, [3, 25]).min() >= 0.2
    # TuRF keeps X resident on the device and agrees with the CPU backend
    a = TuRF(RReliefF(backend="gpu", **kw), n_features_to_select=6, pct_remove=0.3).fit(x, y)
    b = TuRF(RReliefF(backend="cpu", **kw), n_features_to_select=6, pct_remove=0.3).fit(x, y)
    assert np.array_equal(a.top_features_, b.top_features_)


def test_refusals_on_the_device(oracle):
    import torch
    x, recip, isd, k, targets, _ = case("mixed", oracle)
    p = x.shape[1]
    buf = torch.full((3 * p + 2,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()  # the plans run on streams of their own
    p0 = buf.data_ptr()

    def snapshot():
        h = buf.cpu().numpy()
        return h[:p], h[p:3 * p], h[3 * p:]

    refusal_cases("gpu", x, recip, isd, k, targets, (p0, p0 + 8 * p, p0 + 8 * 3 * p, snapshot))
    assert float(buf.min()) == float(buf.max()) == -7.0
