"""STIR for ReliefF on the GPU (fs_stir_relieff.hip: k_rf_stir and
k_rf_stir_counts inside fs_plan_score_stir) against the float64 numpy model
(stir_relieff_np.py) and against itself.

Sum bar.  Every term of the four sums is non-negative, so nothing cancels:
the relative error of a sum is bounded by that of its terms.  A term is
|a - b| of two float32 pass-2 operands, each rounded once (~6e-8 of the
feature's range), or its square, widened to float64 before it is summed: the
sums sit well below 1e-6 (seen on an MI355X: 6.7e-8 at most over the five
shapes); the assertion is the project's parity bar, 1e-5, on every entry,
and t is held to that bar propagated through the epilogue
(stir_np.t_tolerance).  Sums that regroup the device's own float64 terms (row
ranges) are held to 1e-12; a repeated call and the two accumulation modes
(the same lists, the same kernel) give the same bits.
"""
import numpy as np
import pytest

import stir_np
import stir_relieff_np as M
from test_stir_relieff import mixed_model, plan_stir, rel_err

pytestmark = pytest.mark.gpu

SUM_TOL = 1e-5
ADD_TOL = 1e-12

_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    from fastselect_amd import _lib
    assert _lib.device_count() >= 1, "no HIP device visible: GPU tests cannot run"


# name -> (n, continuous columns, discrete columns, k)
SHAPES = {
    # five 64-row blocks with a ragged last one; one feature block half
    # continuous, half discrete
    "mixed": (300, 20, 20, 3),
    # one sample past a 128-row tile; the continuous part padded to 256, a
    # wholly discrete block with a ragged tail; lists of 10 = 4 + 4 + 2
    "n130-p270": (130, 200, 70, 10),
    # ties at nearly every k-th key: numba's order in the model
    "discrete-p64": (130, 0, 64, 5),
    # the unroll's tail with a single neighbour
    "continuous-p64": (130, 64, 0, 1),
    # found < k, and a found count (3) that is no multiple of the unroll
    "three-class": (300, 20, 20, 5),
}


def case(name, oracle):
    """(x, y_enc, recip, isd, probs, k, (model sums, |H|, |M|)), once per session."""
    if name not in _CACHE:
        n, pc, pd, k = SHAPES[name]
        x, y = M.three_class_case() if name == "three-class" else stir_np.mixed_case(n, pc, pd)
        pre = M.preprocess(x, y)
        assert int(pre[2].sum()) == pd
        argsort = oracle.numba_argsort if name == "discrete-p64" else None
        model = mixed_model(k) if name == "mixed" else M.stir_sums(x, pre[0], pre[1], pre[2], k,
                                                                   argsort=argsort)
        _CACHE[name] = (x,) + pre + (k, model)
    return _CACHE[name]


def whole(name, oracle):
    if ("whole", name) not in _CACHE:
        _CACHE["whole", name] = plan_stir("gpu", *case(name, oracle)[:6])
    return _CACHE["whole", name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_sums_and_counts_match_the_model(name, oracle):
    x, y_enc, recip, isd, probs, k, (m_sums, m_h, m_m) = case(name, oracle)
    r = whole(name, oracle)
    assert (r["n_hit"], r["n_miss"]) == (m_h, m_m)
    assert np.all(m_sums > 0)
    err = rel_err(r["stir"], m_sums)
    print(f"{name}: max relative error of the four sums {err:.3e}, "
          f"k_rf_stir {r['kernel_ms']:.3f} ms")
    assert err <= SUM_TOL
    # a discrete feature's squares are its diffs
    assert np.array_equal(r["stir"][1][isd], r["stir"][0][isd])
    assert np.array_equal(r["stir"][3][isd], r["stir"][2][isd])
    # the score's bits, before, inside and after; a second call's bits
    assert r["before"].any()
    assert np.array_equal(r["sums"], r["before"]) and np.array_equal(r["after"], r["before"])
    s2, t2, h2, m2 = r["again"]
    assert np.array_equal(s2, r["before"]) and np.array_equal(t2, r["stir"])
    assert (h2, m2) == (m_h, m_m)
    assert r["kernel_ms"] > 0


def test_three_class_counts(oracle):
    """Class 2 has 4 members, k = 5: 3 hits per class-2 row, no self pair."""
    m_h, m_m = case("three-class", oracle)[6][1:]
    assert (m_h, m_m) == (296 * 5 + 4 * 3, 296 * 9 + 4 * 10)
    r = whole("three-class", oracle)
    assert (r["n_hit"], r["n_miss"]) == (m_h, m_m)


def test_row_ranges_add_up(oracle):
    args = case("mixed", oracle)[:6]
    ref = whole("mixed", oracle)
    parts = [plan_stir("gpu", *args, rows=rg) for rg in ((0, 77), (77, 128), (128, 300))]
    assert sum(p["n_hit"] for p in parts) == ref["n_hit"]
    assert sum(p["n_miss"] for p in parts) == ref["n_miss"]
    assert all(np.all(p["stir"] > 0) for p in parts)
    np.testing.assert_allclose(sum(p["stir"] for p in parts), ref["stir"], rtol=ADD_TOL, atol=0)
    m = M.stir_sums(*args[:4], args[5], rows=(77, 128))
    assert (parts[1]["n_hit"], parts[1]["n_miss"]) == m[1:]
    assert rel_err(parts[1]["stir"], m[0]) <= SUM_TOL
    e = plan_stir("gpu", *args, rows=(128, 128))
    assert (e["n_hit"], e["n_miss"]) == (0, 0) and not e["stir"].any()


def test_reference_accumulation(oracle):
    args = case("mixed", oracle)[:6]
    fast = whole("mixed", oracle)
    r = plan_stir("gpu", *args, accumulation="reference")
    assert r["before"].any()
    assert np.array_equal(r["sums"], r["before"]) and np.array_equal(r["after"], r["before"])
    assert (r["n_hit"], r["n_miss"]) == (fast["n_hit"], fast["n_miss"])
    np.testing.assert_allclose(r["stir"], fast["stir"], rtol=ADD_TOL, atol=0)


def test_feature_subset_of_both_kinds(oracle):
    x, y_enc, recip, isd, probs, k, _ = case("mixed", oracle)
    feat = np.array([1, 3, 7, 19, 22, 25, 30, 38])
    r = plan_stir("gpu", x, y_enc, recip, isd, probs, k, feat=feat)
    m_sums, m_h, m_m = M.stir_sums(np.ascontiguousarray(x[:, feat]), y_enc, recip[feat],
                                   isd[feat], k)
    assert r["stir"].shape == (4, feat.size) and (r["n_hit"], r["n_miss"]) == (m_h, m_m)
    assert np.all(m_sums > 0)
    err = rel_err(r["stir"], m_sums)
    print(f"subset: max relative error {err:.3e}")
    assert err <= SUM_TOL
    assert np.array_equal(r["sums"], r["before"])


def test_estimator_against_the_cpu_backend():
    from fastselect_amd import ReliefF
    x, y = stir_np.mixed_case(300, 20, 20)
    k = 10
    m_sums, m_h, m_m = mixed_model(k)
    m_t = M.statistics(m_sums, m_h, m_m)[2]
    first = np.argsort(m_t)[::-1][:2].tolist()
    assert set(first) == {3, 25}  # the planted pair, on the model first
    tol = M.t_tolerance(m_sums, m_h, m_m, SUM_TOL)
    gpu = ReliefF(n_features_to_select=2, n_neighbors=k, backend="gpu").stir_test(x, y)
    cpu = ReliefF(n_features_to_select=2, n_neighbors=k, backend="cpu").stir_test(x, y)
    assert gpu.effective_backend_ == "gpu" and gpu.devices_ == [0]
    for est in (gpu, cpu):
        assert (est.stir_n_hit_pairs_, est.stir_n_miss_pairs_) == (m_h, m_m)
        print(f"{est.effective_backend_}: max |t - model| / tolerance "
              f"{np.max(np.abs(est.stir_t_ - m_t) / tol):.3e}")
        assert np.all(np.abs(est.stir_t_ - m_t) <= tol)
        assert np.argsort(est.stir_t_)[::-1][:2].tolist() == first
    assert gpu.stir_df_ == cpu.stir_df_ == m_h + m_m - 2
    with pytest.raises(ValueError, match="one device"):
        ReliefF(backend="gpu", devices=[0, 0]).stir_test(x, y)


def test_refusals_on_the_device(oracle):
    import torch
    from fastselect_amd import _lib
    x, y_enc, recip, isd, probs, k, _ = case("mixed", oracle)
    p = x.shape[1]
    s = torch.empty(p, dtype=torch.float64, device="cuda")
    t = torch.empty(4 * p, dtype=torch.float64, device="cuda")
    c = torch.empty(2, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()  # the plans run on streams of their own
    surf = _lib.RowsPlan("gpu", "surf", x.astype(np.float64), y_enc, recip, isd)
    try:
        with pytest.raises(RuntimeError, match="SURF"):
            surf.score_stir(s.data_ptr(), t.data_ptr(), c.data_ptr())
    finally:
        surf.close()
    rf = _lib.RowsPlan("gpu", "relieff", x, y_enc, recip, isd, k=k, class_probs=probs)
    try:
        assert rf.stir_kernel_ms(2) == -1.0  # no score_stir yet
        with pytest.raises(ValueError, match="NULL"):
            rf.score_stir(s.data_ptr(), 0, c.data_ptr())
        with pytest.raises(ValueError, match="MultiSURF plans"):
            rf.stir(t.data_ptr())
    finally:
        rf.close()
