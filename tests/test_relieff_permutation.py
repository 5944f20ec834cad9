"""The ReliefF permutation test on the CPU backend:
fs_plan_relieff_score_labels / fs_relieff_score_labels
(fs_relieff_labels_cpu.cpp) and ReliefF.permutation_test.

The CPU backend computes the label-independent state once and, per labelling,
runs the plan's own selection and update on the swapped labels, class count
and priors, so every row is held to the bits of a plan created with that
labelling -- no tolerance there.  Against the float64 numpy model
(relieff_labels_np.py) the float64 sums of float32 pass-2 operands (each
rounded once, ~6e-8 of the feature's range) are held to 1e-6 of the two
non-cancelling parts, Miss_f + Hit_f.
"""
import ctypes
import warnings

import numpy as np
import pytest

import relieff_labels_np as model

from fastselect_amd import ReliefF, _lib as L

_CACHE = {}
K = 10

# permutation_test seed of the planted case: with it both planted features
# reach the smallest p (0.01 at B = 99); the smallest max-T p among the noise
# features is printed by planted_check (k = 10, both backends: 0.52)
PLANTED_SEED = 0
PLANTED = (3, 25)


def mixed():
    """(x, y_enc, recip, isd, probs) of the standard 300 x (20 + 20) case."""
    if "mixed" not in _CACHE:
        x, y = model.mixed_case()
        _CACHE["mixed"] = (x,) + model.preprocess(x, y)
    return _CACHE["mixed"]


def five_labellings(y_enc, seed=3):
    """y, three permutations, and a labelling with a 4-member class of code 5
    (fewer than K other members: the self-hit; codes 2..4 have no member)."""
    rng = np.random.default_rng(seed)
    rows = [y_enc] + [rng.permutation(y_enc) for _ in range(3)]
    last = y_enc.copy()
    last[[7, 90, 131, 299]] = 5
    return np.stack(rows + [last]).astype(np.int32)


def plan_for(lab_b, backend="cpu", k=K, x=None, recip=None, isd=None, rows=None):
    """A plan created with labelling lab_b as y, the way the estimator forms
    its inputs (compact codes, float32 class shares)."""
    if x is None:
        x, _, recip, isd, _ = mixed()
    codes, enc, cnt = np.unique(lab_b, return_inverse=True, return_counts=True)
    probs = (cnt / lab_b.size).astype(np.float32)
    return L.RowsPlan(backend, "relieff", x, enc.astype(np.int32), recip, isd, k=k,
                      class_probs=probs, rows=rows)


def plan_sums(pl, n_kept):
    out = np.zeros(n_kept)
    pl.score(out.ctypes.data)
    return out


def _abi_call(pl, lab, B, out):
    lab = np.ascontiguousarray(lab, dtype=np.int32)
    return L.lib().fs_plan_relieff_score_labels(
        pl._h, lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.c_int64(B),
        ctypes.c_void_p(out.ctypes.data))


def test_every_row_is_a_fresh_plans_score_bit_for_bit():
    x, y_enc, recip, isd, probs = mixed()
    n, p = x.shape
    lab = five_labellings(y_enc)
    pl = plan_for(y_enc)
    try:
        before = plan_sums(pl, p)
        out = np.full(5 * p, np.nan)
        pl.score_labels(lab, out.ctypes.data)
        assert pl.labels_info() == (0, 5, 0, 0)
        assert pl.labels_kernel_ms(3) == -1.0  # no GPU plan
        after = plan_sums(pl, p)
    finally:
        pl.close()
    out = out.reshape(5, p)
    assert np.array_equal(before, after) and before.any()
    assert np.array_equal(out[0], before)
    for b in range(5):
        fresh = plan_for(lab[b])
        try:
            assert np.array_equal(out[b], plan_sums(fresh, p)), f"labelling {b}"
        finally:
            fresh.close()
    assert not np.array_equal(out[0], out[1])
    # the one-shot call: the same sums divided by n, and fs_relieff_score's bits
    s = L.relieff_score_labels("cpu", x, lab, recip, isd, K)
    assert s.shape == (5, p) and s.dtype == np.float32
    assert np.array_equal(s, (out / n).astype(np.float32))
    assert np.array_equal(s[0], L.relieff_score("cpu", x, y_enc, recip, isd, K, probs))
    assert np.array_equal(L.relieff_score_labels("cpu", x, lab, recip, isd, K, n_jobs=3), s)


def test_model_agrees(oracle):
    x, y_enc, recip, isd, _ = mixed()
    lab = five_labellings(y_enc)
    miss, hit, score, sets = model.score_parts(x, lab, recip, isd, K,
                                               argsort=oracle.numba_argsort, neighbours=True)
    n = x.shape[0]
    s = L.relieff_score_labels("cpu", x, lab, recip, isd, K).astype(np.float64)
    r = float(np.max(np.abs(s - score / n) / ((miss + hit) / n)))
    print(f"cpu: max |S - S_model| / (Miss + Hit) = {r:.3e}")
    assert r <= 1e-6
    # the small class: 3 other members, so its rows meet themselves on the walk
    for i in (7, 90, 131, 299):
        assert len(sets[4][i][5]) == 3 and i not in sets[4][i][5]
    assert all(len(sets[0][i][c]) == K for i in range(n) for c in (0, 1))


def test_set_features_and_no_earlier_score():
    x, y_enc, recip, isd, _ = mixed()
    lab = five_labellings(y_enc)
    feat = np.array([25, 3, 11, 30])
    pl = plan_for(y_enc)
    try:
        pl.set_features(feat)
        out = np.zeros(5 * feat.size)
        assert _abi_call(pl, lab, 5, out) == L.FS_OK
    finally:
        pl.close()
    xs = np.ascontiguousarray(x[:, feat])
    for b in (0, 4):
        fresh = plan_for(lab[b], x=xs, recip=recip[feat], isd=isd[feat])
        try:
            assert np.array_equal(out.reshape(5, -1)[b], plan_sums(fresh, feat.size))
        finally:
            fresh.close()


def test_status_codes():
    x, y_enc, recip, isd, probs = mixed()
    n, p = x.shape
    lab = five_labellings(y_enc)
    out = np.full(5 * p, np.nan)
    lib = L.lib()

    def code(pl, labels=lab, B=5):
        try:
            return _abi_call(pl, labels, B, out)
        finally:
            pl.close()

    # fs_plan_score_labels keeps refusing ReliefF plans
    pl = plan_for(y_enc)
    try:
        assert lib.fs_plan_score_labels(pl._h, lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                        ctypes.c_int64(5),
                                        ctypes.c_void_p(out.ctypes.data)) == L.FS_EINVAL
        info = np.zeros(4, dtype=np.int64)
        assert lib.fs_plan_relieff_labels_info(
            pl._h, info.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) == L.FS_EINVAL
        # B = 0 writes nothing
        assert _abi_call(pl, lab, 0, out) == L.FS_OK and np.all(np.isnan(out))
    finally:
        pl.close()
    # MultiSURF and SURF plans
    y = y_enc.astype(np.float64)
    assert code(L.Plan("cpu", x, y, recip, isd)) == L.FS_EINVAL
    assert code(L.RowsPlan("cpu", "surf", x, y_enc, recip, isd)) == L.FS_EINVAL
    # a row range, reference order
    assert code(plan_for(y_enc, rows=(0, 150))) == L.FS_ENOTSUP
    with L.accumulation("reference"):
        pl = plan_for(y_enc)
    assert code(pl) == L.FS_ENOTSUP
    # a single class, a code outside [0, 64): nothing is written
    one = lab.copy()
    one[3] = 1
    assert code(plan_for(y_enc), labels=one) == L.FS_EINVAL
    assert "labelling 3" in lib.fs_last_error().decode()
    for bad in (64, -1):
        wide = lab.copy()
        wide[2, 17] = bad
        assert code(plan_for(y_enc), labels=wide) == L.FS_EINVAL
    assert np.all(np.isnan(out))
    # arguments
    assert code(plan_for(y_enc), B=-1) == L.FS_EINVAL
    assert lib.fs_plan_relieff_score_labels(None, None, ctypes.c_int64(1), None) == L.FS_EINVAL
    assert lib.fs_plan_relieff_labels_kernel_ms(None, 0) == -1.0
    with pytest.raises(ValueError):
        L.relieff_score_labels("cpu", x, lab[:, :-1], recip, isd, K)
    with pytest.raises(ValueError):
        L.relieff_score_labels("cpu", x, one, recip, isd, K)
    with L.accumulation("reference"), pytest.raises(RuntimeError, match="reference"):
        L.relieff_score_labels("cpu", x, lab, recip, isd, K)


# ---- the estimator ---------------------------------------------------------

def planted_check(backend):
    """The planted 300 x 40 case at B = 99 (shared with the GPU file): both
    planted features at the smallest p-value, no noise feature significant."""
    x, y = model.mixed_case()
    est = ReliefF(n_features_to_select=2, n_neighbors=K, backend=backend).permutation_test(
        x, y, n_permutations=99, random_state=PLANTED_SEED)
    noise = np.setdiff1d(np.arange(x.shape[1]), PLANTED)
    print(f"{backend}: planted max-T p {est.p_values_maxT_[list(PLANTED)]}, smallest noise "
          f"max-T p {est.p_values_maxT_[noise].min():.2f}")
    assert np.all(est.p_values_maxT_[list(PLANTED)] == 0.01)
    assert np.all(est.p_values_[list(PLANTED)] == 0.01)
    assert np.all(est.p_values_maxT_[noise] > 0.05)
    assert set(est.top_features_.tolist()) == set(PLANTED)
    return est


def test_planted_features_are_significant_and_noise_is_not():
    est = planted_check("cpu")
    assert est.effective_backend_ == "cpu" and est.n_permutations_ == 99
    assert est.devices_ is None and not hasattr(est, "null_scores_")


def test_p_values_are_the_formulas_on_the_null():
    x, y = model.mixed_case()
    B = 12
    est = ReliefF(backend="cpu", n_neighbors=K).permutation_test(
        x, y, n_permutations=B, random_state=5, keep_null=True)
    null, obs = est.null_scores_, est.feature_importances_.astype(np.float64)
    p = x.shape[1]
    assert null.shape == (B, p)
    exp = np.array([(1 + np.sum(null[:, f] >= obs[f])) / (1 + B) for f in range(p)])
    mx = null.max(axis=1)
    exp_max = np.array([(1 + np.sum(mx >= obs[f])) / (1 + B) for f in range(p)])
    assert np.array_equal(est.p_values_, exp) and np.array_equal(est.p_values_maxT_, exp_max)
    assert np.array_equal(est.null_max_scores_, mx)
    assert np.array_equal(est.null_mean_, null.mean(axis=0))
    assert np.array_equal(est.null_std_, null.std(axis=0))
    assert est.n_permutations_ == B
    # the fit attributes are the plain fit's
    fit = ReliefF(backend="cpu", n_neighbors=K).fit(x, y)
    assert np.array_equal(est.feature_importances_, fit.feature_importances_)
    assert np.array_equal(est.top_features_, fit.top_features_)
    # a null row is the plain score of the permuted labels
    y_enc, recip, isd, probs = model.preprocess(x, y)
    first = np.random.default_rng(5).permutation(y_enc)
    ref = L.relieff_score("cpu", x, first, recip, isd, K, probs)
    assert np.array_equal(null[0].astype(np.float32), ref)
    again = ReliefF(backend="cpu", n_neighbors=K).permutation_test(
        x, y, n_permutations=B, random_state=5)
    assert np.array_equal(again.p_values_, est.p_values_) and not hasattr(again, "null_scores_")


def test_value_errors_and_the_small_class_warning():
    x, y = model.mixed_case()
    with pytest.raises(ValueError, match="reference"):
        ReliefF(backend="cpu", accumulation="reference").permutation_test(x, y, n_permutations=3)
    for bad in (0, -4):
        with pytest.raises(ValueError, match="n_permutations"):
            ReliefF(backend="cpu").permutation_test(x, y, n_permutations=bad)
    with pytest.raises(ValueError, match="single class"):
        ReliefF(backend="cpu").permutation_test(x, np.zeros_like(y), n_permutations=3)
    x3, y3 = model.three_class_case()
    with pytest.warns(UserWarning, match="smallest class size"):
        est = ReliefF(backend="cpu", n_neighbors=5).permutation_test(x3, y3, n_permutations=2)
    assert est.p_values_.shape == (x3.shape[1],)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ReliefF(backend="cpu", n_neighbors=3).permutation_test(x, y, n_permutations=2)
