"""The MultiSURF permutation test on the CPU backend: fs_plan_score_labels /
fs_multisurf_score_labels (fs_labels_cpu.cpp) and MultiSURF.permutation_test.

The CPU backend plans once and, per labelling, runs the plan's own count loop
and pass 2 on the swapped labels, so every row is held to the bits of
``multisurf_score`` with that labelling as y -- no tolerance anywhere here.
"""
import ctypes

import numpy as np
import pytest

import multisurf_labels_np as model

from fastselect_amd import MultiSURF, _lib as L

_CACHE = {}

# permutation_test seed of the planted case, chosen on the CPU backend: with it
# both planted features reach the smallest p (0.01 at B = 99) and no noise
# feature has a max-T p-value at or below 0.05 (smallest: see planted_check)
PLANTED_SEED = 0
PLANTED = (3, 25)


def mixed(classes=2):
    """(x, y, recip, isd) of the standard 300 x (20 + 20) case; classes=3: a
    three-class y from the same two planted columns."""
    if classes not in _CACHE:
        x, y = model.mixed_case()
        if classes == 3:
            y = np.digitize(x[:, 3] + 0.5 * (x[:, 25] == 2), [0.45, 0.9]).astype(np.float64)
            assert np.unique(y).size == 3
        _CACHE[classes] = (x, y) + model.preprocess(x)
    return _CACHE[classes]


def five_labellings(y, seed=3):
    rng = np.random.default_rng(seed)
    enc = np.unique(y, return_inverse=True)[1].astype(np.int32)
    return np.stack([enc] + [rng.permutation(enc) for _ in range(4)])


@pytest.mark.parametrize("classes", [2, 3])
def test_every_row_is_the_plain_score_bit_for_bit(classes):
    x, y, recip, isd = mixed(classes)
    lab = five_labellings(y)
    s = L.multisurf_score_labels("cpu", x, lab, recip, isd)
    assert s.shape == (5, x.shape[1]) and s.dtype == np.float32
    for b in range(5):
        ref = L.multisurf_score("cpu", x, lab[b].astype(np.float64), recip, None, False, isd)
        assert np.array_equal(s[b], ref), f"labelling {b}"
    # row 0 is y itself: labels are compared by equality only
    assert np.array_equal(s[0], L.multisurf_score("cpu", x, y, recip, None, False, isd))
    # the labellings differ (a test of nothing otherwise)
    assert not np.array_equal(s[0], s[1])


def test_label_values_do_not_matter():
    x, y, recip, isd = mixed()
    lab = five_labellings(y)
    a = L.multisurf_score_labels("cpu", x, lab, recip, isd)
    b = L.multisurf_score_labels("cpu", x, 1000 - 7 * lab, recip, isd)
    assert np.array_equal(a, b)


def test_feature_subsets_bit_for_bit():
    x, y, recip, isd = mixed()
    lab = five_labellings(y)
    for feat in (np.array([1, 3, 7, 19, 22, 25, 30, 38]), np.array([25, 3]), np.arange(20, 40)):
        s = L.multisurf_score_labels("cpu", x, lab, recip, isd, feat_idx=feat)
        assert s.shape == (5, feat.size)
        for b in range(5):
            ref = L.multisurf_score("cpu", x, lab[b].astype(np.float64), recip, feat, False, isd)
            assert np.array_equal(s[b], ref)


def test_same_bits_for_every_n_jobs():
    x, y, recip, isd = mixed()
    lab = five_labellings(y)
    ref = L.multisurf_score_labels("cpu", x, lab, recip, isd, n_jobs=1)
    assert np.array_equal(L.multisurf_score_labels("cpu", x, lab, recip, isd, n_jobs=5), ref)


def test_model_agrees():
    """The numpy model's counts are the plan's, and its scores the library's
    (float32 scores of float64 sums: 1e-6 of the non-cancelling parts)."""
    x, y, recip, isd = mixed()
    lab = five_labellings(y)
    miss, hit, score, counts = model.score_parts(x, lab, recip, isd)
    n = x.shape[0]
    s = L.multisurf_score_labels("cpu", x, lab, recip, isd)
    assert np.all(np.abs(s - score / n) <= 1e-6 * (miss + hit) / n)
    pl = L.Plan("cpu", x, y, recip, isd)
    try:
        rs, cn = np.zeros(3 * n), np.zeros(2 * n)
        pl.pass1(rs.ctypes.data)
        pl.select(rs.ctypes.data, cn.ctypes.data)
    finally:
        pl.close()
    assert np.array_equal(cn.reshape(n, 2).astype(np.int64), counts[0])


# ---- the plan call and its status codes, through the ABI ---------------------

def _abi_call(pl, lab, B, out):
    lab = np.ascontiguousarray(lab, dtype=np.int32)
    return L.lib().fs_plan_score_labels(pl._h, lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                        ctypes.c_int64(B), ctypes.c_void_p(out.ctypes.data))


def _selected(pl, n):
    rs, cn = np.zeros(3 * n), np.zeros(2 * n)
    pl.pass1(rs.ctypes.data)
    pl.select(rs.ctypes.data, cn.ctypes.data)
    return rs, cn


def test_plan_call_and_pass2_untouched():
    x, y, recip, isd = mixed()
    n, p = x.shape
    lab = five_labellings(y)
    pl = L.Plan("cpu", x, y, recip, isd)
    try:
        rs, cn = _selected(pl, n)
        before = np.zeros(p)
        pl.pass2(cn.ctypes.data, before.ctypes.data)
        out = np.full(5 * p, np.nan)
        assert _abi_call(pl, lab, 5, out) == L.FS_OK
        after = np.zeros(p)
        pl.pass2(cn.ctypes.data, after.ctypes.data)
        assert np.array_equal(before, after)
        # sums, not divided by n; row 0 = the plan's own pass 2
        assert np.array_equal(out.reshape(5, p)[0], before)
        ref = L.multisurf_score_labels("cpu", x, lab, recip, isd)
        assert np.array_equal((out.reshape(5, p) / n).astype(np.float32), ref)
        # B = 0 writes nothing
        out[:] = np.nan
        assert _abi_call(pl, lab, 0, out) == L.FS_OK and np.all(np.isnan(out))
        # honours set_features (after a new pass1 + select)
        feat = np.array([25, 3, 11])
        pl.set_features(feat)
        out3 = np.zeros(5 * 3)
        assert _abi_call(pl, lab, 5, out3) == L.FS_EINVAL  # re-targeted: no select yet
        _selected(pl, n)
        assert _abi_call(pl, lab, 5, out3) == L.FS_OK
        ref3 = L.multisurf_score_labels("cpu", x, lab, recip, isd, feat_idx=feat)
        assert np.array_equal((out3.reshape(5, 3) / n).astype(np.float32), ref3)
    finally:
        pl.close()


def test_status_codes():
    x, y, recip, isd = mixed()
    n, p = x.shape
    lab = five_labellings(y)
    out = np.zeros(5 * p)

    def code(pl, prepare=True, B=5):
        try:
            if prepare:
                _selected(pl, n)
            return _abi_call(pl, lab, B, out)
        finally:
            pl.close()

    # no select since creation / since pass 1
    assert code(L.Plan("cpu", x, y, recip, isd), prepare=False) == L.FS_EINVAL
    pl = L.Plan("cpu", x, y, recip, isd)
    rs, _ = _selected(pl, n)
    pl.pass1(rs.ctypes.data)
    assert code(pl, prepare=False) == L.FS_EINVAL
    assert "fs_plan_select" in L.lib().fs_last_error().decode()
    # a rank of two, a re-targeted shard, a row range
    assert code(L.Plan("cpu", x, y, recip, isd, rank=0, world=2)) == L.FS_ENOTSUP
    pl = L.Plan("cpu", x, y, recip, isd)
    pl.set_shard(1, 3)
    assert code(pl) == L.FS_ENOTSUP
    pl = L.Plan("cpu", x, y, recip, isd)
    _selected(pl, n)
    pl.set_rows(0, 150)
    assert code(pl, prepare=False) == L.FS_ENOTSUP
    # MultiSURF*, reference-order accumulation
    assert code(L.Plan("cpu", x, y, recip, isd, use_star=True)) == L.FS_ENOTSUP
    with L.accumulation("reference"):
        pl = L.Plan("cpu", x, y, recip, isd)
    assert code(pl) == L.FS_ENOTSUP
    # ReliefF and SURF plans
    yi = y.astype(np.int32)
    probs = np.bincount(yi) / n
    assert code(L.RowsPlan("cpu", "relieff", x, yi, recip, isd, k=3, class_probs=probs),
                prepare=False) == L.FS_EINVAL
    assert code(L.RowsPlan("cpu", "surf", x, yi, recip, isd), prepare=False) == L.FS_EINVAL
    # arguments
    pl = L.Plan("cpu", x, y, recip, isd)
    assert code(pl, B=-1) == L.FS_EINVAL
    assert L.lib().fs_plan_score_labels(None, None, ctypes.c_int64(1), None) == L.FS_EINVAL
    with pytest.raises(ValueError):
        L.multisurf_score_labels("cpu", x, lab[:, :-1], recip, isd)
    with L.accumulation("reference"), pytest.raises(RuntimeError, match="reference"):
        L.multisurf_score_labels("cpu", x, lab, recip, isd)


def test_kernel_ms_getter_without_a_gpu_plan():
    x, y, recip, isd = mixed()
    pl = L.Plan("cpu", x, y, recip, isd)
    try:
        assert pl.labels_kernel_ms(2) == -1.0
    finally:
        pl.close()


# ---- the estimator ---------------------------------------------------------

def planted_check(backend):
    """The planted 300 x 40 case at B = 99 (shared with the GPU file): both
    planted features at the smallest p-value, no noise feature significant."""
    x, y = model.mixed_case()
    est = MultiSURF(n_features_to_select=2, backend=backend).permutation_test(
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
    assert not hasattr(est, "null_scores_")


def test_p_values_are_the_formulas_on_the_null():
    x, y = model.mixed_case()
    B = 20
    est = MultiSURF(backend="cpu").permutation_test(x, y, n_permutations=B, random_state=5,
                                                    keep_null=True)
    null, obs = est.null_scores_, est.feature_importances_.astype(np.float64)
    p = x.shape[1]
    assert null.shape == (B, p)
    exp = np.array([(1 + np.sum(null[:, f] >= obs[f])) / (1 + B) for f in range(p)])
    mx = null.max(axis=1)
    exp_max = np.array([(1 + np.sum(mx >= obs[f])) / (1 + B) for f in range(p)])
    assert np.array_equal(est.p_values_, exp) and np.array_equal(est.p_values_maxT_, exp_max)
    assert np.array_equal(est.null_max_scores_, mx) and est.null_max_scores_.shape == (B,)
    assert np.array_equal(est.null_mean_, null.mean(axis=0))
    assert np.array_equal(est.null_std_, null.std(axis=0))
    assert np.all(est.p_values_maxT_ >= est.p_values_)
    assert est.n_permutations_ == B
    # the null rows are plain scores of permuted labels: the first permutation
    enc = np.unique(y, return_inverse=True)[1].astype(np.int32)
    first = np.random.default_rng(5).permutation(enc)
    recip, isd = model.preprocess(x)
    ref = L.multisurf_score("cpu", x, first.astype(np.float64), recip, None, False, isd)
    assert np.array_equal(null[0].astype(np.float32), ref)
    # the same random_state gives the same null, another one does not
    again = MultiSURF(backend="cpu").permutation_test(x, y, n_permutations=B, random_state=5,
                                                      keep_null=True)
    assert np.array_equal(again.null_scores_, null)
    other = MultiSURF(backend="cpu").permutation_test(x, y, n_permutations=B, random_state=6,
                                                      keep_null=True)
    assert not np.array_equal(other.null_scores_, null)


def test_fit_attributes_equal_the_stir_route():
    x, y = model.mixed_case()
    a = MultiSURF(n_features_to_select=5, backend="cpu").permutation_test(x, y, n_permutations=3,
                                                                          random_state=0)
    b = MultiSURF(n_features_to_select=5, backend="cpu").stir_test(x, y)
    assert np.array_equal(a.feature_importances_, b.feature_importances_)
    assert np.array_equal(a.top_features_, b.top_features_)
    assert np.array_equal(a.is_discrete_, b.is_discrete_)
    assert a.n_features_in_ == b.n_features_in_ == x.shape[1]
    assert a.effective_backend_ == "cpu" and a.devices_ is None
    # and the plain fit
    c = MultiSURF(n_features_to_select=5, backend="cpu").fit(x, y)
    assert np.array_equal(a.feature_importances_, c.feature_importances_)


def test_value_errors():
    x, y = model.mixed_case()
    with pytest.raises(ValueError, match="use_star"):
        MultiSURF(backend="cpu", use_star=True).permutation_test(x, y, n_permutations=3)
    with pytest.raises(ValueError, match="reference"):
        MultiSURF(backend="cpu", accumulation="reference").permutation_test(x, y, n_permutations=3)
    for bad in (0, -4):
        with pytest.raises(ValueError, match="n_permutations"):
            MultiSURF(backend="cpu").permutation_test(x, y, n_permutations=bad)
