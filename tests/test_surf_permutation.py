"""The SURF / SURF* permutation test on the CPU backend
(fs_surf_labels_cpu.cpp), its refusals, the estimator method and the numpy
model the GPU tests use (surf_labels_np.py).

The CPU rows are the plan's own arithmetic on swapped labels, so they are held
to the plan bit for bit; against the float64 model they are held to the bar of
the GPU tests: |S - S_model| <= 1e-5 x (the sum of the non-cancelling parts the
score is made of), per entry.
"""
import ctypes

import numpy as np
import pytest

import surf_labels_np as model
from fastselect_amd import SURF, SURFstar, _lib
from oracle import relief_np
from test_multisurf_permutation import PLANTED, PLANTED_SEED

TOL = 1e-5

_CACHE = {}


def case():
    """(x64, y, recip, isd, labellings, parts) of the mixed 300 x (20 + 20) case."""
    if "case" not in _CACHE:
        x, y = model.mixed_case()
        x = x.astype(np.float64)
        recip, isd = model.preprocess(x)
        lab = model.labellings(y)
        _CACHE["case"] = (x, y, recip, isd, lab, model.score_parts(x, lab, recip, isd))
    return _CACHE["case"]


def plan_rows(star):
    """(rows[37, p] of fs_plan_surf_score_labels on a CPU plan, its info)."""
    if ("rows", star) not in _CACHE:
        x, y, recip, isd, lab, _ = case()
        pl = _lib.RowsPlan("cpu", "surf", x, lab[0], recip, isd, use_star=star)
        try:
            out = np.full((lab.shape[0], x.shape[1]), np.nan)
            pl.surf_score_labels(lab, out.ctypes.data)
            _CACHE[("rows", star)] = (out, pl.surf_labels_info())
        finally:
            pl.close()
    return _CACHE[("rows", star)]


@pytest.mark.parametrize("star", [False, True])
def test_the_model_is_the_oracle(star):
    """surf_labels_np decides and sums as oracle/relief_np.surf does: its
    scores of y and of a 3-class labelling are the oracle's float32 scores."""
    x, y, recip, isd, lab, parts = case()
    sc, tot = model.scores(parts, star)
    for b in (0, 33):
        ref = relief_np.surf(x, lab[b], recip, isd, star).astype(np.float64)
        # the oracle rounds its mean of n samples to float32
        assert np.all(np.abs(sc[b] / x.shape[0] - ref) <= 2.0 ** -22 * np.maximum(np.abs(ref), 1.0))
    near = model.near_sets(x, recip, isd)
    assert parts[4] == int(near.sum()) and 0 < parts[4] < x.shape[0] * (x.shape[0] - 1)


@pytest.mark.parametrize("star", [False, True])
def test_every_row_is_the_plans_score_with_that_labelling(star):
    x, y, recip, isd, lab, _ = case()
    rows, info = plan_rows(star)
    for b in range(lab.shape[0]):
        pl = _lib.RowsPlan("cpu", "surf", x, lab[b], recip, isd, use_star=star)
        try:
            one = np.full(x.shape[1], np.nan)
            pl.score(one.ctypes.data)
        finally:
            pl.close()
        assert np.array_equal(one, rows[b]), b
    assert info[2] == lab.shape[0] and info[3] == 0


@pytest.mark.parametrize("star", [False, True])
def test_one_shot_call_is_surf_score_bit_for_bit(star):
    x, y, recip, isd, lab, _ = case()
    s = _lib.surf_score_labels("cpu", x, lab, recip, isd, use_star=star)
    assert s.shape == (37, x.shape[1]) and s.dtype == np.float32
    for b in (0, 5, 33, 35, 36):
        assert np.array_equal(s[b], _lib.surf_score("cpu", x, lab[b], recip, star, isd)), b
    rows = plan_rows(star)[0]
    assert np.array_equal(s, (rows / x.shape[0]).astype(np.float32))


@pytest.mark.parametrize("star", [False, True])
def test_cpu_rows_match_the_model(star):
    x, y, recip, isd, lab, parts = case()
    sc, tot = model.scores(parts, star)
    rows, info = plan_rows(star)
    assert np.all(tot > 0)
    r = float(np.max(np.abs(rows - sc) / tot))
    print(f"star={star}: max |S_cpu - S_model| / parts = {r:.3e}")
    assert r <= TOL
    # the near sides are the model's; every near side belongs to a listed pair
    assert info[1] == parts[4] and info[1] / 2 <= info[0] <= info[1]
    # the all-equal labelling has no miss: SURF's scores are minus the near hits
    if not star:
        assert np.all(rows[36] <= 0)


def test_refusals():
    x, y, recip, isd, lab, _ = case()
    n, p = x.shape
    out = np.zeros((37, p))
    labp = lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    outp = ctypes.c_void_p(out.ctypes.data)
    call = _lib.lib().fs_plan_surf_score_labels

    def code(pl, B=37, lp=labp, op=outp):
        try:
            return call(pl._h, lp, ctypes.c_int64(B), op)
        finally:
            pl.close()

    yi = y.astype(np.int32)
    x32 = x.astype(np.float32)
    pl = _lib.RowsPlan("cpu", "relieff", x32, yi, recip, isd, k=3,
                       class_probs=np.bincount(yi) / n)
    assert code(pl) == _lib.FS_EINVAL
    assert code(_lib.Plan("cpu", x32, y, recip, isd)) == _lib.FS_EINVAL
    assert code(_lib.RowsPlan("cpu", "surf", x, yi, recip, isd), op=None) == _lib.FS_EINVAL
    assert code(_lib.RowsPlan("cpu", "surf", x, yi, recip, isd), lp=None) == _lib.FS_EINVAL
    with _lib.accumulation("reference"):
        pl = _lib.RowsPlan("cpu", "surf", x, yi, recip, isd)
    assert code(pl) == _lib.FS_ENOTSUP
    assert code(_lib.RowsPlan("cpu", "surf", x, yi, recip, isd, rows=(0, 100))) == _lib.FS_ENOTSUP
    # B = 0 writes nothing; the CPU backend takes any codes and any number of classes
    assert code(_lib.RowsPlan("cpu", "surf", x, yi, recip, isd), B=0, lp=None,
                op=None) == _lib.FS_OK
    many = (np.arange(n, dtype=np.int32) % 11) * 1000 - 3
    manyp = many.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    for star in (False, True):
        assert code(_lib.RowsPlan("cpu", "surf", x, yi, recip, isd, use_star=star), B=1,
                    lp=manyp) == _lib.FS_OK
    # the two older label calls still refuse a SURF plan with their code
    pl = _lib.RowsPlan("cpu", "surf", x, yi, recip, isd)
    try:
        assert _lib.lib().fs_plan_score_labels(pl._h, labp, ctypes.c_int64(37),
                                               outp) == _lib.FS_EINVAL
        assert _lib.lib().fs_plan_relieff_score_labels(pl._h, labp, ctypes.c_int64(37),
                                                       outp) == _lib.FS_EINVAL
        with pytest.raises(Exception):
            pl.surf_labels_info()  # no completed call yet
    finally:
        pl.close()
    with _lib.accumulation("reference"):
        with pytest.raises(Exception):
            _lib.surf_score_labels("cpu", x, lab, recip, isd)


def epistatic_case():
    """The X of the planted case with two binary columns whose XOR is y: a pure
    interaction, which SURF* is built for."""
    x, _ = model.mixed_case()
    rng = np.random.default_rng(7)
    a, b = EPISTATIC
    x[:, a] = rng.integers(0, 2, size=x.shape[0])
    x[:, b] = rng.integers(0, 2, size=x.shape[0])
    return x, (x[:, a] != x[:, b]).astype(np.float64)


EPISTATIC = (22, 31)


def planted_check(backend, cls):
    """B = 99 on the planted 300 x 40 case of test_multisurf_permutation (its
    data builder).  SURF: both planted features at the smallest p-value on both
    p-values, no noise feature significant; seen on the CPU backend: planted
    max-T p 0.01 / 0.01, smallest noise max-T p 1.00.

    SURF* does not separate that case on the CPU backend at any seed or size
    tried (n = 200, 300, 600, seeds 0-2: the planted columns rank 5th to 21st
    of 40, and with B = 99 their p-values are 1.0): its far pairs weigh a main
    effect's misses negatively, and y there is a sum of two main effects.  For
    SURFstar the check therefore runs on ``epistatic_case``: the same X with
    two binary columns whose XOR is y.  Seen on the CPU backend: planted max-T
    p 0.01 / 0.01, smallest noise max-T p 0.83."""
    if cls is SURFstar:
        (x, y), planted = epistatic_case(), EPISTATIC
    else:
        x, y = model.mixed_case()
        planted = PLANTED
    est = cls(n_features_to_select=2, backend=backend).permutation_test(
        x.astype(np.float64), y, n_permutations=99, random_state=PLANTED_SEED)
    noise = np.setdiff1d(np.arange(x.shape[1]), planted)
    print(f"{backend} {cls.__name__}: planted max-T p {est.p_values_maxT_[list(planted)]}, "
          f"smallest noise max-T p {est.p_values_maxT_[noise].min():.2f}")
    assert np.all(est.p_values_maxT_[list(planted)] == 0.01)
    assert np.all(est.p_values_[list(planted)] == 0.01)
    assert np.all(est.p_values_maxT_[noise] > 0.05)
    assert set(est.top_features_.tolist()) == set(planted)
    return est


@pytest.mark.parametrize("cls", [SURF, SURFstar])
def test_planted_features_are_significant_and_noise_is_not(cls):
    est = planted_check("cpu", cls)
    assert est.effective_backend_ == "cpu" and est.n_permutations_ == 99
    assert est.devices_ is None and not hasattr(est, "null_scores_")
    assert est.use_star == (cls is SURFstar)


@pytest.mark.parametrize("cls", [SURF, SURFstar])
def test_p_values_are_the_formulas_on_the_null(cls):
    x, y = model.mixed_case()
    x = x.astype(np.float64)
    B = 20
    est = cls(backend="cpu").permutation_test(x, y, n_permutations=B, random_state=5,
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
    assert est.n_permutations_ == B
    # the observed scores are fit's; a null row is the plain score of that permutation
    fit = cls(backend="cpu").fit(x, y)
    assert np.array_equal(est.feature_importances_, fit.feature_importances_)
    enc = np.unique(y, return_inverse=True)[1].astype(np.int32)
    first = np.random.default_rng(5).permutation(enc)
    recip, isd = model.preprocess(x)
    assert np.array_equal(null[0].astype(np.float32),
                          _lib.surf_score("cpu", x, first, recip, est.use_star, isd))
    # keep_null=False on the same estimator drops the stored null
    est.permutation_test(x, y, n_permutations=3, random_state=5)
    assert not hasattr(est, "null_scores_") and est.n_permutations_ == 3


def test_value_errors():
    x, y = model.mixed_case()
    x = x.astype(np.float64)
    with pytest.raises(ValueError, match="single class"):
        SURF(backend="cpu").permutation_test(x, np.zeros(x.shape[0]), n_permutations=5)
    with pytest.raises(ValueError, match="reference"):
        SURF(backend="cpu", accumulation="reference").permutation_test(x, y, n_permutations=5)
    with pytest.raises(ValueError, match="n_permutations"):
        SURFstar(backend="cpu").permutation_test(x, y, n_permutations=0)
    assert SURFstar.permutation_test is SURF.permutation_test
