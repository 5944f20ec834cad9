"""The SURF / SURF* permutation test on the GPU (fs_surf_labels.hip:
lab_records with SURF's decisions, k_surf_lab_weights, k_lab_score; SURF*:
k_star_sort, k_star_lab_walk, k_star_lab_apply of fs_starterm.hip) against the
float64 numpy model (surf_labels_np.py) and against itself.

Accuracy bar.  A SURF score is NearMiss_f - NearHit_f and a SURF* score
NearMiss_f - NearHit_f + FarHit_f - FarMiss_f: sums of non-negative terms, so
each sum's relative error is bounded by its terms'.  A term is |a - b| of two
float32 pass-2 operands (each rounded once, ~6e-8 of the feature's range) times
an exact weight (+-1, +-2), summed in float32 chains of at most 256 pairs and
then in float64; the star part is summed in float64 from the same float32
operands.  Per entry |S_gpu - S_model| <= 1e-5 x (the sum of the parts the
score is made of), the project's bar of test_gpu_multisurf_labels.py; relative
to the score itself it would mean nothing on permuted labels, where the score
cancels to noise.  Largest ratio seen on an MI355X over the 37 labellings
(SURF / SURF*): see RATIOS_SEEN below.

Regrouping bar.  labels_chunk, labels_seg_len and star_lab_seg only regroup
float64 sums (the float32 partials are cut per tile; the walk's segments add
float64 partial sums in segment order), which moves a sum of terms of total
size T by a few 2^-53 T: held to 1e-12 T.
"""
import ctypes

import numpy as np
import pytest

import surf_labels_np as model

pytestmark = pytest.mark.gpu

TOL = 1e-5
ADD_TOL = 1e-12

# max |S_gpu - S_model| / parts per shape, (SURF, SURF*), on an MI355X; the
# regrouped runs differed from the default run by exactly 0 at every entry
RATIOS_SEEN = {
    "mixed": (4.4e-8, 4.5e-8),
    "n130-p270": (1.8e-7, 1.7e-7),
    "continuous-p64": (1.7e-7, 1.6e-7),
    "discrete-p64": (0.0, 0.0),
    "n600-p140": (2.6e-8, 2.5e-8),
    "n1100-p24": (1.5e-8, 1.3e-8),
}

_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    from fastselect_amd import _lib
    assert _lib.device_count() >= 1, "no HIP device visible: GPU tests cannot run"


# name -> (n, continuous columns, discrete columns): those of the MultiSURF
# test, and one with n above 1024 and few columns, where the column sort holds
# more than 4 items per thread and the walk cuts a column into 4 segments
SHAPES = {
    "mixed": (300, 20, 20),
    "n130-p270": (130, 200, 70),
    "continuous-p64": (130, 64, 0),
    "discrete-p64": (130, 0, 64),
    "n600-p140": (600, 100, 40),
    "n1100-p24": (1100, 12, 12),
}


def case(name):
    """(x64, y int32, recip, isd, labellings, parts), once per session."""
    if name not in _CACHE:
        n, pc, pd = SHAPES[name]
        x, y = model.mixed_case(n, pc, pd)
        x = x.astype(np.float64)
        recip, isd = model.preprocess(x)
        assert int(isd.sum()) == pd
        lab = model.labellings(y)
        _CACHE[name] = (x, lab[0].copy(), recip, isd, lab, model.score_parts(x, lab, recip, isd))
    return _CACHE[name]


def gpu_run(x, y, recip, isd, lab, star, feat=None, twice=False):
    """One plan: score, surf_score_labels (once or twice), score.  Returns
    (sums[B, k] or the list of two, the plan's score sums before / after,
    info, the four stage times)."""
    import torch
    from fastselect_amd import _lib
    pl = _lib.RowsPlan("gpu", "surf", x, y, recip, isd, use_star=star)
    try:
        if feat is not None:
            pl.set_features(feat)
        k = pl.n_kept
        torch.cuda.synchronize()

        def score():
            buf = torch.full((k,), float("nan"), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            pl.score(buf.data_ptr())
            return buf.cpu().numpy()

        s0 = score()
        outs = []
        for _ in range(2 if twice else 1):
            out = torch.full((lab.shape[0] * k,), float("nan"), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            pl.surf_score_labels(lab, out.data_ptr())
            outs.append(out.cpu().numpy().reshape(lab.shape[0], k))
        info = pl.surf_labels_info()
        ms = [pl.surf_labels_kernel_ms(w) for w in range(4)]
        s1 = score()
        return (outs if twice else outs[0]), (s0, s1), info, ms
    finally:
        pl.close()
        torch.cuda.synchronize()


def default_run(name, star):
    if ("run", name, star) not in _CACHE:
        _CACHE[("run", name, star)] = gpu_run(*case(name)[:5], star, twice=name == "mixed")
    return _CACHE[("run", name, star)]


def ratio(s, score, tot):
    return float(np.max(np.abs(s - score) / tot))


@pytest.mark.parametrize("star", [False, True])
@pytest.mark.parametrize("name", list(SHAPES))
def test_scores_match_the_model(name, star):
    x, y, recip, isd, lab, parts = case(name)
    score, tot = model.scores(parts, star)
    sums, plan, info, ms = default_run(name, star)
    if name == "mixed":
        sums = sums[0]
    # the decisions first: the near sides are the model's
    assert info[1] == parts[4] and info[0] > 0 and info[0] <= info[1]
    assert info[2] == 2 and info[3] == int(star)
    assert sums.shape == score.shape and np.all(np.isfinite(sums))
    assert np.all(tot > 0)
    r = ratio(sums, score, tot)
    print(f"{name} star={star}: max |S_gpu - S_model| / parts = {r:.3e}")
    assert r <= TOL
    # row 0 against the plan's own score
    assert np.all(np.abs(sums[0] - plan[0]) <= TOL * tot[0])
    assert all(m > 0 for m in ms[:3]) and (ms[3] > 0 if star else ms[3] == -1.0)
    if not star:  # the all-equal labelling has no miss: minus the near hits
        assert np.all(sums[36] <= 0)


@pytest.mark.parametrize("star", [False, True])
def test_the_plans_score_is_untouched_and_the_call_is_deterministic(star):
    sums, plan, _, _ = default_run("mixed", star)
    assert np.all(np.isfinite(plan[0])) and np.array_equal(plan[0], plan[1])
    assert np.array_equal(sums[0], sums[1])


@pytest.mark.parametrize("star", [False, True])
@pytest.mark.parametrize("hook", [("labels_chunk", 5, "labels_seg_len", 1, "star_lab_seg", 200),
                                  ("labels_chunk", 7, "labels_seg_len", 3, "star_lab_seg", 150),
                                  ("star_lab_seg", 32), ("star_lab_seg", 600)])
def test_chunks_and_segments_regroup_float64_sums_only(hooks, hook, star):
    """600 sorted items in 3 segments (200), 4 unaligned ones (150), 19 (32) or
    one (600); the default cuts them into 2 of 320."""
    x, y, recip, isd, lab, parts = case("n600-p140")
    score, tot = model.scores(parts, star)
    ref = default_run("n600-p140", star)[0]
    for q in range(0, len(hook), 2):
        hooks(hook[q], hook[q + 1])
    sums, _, info, _ = gpu_run(x, y, recip, isd, lab, star)
    assert ratio(sums, score, tot) <= TOL
    d = float(np.max(np.abs(sums - ref) / tot))
    print(f"{hook} star={star}: max |S - S_default| / parts = {d:.3e}")
    assert d <= ADD_TOL
    if hook[0] == "labels_chunk":
        assert info[2] == -(-37 // hook[1])


@pytest.mark.parametrize("star", [False, True])
@pytest.mark.parametrize("B", [1, 33])
def test_one_labelling_and_a_chunk_plus_one(B, star):
    x, y, recip, isd, lab, parts = case("mixed")
    score, tot = model.scores(parts, star)
    sums = gpu_run(x, y, recip, isd, lab[:B], star)[0]
    assert sums.shape == (B, x.shape[1])
    assert ratio(sums, score[:B], tot[:B]) <= TOL
    # a labelling is one column of the B operand and one lane of the walk: the
    # same bits in any company
    assert np.array_equal(sums, default_run("mixed", star)[0][0][:B])


@pytest.mark.parametrize("star", [False, True])
def test_feature_subset_matches_a_fresh_plan(star):
    x, y, recip, isd, lab, _ = case("mixed")
    feat = np.array([1, 3, 7, 19, 22, 25, 30, 38])
    sub = gpu_run(x, y, recip, isd, lab, star, feat=feat)[0]
    xs = np.ascontiguousarray(x[:, feat])
    fresh = gpu_run(xs, y, recip[feat], isd[feat], lab, star)[0]
    score, tot = model.scores(model.score_parts(xs, lab, recip[feat], isd[feat]), star)
    assert sub.shape == (37, feat.size)
    assert ratio(sub, score, tot) <= TOL and ratio(fresh, score, tot) <= TOL
    assert float(np.max(np.abs(sub - fresh) / tot)) <= 2 * TOL


@pytest.mark.parametrize("star", [False, True])
@pytest.mark.parametrize("f64", [0, 1])
def test_both_distance_routes_decide_as_the_model(hooks, f64, star):
    x, y, recip, isd, lab, parts = case("mixed")
    score, tot = model.scores(parts, star)
    hooks("surf_f64", f64)
    sums, plan, info, _ = gpu_run(x, y, recip, isd, lab, star)
    assert info[1] == parts[4]
    assert ratio(sums, score, tot) <= TOL
    assert np.array_equal(plan[0], plan[1])


@pytest.mark.parametrize("split", [0, 1])
def test_both_star_forms_of_the_plan(hooks, split):
    """A SURF* plan in the dense star form keeps no feature-major operands: the
    call builds them; a plan in the split form lends its own."""
    x, y, recip, isd, lab, parts = case("n130-p270")
    score, tot = model.scores(parts, True)
    hooks("star_split", split)
    sums, plan, info, _ = gpu_run(x, y, recip, isd, lab, True)
    assert ratio(sums, score, tot) <= TOL and info[3] == 1
    assert np.all(np.abs(sums[0] - plan[0]) <= TOL * tot[0])
    assert np.array_equal(plan[0], plan[1])
    assert np.array_equal(sums, default_run("n130-p270", True)[0])


def test_one_shot_call():
    from fastselect_amd import _lib
    x, y, recip, isd, lab, parts = case("mixed")
    n = x.shape[0]
    for star in (False, True):
        score, tot = model.scores(parts, star)
        s = _lib.surf_score_labels("gpu", x, lab, recip, isd, use_star=star)
        assert s.shape == (37, x.shape[1]) and s.dtype == np.float32
        # one float32 rounding of the score on top of the bar
        assert np.all(np.abs(s - score / n) <= TOL * tot / n + 2.0 ** -23 * np.abs(score / n))


def test_refusals_on_the_device():
    import torch
    from fastselect_amd import _lib
    x, y, recip, isd, lab, _ = case("mixed")
    n, p = x.shape
    out = torch.full((37 * p,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()  # the plans run on streams of their own
    call = _lib.lib().fs_plan_surf_score_labels

    def code(pl, labels=lab, B=37):
        lp = labels.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        try:
            return call(pl._h, lp, ctypes.c_int64(B), ctypes.c_void_p(out.data_ptr()))
        finally:
            pl.close()
            torch.cuda.synchronize()

    surf = lambda **kw: _lib.RowsPlan("gpu", "surf", x, y, recip, isd, **kw)  # noqa: E731
    x32 = x.astype(np.float32)
    pl = _lib.RowsPlan("gpu", "relieff", x32, y, recip, isd, k=3, class_probs=np.bincount(y) / n)
    assert code(pl) == _lib.FS_EINVAL
    assert code(_lib.Plan("gpu", x32, y.astype(np.float64), recip, isd)) == _lib.FS_EINVAL
    with _lib.accumulation("reference"):
        pl = surf()
    assert code(pl) == _lib.FS_ENOTSUP
    # a SURF plan's focal rows are fixed at creation (fs_plan_set_rows is
    # MultiSURF's): the slice is a plan created on rows [0, 128)
    assert code(surf(rows=(0, 128))) == _lib.FS_ENOTSUP
    wide = lab.copy()
    wide[35, 0] = 8
    assert code(surf(use_star=True), labels=wide) == _lib.FS_ENOTSUP
    assert code(surf(use_star=True), B=0) == _lib.FS_OK
    assert bool(torch.isnan(out).all())  # nothing was written by any of them
    # plain SURF compares labels by equality only: any code
    assert code(surf(), labels=wide) == _lib.FS_OK
    assert code(surf(use_star=True)) == _lib.FS_OK
    # the two older label calls still refuse a SURF plan with their code
    pl = surf()
    lp = lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    try:
        for name in ("fs_plan_score_labels", "fs_plan_relieff_score_labels"):
            assert getattr(_lib.lib(), name)(pl._h, lp, ctypes.c_int64(37),
                                             ctypes.c_void_p(out.data_ptr())) == _lib.FS_EINVAL
        with pytest.raises(Exception):
            pl.surf_labels_info()
        assert pl.surf_labels_kernel_ms(0) == -1.0
    finally:
        pl.close()
        torch.cuda.synchronize()


def test_estimator_on_the_planted_case():
    from fastselect_amd import SURF, SURFstar
    from test_surf_permutation import planted_check
    for cls in (SURF, SURFstar):
        est = planted_check("gpu", cls)
        assert est.effective_backend_ == "gpu" and est.devices_ == [0]
    x, y = model.mixed_case()
    with pytest.raises(ValueError, match="one device"):
        SURF(backend="gpu", devices=[0, 0]).permutation_test(x.astype(np.float64), y,
                                                             n_permutations=3)
