"""The MultiSURF permutation test on the GPU (fs_labels.hip: k_lab_count /
k_lab_fill, k_lab_counts, k_lab_weights, k_lab_score) against the float64 numpy model
(multisurf_labels_np.py) and against itself.

Accuracy bar.  A score is Miss_f - Hit_f, two sums of non-negative terms, so
each sum's relative error is bounded by its terms': a term is |a - b| of two
float32 pass-2 operands (each rounded once, ~6e-8 of the feature's range)
times a float32 weight (6e-8), summed in float32 chains of at most 256 pairs
and then in float64.  Per entry |S_gpu - S_model| <= 1e-5 (Miss_f + Hit_f),
the project's parity bar on the two non-cancelling sums; relative to the score
itself it would mean nothing on permuted labels, where the score cancels to
noise.  Largest ratio |S_gpu - S_model| / (Miss_f + Hit_f) seen on an MI355X
over the 37 labellings: 2.2e-7 (mixed), 1.6e-7 (n130-p270), 1.9e-7
(continuous-p64), 1.7e-7 (discrete-p64), 6.9e-8 (n600-p140).

Regrouping bar.  labels_chunk and labels_seg_len only regroup float64 sums of
the device's own float32 partials (the partials are cut per tile, and a
labelling is one column of the MFMA's B operand).  A float64 sum of terms of
total size T = Miss_f + Hit_f moves by a few 2^-53 T when regrouped, so those
results are held to 1e-12 T (seen on an MI355X: exactly 0 -- float64 sums of a
few thousand float32 values are exact).  Relative to the entry itself the
bound could not hold by construction: among 10^4 null entries some cancel to
1e-6 T.
"""
import ctypes

import numpy as np
import pytest

import multisurf_labels_np as model

pytestmark = pytest.mark.gpu

TOL = 1e-5
ADD_TOL = 1e-12

_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    from fastselect_amd import _lib
    assert _lib.device_count() >= 1, "no HIP device visible: GPU tests cannot run"


# name -> (n, continuous columns, discrete columns), as test_gpu_stir.py
SHAPES = {
    "mixed": (300, 20, 20),
    "n130-p270": (130, 200, 70),
    "continuous-p64": (130, 64, 0),
    "discrete-p64": (130, 0, 64),
    "n600-p140": (600, 100, 40),
}


def case(name):
    """(x, y, recip, isd, labellings, miss, hit, score, counts), once per session."""
    if name not in _CACHE:
        n, pc, pd = SHAPES[name]
        x, y = model.mixed_case(n, pc, pd)
        recip, isd = model.preprocess(x)
        assert int(isd.sum()) == pd
        lab = model.labellings(y)
        _CACHE[name] = (x, y, recip, isd, lab) + model.score_parts(x, lab, recip, isd)
    return _CACHE[name]


def gpu_run(x, y, recip, isd, lab, feat=None, twice=False):
    """One job: step, score_labels (float64 sums through the plan), step.
    Returns (sums[B, k] or the list of two, step scores before / after, the
    step's counts[n, 2], weighted pairs before / after)."""
    import torch
    from fastselect_amd.parallel import ShardedMultiSURF
    job = ShardedMultiSURF(x, y, recip, isd, backend="gpu", shard=False)
    try:
        if feat is not None:
            job.set_features(feat)
        s0, p0 = job.step().cpu().numpy(), job.weighted_pairs()
        counts = job.counts.cpu().numpy().reshape(-1, 2).astype(np.int64)
        k = job.plan.n_kept
        outs = []
        for _ in range(2 if twice else 1):
            with job._on_stream():
                out = torch.full((lab.shape[0] * k,), float("nan"), dtype=torch.float64,
                                 device=job.tdev)
                job.plan.score_labels(lab, out.data_ptr())
            outs.append(out.cpu().numpy().reshape(lab.shape[0], k))
        s1, p1 = job.step().cpu().numpy(), job.weighted_pairs()
        return (outs if twice else outs[0]), (s0, s1), counts, (p0, p1)
    finally:
        job.close()


def default_run(name):
    if ("run", name) not in _CACHE:
        _CACHE[("run", name)] = gpu_run(*case(name)[:5], twice=name == "mixed")
    return _CACHE[("run", name)]


def ratio(s, score, miss, hit):
    return float(np.max(np.abs(s - score) / (miss + hit)))


@pytest.mark.parametrize("name", list(SHAPES))
def test_scores_match_the_model(name):
    x, y, recip, isd, lab, miss, hit, score, counts = case(name)
    sums, steps, cn, _ = default_run(name)
    if name == "mixed":
        sums = sums[0]
    # the decisions first: labelling 0 is y, the plan's counts are the model's
    assert np.array_equal(cn, counts[0])
    assert sums.shape == score.shape and np.all(np.isfinite(sums))
    assert np.all(miss[:-1] + hit[:-1] > 0)
    r = ratio(sums, score, miss, hit)
    print(f"{name}: max |S_gpu - S_model| / (Miss + Hit) = {r:.3e}")
    assert r <= TOL
    # the single-sample class has no hit term of its own, the all-equal
    # labelling no miss term at all: its scores are minus the hit part
    assert np.all(counts[35][x.shape[0] // 2] == (0, counts[35][x.shape[0] // 2].sum()))
    assert np.all(miss[36] == 0) and np.all(sums[36] <= 0)
    # row 0 against the step of the same plan (float32 scores, divided by n)
    n = x.shape[0]
    assert np.all(np.abs(sums[0] / n - steps[0]) <= TOL * (miss[0] + hit[0]) / n)


def test_pass2_is_untouched_and_the_call_is_deterministic():
    sums, steps, _, pairs = default_run("mixed")
    assert np.array_equal(steps[0], steps[1])
    assert pairs[0] == pairs[1] and pairs[0] > 0
    assert np.array_equal(sums[0], sums[1])


@pytest.mark.parametrize("hook", [("labels_chunk", 5), ("labels_seg_len", 1),
                                  ("labels_seg_len", 3), ("both", 0)])
def test_chunks_and_segments_regroup_float64_sums_only(hooks, hook):
    x, y, recip, isd, lab, miss, hit, score, _ = case("n600-p140")
    ref = default_run("n600-p140")[0]
    if hook[0] == "both":
        hooks("labels_chunk", 7)
        hooks("labels_seg_len", 15)  # one workgroup walks all 15 tiles
    else:
        hooks(*hook)
    sums = gpu_run(x, y, recip, isd, lab)[0]
    assert ratio(sums, score, miss, hit) <= TOL
    d = float(np.max(np.abs(sums - ref) / (miss + hit)))
    print(f"{hook}: max |S - S_default| / (Miss + Hit) = {d:.3e}")
    assert d <= ADD_TOL


def test_feature_subset_matches_a_fresh_plan():
    x, y, recip, isd, lab = case("mixed")[:5]
    feat = np.array([1, 3, 7, 19, 22, 25, 30, 38])
    sub = gpu_run(x, y, recip, isd, lab, feat=feat)[0]
    xs = np.ascontiguousarray(x[:, feat])
    fresh = gpu_run(xs, y, recip[feat], isd[feat], lab)[0]
    miss, hit, score, _ = model.score_parts(xs, lab, recip[feat], isd[feat])
    assert sub.shape == (37, feat.size)
    assert ratio(sub, score, miss, hit) <= TOL and ratio(fresh, score, miss, hit) <= TOL
    assert float(np.max(np.abs(sub - fresh) / (miss + hit))) <= 2 * TOL


@pytest.mark.parametrize("B", [1, 33])
def test_one_labelling_and_a_chunk_plus_one(B):
    x, y, recip, isd, lab, miss, hit, score, _ = case("mixed")
    sums = gpu_run(x, y, recip, isd, lab[:B])[0]
    assert sums.shape == (B, x.shape[1])
    assert ratio(sums, score[:B], miss[:B], hit[:B]) <= TOL
    # a labelling is one column of the B operand: the same bits in any company
    assert np.array_equal(sums, default_run("mixed")[0][0][:B])


def test_one_shot_and_job_wrappers():
    from fastselect_amd import _lib
    from fastselect_amd.parallel import ShardedMultiSURF
    x, y, recip, isd, lab, miss, hit, score, _ = case("mixed")
    n = x.shape[0]
    s = _lib.multisurf_score_labels("gpu", x, lab, recip, isd)
    assert s.shape == (37, x.shape[1]) and s.dtype == np.float32
    assert np.all(np.abs(s - score / n) <= TOL * (miss + hit) / n)
    job = ShardedMultiSURF(x, y, recip, isd, backend="gpu", shard=False)
    try:
        with pytest.raises(ValueError, match="step"):
            job.score_labels(lab)
        step = job.step().cpu().numpy()
        t = job.score_labels(lab).cpu().numpy()
        ms = [job.plan.labels_kernel_ms(w) for w in range(3)]
    finally:
        job.close()
    assert t.shape == (37, x.shape[1]) and t.dtype == np.float32
    assert np.all(np.abs(t - score / n) <= TOL * (miss + hit) / n)
    assert np.all(np.abs(t[0] - step) <= TOL * (miss[0] + hit[0]) / n)
    assert all(m > 0 for m in ms)


def test_refusals_on_the_device():
    import torch
    from fastselect_amd import _lib
    x, y, recip, isd, lab = case("mixed")[:5]
    n, p = x.shape
    out = torch.zeros(37 * p, dtype=torch.float64, device="cuda")
    rs = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
    cn = torch.zeros(2 * n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()  # the plans run on streams of their own
    labp = lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))

    def code(pl, select=True, after=None):
        try:
            if select:
                pl.pass1(rs.data_ptr())
                pl.select(rs.data_ptr(), cn.data_ptr())
            if after:
                after(pl)
            return _lib.lib().fs_plan_score_labels(pl._h, labp, ctypes.c_int64(37),
                                                   ctypes.c_void_p(out.data_ptr()))
        finally:
            pl.close()
            torch.cuda.synchronize()

    assert code(_lib.Plan("gpu", x, y, recip, isd), select=False) == _lib.FS_EINVAL
    assert code(_lib.Plan("gpu", x, y, recip, isd, use_star=True)) == _lib.FS_ENOTSUP
    assert code(_lib.Plan("gpu", x, y, recip, isd, rank=1, world=2)) == _lib.FS_ENOTSUP
    assert code(_lib.Plan("gpu", x, y, recip, isd),
                after=lambda pl: pl.set_rows(0, 100)) == _lib.FS_ENOTSUP
    assert code(_lib.Plan("gpu", x, y, recip, isd),
                after=lambda pl: pl.set_features(np.arange(5))) == _lib.FS_EINVAL
    with _lib.accumulation("reference"):
        pl = _lib.Plan("gpu", x, y, recip, isd)
    assert code(pl) == _lib.FS_ENOTSUP
    yi = y.astype(np.int32)
    pl = _lib.RowsPlan("gpu", "relieff", x, yi, recip, isd, k=3, class_probs=np.bincount(yi) / n)
    assert code(pl, select=False) == _lib.FS_EINVAL
    assert code(_lib.Plan("gpu", x, y, recip, isd)) == _lib.FS_OK


def test_estimator_on_the_planted_case():
    from test_multisurf_permutation import planted_check
    est = planted_check("gpu")
    assert est.effective_backend_ == "gpu" and est.devices_ == [0]
