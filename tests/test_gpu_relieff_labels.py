"""The ReliefF permutation test on the GPU (fs_relieff_labels.hip) against the
float64 numpy model (relieff_labels_np.py), against fresh plans and against
itself, on both routes: the fast route (k_rfl_prefix, k_rfl_walk, then
k_lab_score / k_lab_reduce) and the general route (relieff_select_update per
labelling on the resident keys).

Accuracy bar.  A score is Miss_f - Hit_f, two sums of non-negative terms, so
each sum's relative error is bounded by its terms': a term is |a - b| of two
float32 pass-2 operands (each rounded once, ~6e-8 of the feature's range)
times a weight (float64 on the general route; rounded once to float32, 6e-8,
and summed in float32 chains of at most 256 records on the fast route).  Per
entry |S_gpu - S_model| <= 1e-5 T with T = Miss_f + Hit_f, the project's
parity bar on the two non-cancelling sums; relative to the score itself it
would mean nothing on permuted labels, where the score cancels to noise.  At
these n one wrong neighbour moves an entry by about 1 / (n k) of that scale,
far above the bar: fast against general on the same plan catches a wrong tie
order, a wrong exact key or a wrong prefix.  Largest ratio seen on an MI355X
over the 36 labellings, automatic route / general route: 2.4e-8 / 4.8e-9
(mixed), 3.1e-8 / 2.1e-15 (discrete), 2.1e-8 / 1.0e-8 (duplicates), 1.9e-8 /
5.1e-9 (three-class), 2.3e-8 / 3.3e-9 (multi-block); fast against general on
the same plan: 3.1e-8 at most.

Fresh-plan bar.  A general-route row b runs the kernels, and the order, of
fs_plan_score of a plan created with labelling b; the codes of a labelling
may have gaps where the fresh plan's are compact, which changes no sum.  Held
to 1e-12 T; seen on an MI355X: exactly 0 on every shape.

Regrouping bar.  labels_chunk and labels_seg_len only regroup float64 sums of
the device's own float32 partials (cut per group of 256 records; a labelling
is one column of the MFMA's B operand): 1e-12 T against the default run.

The fast route must really run: on the default run of every shape the info
reports 35 fast-route labellings, 1 general-route labelling (the one with a
4-member class) and 0 overflows.  The chance that a class has fewer than k
members among a row's first L candidates is the hypergeometric tail the test
computes first: 7.5e-10 per (row, labelling) on mixed (classes of 159 / 141,
L = 64), 1.8e-11 on three-class, below 1e-20 elsewhere, 0 where the prefix
holds the whole row (discrete) -- at most 8e-6 expected overflows per run.
"""
import ctypes

import numpy as np
import pytest

import relieff_labels_np as model

pytestmark = pytest.mark.gpu

TOL = 1e-5
ADD_TOL = 1e-12

_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    from fastselect_amd import _lib
    assert _lib.device_count() >= 1, "no HIP device visible: GPU tests cannot run"


# name -> (n, continuous columns, discrete columns, k)
SHAPES = {
    "mixed": (300, 20, 20, 10),
    # keys tie in every row: numba's order decides the neighbours
    "discrete": (130, 0, 64, 5),
    # 10 duplicated rows: exact ties between continuous keys
    "duplicates": (130, 64, 0, 5),
    # class shares .5 / .3 / .2
    "three-class": (300, 20, 20, 5),
    # several 64-row blocks of the update, three feature blocks
    "multi-block": (600, 100, 40, 10),
}


def case(name, oracle):
    """(x, y_enc, recip, isd, k, labellings, miss, hit, score), once per session."""
    if name not in _CACHE:
        n, pc, pd, k = SHAPES[name]
        if name == "duplicates":
            x, y = model.duplicates_case(n, pc)
        else:
            x, y = model.mixed_case(n, pc, pd)
        if name == "three-class":
            y = np.digitize(x[:, 3], np.quantile(x[:, 3], [0.5, 0.8])).astype(np.float64)
            assert np.bincount(y.astype(int)).tolist() == [150, 90, 60]
        y_enc, recip, isd, _ = model.preprocess(x, y)
        assert int(isd.sum()) == pd
        lab = model.labellings(y_enc)
        assert lab.shape == (36, n) and np.sum(lab[35] == 5) == 4
        parts = model.score_parts(x, lab, recip, isd, k, argsort=oracle.numba_argsort)[:3]
        _CACHE[name] = (x, y_enc, recip, isd, k, lab) + parts
    return _CACHE[name]


def make_plan(x, lab_b, recip, isd, k):
    """A GPU plan with labelling lab_b as y, inputs formed as the estimator
    forms them (compact codes, float32 class shares)."""
    from fastselect_amd import _lib
    _, enc, cnt = np.unique(lab_b, return_inverse=True, return_counts=True)
    return _lib.RowsPlan("gpu", "relieff", x, enc.astype(np.int32), recip, isd, k=k,
                         class_probs=(cnt / lab_b.size).astype(np.float32))


def plan_score(pl):
    import torch
    out = torch.full((pl.n_kept,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()  # the plan runs on a stream of its own
    pl.score(out.data_ptr())
    return out.cpu().numpy()


def plan_labels(pl, lab):
    import torch
    out = torch.full((lab.shape[0] * pl.n_kept,), float("nan"), dtype=torch.float64,
                     device="cuda")
    torch.cuda.synchronize()
    pl.score_labels(lab, out.data_ptr())
    return out.cpu().numpy().reshape(lab.shape[0], pl.n_kept)


def gpu_run(x, y_enc, recip, isd, k, lab, feat=None, twice=False, **hooks):
    """One plan: score, score_labels (once or twice, under the test hooks),
    score.  Returns (sums or the list of two, the plan's scores before /
    after, info, kernel ms)."""
    from fastselect_amd import _lib
    pl = make_plan(x, y_enc, recip, isd, k)
    try:
        if feat is not None:
            pl.set_features(feat)
            before = None  # score_labels needs no earlier score
        else:
            before = plan_score(pl)
        with _lib.test_hooks(**hooks):
            outs = [plan_labels(pl, lab) for _ in range(2 if twice else 1)]
        info, ms = pl.labels_info(), [pl.labels_kernel_ms(w) for w in range(4)]
        after = plan_score(pl)
        return (outs if twice else outs[0]), (before, after), info, ms
    finally:
        pl.close()


def default_run(name, oracle):
    if ("run", name) not in _CACHE:
        _CACHE["run", name] = gpu_run(*case(name, oracle)[:6], twice=True)
    return _CACHE["run", name]


def general_run(name, oracle):
    if ("general", name) not in _CACHE:
        _CACHE["general", name] = gpu_run(*case(name, oracle)[:6], rf_labels_route=1)
    return _CACHE["general", name]


# the depth the rule picks: the smallest of 64 / 128 / 256 that covers
# min(ceil(3 k / smallest class share), n - 1) of y
DEPTH = {"mixed": 64, "discrete": 256, "duplicates": 64, "three-class": 128, "multi-block": 128}


def overflow_tail(name, y_enc):
    """The largest chance over y's classes that fewer than k of a class's
    other members are among a row's first L candidates (0 when the prefix
    holds the whole row)."""
    from scipy.stats import hypergeom
    n, _, _, k = SHAPES[name]
    L = DEPTH[name]
    if L >= n - 1:
        return 0.0
    return max(float(hypergeom.cdf(k - 1, n - 1, c - 1, L)) for c in np.bincount(y_enc))


def ratio(s, ref, miss, hit):
    return float(np.max(np.abs(s - ref) / (miss + hit)))


@pytest.mark.parametrize("name", list(SHAPES))
def test_scores_match_the_model_on_both_routes(name, oracle):
    x, y_enc, recip, isd, k, lab, miss, hit, score = case(name, oracle)
    n = x.shape[0]
    tail = overflow_tail(name, y_enc)
    print(f"{name}: overflow chance per (row, labelling) {tail:.2e}")
    assert tail * n * 35 <= 1e-4
    (sums, again), (before, after), info, ms = default_run(name, oracle)
    gen, (gb, ga), ginfo, gms = general_run(name, oracle)
    assert sums.shape == score.shape and np.all(np.isfinite(sums))
    assert np.all(miss + hit > 0)
    r, rg = ratio(sums, score, miss, hit), ratio(gen, score, miss, hit)
    rf = ratio(sums, gen, miss, hit)
    print(f"{name}: max |S - S_model| / T automatic {r:.3e}, general {rg:.3e}; "
          f"fast against general {rf:.3e}")
    assert r <= TOL and rg <= TOL and rf <= TOL
    # the fast route really ran: y and its 34 permutations on it, the
    # labelling with a 4-member class on the general route, no overflow
    assert info == (35, 1, 0, DEPTH[name])
    assert all(m > 0 for m in ms)
    assert ginfo == (0, 36, 0, 0) and gms[3] > 0 and gms[:3] == [0.0, 0.0, 0.0]
    assert np.array_equal(sums[35], gen[35])
    # the same call twice, and the plan's own score before and after
    assert np.array_equal(sums, again)
    assert before.any() and np.array_equal(before, after) and np.array_equal(gb, ga)
    assert np.array_equal(gen[0], before)


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_general_row_is_a_fresh_plans_score(name, oracle):
    x, y_enc, recip, isd, k, lab, miss, hit, score = case(name, oracle)
    sums = general_run(name, oracle)[0]
    worst = 0.0
    for b in range(lab.shape[0]):
        pl = make_plan(x, lab[b], recip, isd, k)
        try:
            fresh = plan_score(pl)
        finally:
            pl.close()
        worst = max(worst, float(np.max(np.abs(sums[b] - fresh) / (miss[b] + hit[b]))))
    print(f"{name}: max |S_b - S_fresh| / (Miss + Hit) = {worst:.3e} "
          f"({'exactly 0' if worst == 0 else 'not 0'})")
    assert worst <= ADD_TOL


def test_a_capped_prefix_overflows_and_is_rerun(oracle):
    x, y_enc, recip, isd, k, lab, miss, hit, score = case("mixed", oracle)
    sums, _, info, _ = gpu_run(x, y_enc, recip, isd, k, lab, rf_labels_depth_cap=12)
    print(f"depth cap 12: info {info}")
    assert info[0] == 35 and info[1] == 1 and info[2] > 0
    assert ratio(sums, score, miss, hit) <= TOL
    # a rerun row is a general-route row, bit for bit: at least the reruns and
    # the labelling the rule sent there (a fast-route row shares no bits with
    # its general-route twin: float32 weights and MFMA partials)
    gen = general_run("mixed", oracle)[0]
    same = sum(bool(np.array_equal(sums[b], gen[b])) for b in range(lab.shape[0]))
    assert same >= info[1] + info[2]
    base = default_run("mixed", oracle)[0][0]
    moved = [b for b in range(35) if not np.array_equal(sums[b], base[b])]
    assert len(moved) >= info[2] and all(np.array_equal(sums[b], gen[b]) for b in moved)


@pytest.mark.parametrize("depth", [128, 256])
def test_deeper_prefixes(depth, oracle):
    x, y_enc, recip, isd, k, lab, miss, hit, score = case("mixed", oracle)
    sums, _, info, _ = gpu_run(x, y_enc, recip, isd, k, lab, rf_labels_depth=depth)
    assert info == (35, 1, 0, depth)
    assert ratio(sums, score, miss, hit) <= TOL
    assert ratio(sums, default_run("mixed", oracle)[0][0], miss, hit) <= TOL


@pytest.mark.parametrize("hook", [("labels_chunk", 5), ("labels_chunk", 7),
                                  ("labels_seg_len", 1), ("labels_seg_len", 3)])
def test_chunks_and_segments_regroup_float64_sums_only(hook, oracle):
    x, y_enc, recip, isd, k, lab, miss, hit, score = case("multi-block", oracle)
    ref = default_run("multi-block", oracle)[0][0]
    sums, _, info, _ = gpu_run(x, y_enc, recip, isd, k, lab, **{hook[0]: hook[1]})
    assert info == (35, 1, 0, DEPTH["multi-block"])
    assert ratio(sums, score, miss, hit) <= TOL
    d = ratio(sums, ref, miss, hit)
    print(f"{hook}: max |S - S_default| / (Miss + Hit) = {d:.3e}")
    assert d <= ADD_TOL


def test_feature_subset_matches_a_fresh_plan(oracle):
    x, y_enc, recip, isd, k, lab = case("mixed", oracle)[:6]
    feat = np.array([1, 3, 7, 19, 22, 25, 30, 38])
    sub, (_, after), info, _ = gpu_run(x, y_enc, recip, isd, k, lab, feat=feat)
    xs = np.ascontiguousarray(x[:, feat])
    fresh = gpu_run(xs, y_enc, recip[feat], isd[feat], k, lab)[0]
    miss, hit, score = model.score_parts(xs, lab, recip[feat], isd[feat], k,
                                         argsort=oracle.numba_argsort)[:3]
    assert sub.shape == (36, feat.size) and info[:3] == (35, 1, 0)
    assert ratio(sub, score, miss, hit) <= TOL and ratio(fresh, score, miss, hit) <= TOL
    assert ratio(sub, fresh, miss, hit) <= 2 * TOL
    assert ratio(sub[:1], after[None, :], miss[:1], hit[:1]) <= TOL


def test_one_shot_call(oracle):
    from fastselect_amd import _lib
    x, y_enc, recip, isd, k, lab, miss, hit, score = case("mixed", oracle)
    n = x.shape[0]
    s = _lib.relieff_score_labels("gpu", x, lab, recip, isd, k)
    assert s.shape == (36, x.shape[1]) and s.dtype == np.float32
    assert np.all(np.abs(s - score / n) <= TOL * (miss + hit) / n)
    sums = default_run("mixed", oracle)[0][0]
    assert np.array_equal(s, (sums / n).astype(np.float32))  # the same route, the same bits


def test_refusals_on_the_device(oracle):
    import torch
    from fastselect_amd import _lib
    x, y_enc, recip, isd, k, lab = case("mixed", oracle)[:6]
    n, p = x.shape
    out = torch.full((36 * p,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    probs = (np.bincount(y_enc) / n).astype(np.float32)

    def code(pl, labels=lab, B=36):
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        try:
            return _lib.lib().fs_plan_relieff_score_labels(
                pl._h, labels.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.c_int64(B),
                ctypes.c_void_p(out.data_ptr()))
        finally:
            pl.close()
            torch.cuda.synchronize()

    relieff = lambda **kw: _lib.RowsPlan("gpu", "relieff", x, y_enc, recip, isd, k=k,  # noqa: E731
                                         class_probs=probs, **kw)
    assert code(_lib.Plan("gpu", x, y_enc.astype(np.float64), recip, isd)) == _lib.FS_EINVAL
    assert code(_lib.RowsPlan("gpu", "surf", x, y_enc, recip, isd)) == _lib.FS_EINVAL
    assert code(relieff(rows=(0, 128))) == _lib.FS_ENOTSUP
    with _lib.accumulation("reference"):
        pl = relieff()
    assert code(pl) == _lib.FS_ENOTSUP
    one = lab.copy()
    one[20] = 0
    assert code(relieff(), labels=one) == _lib.FS_EINVAL
    wide = lab.copy()
    wide[35, 0] = 64
    assert code(relieff(), labels=wide) == _lib.FS_EINVAL
    assert code(relieff(), B=0) == _lib.FS_OK
    assert bool(torch.isnan(out).all())  # nothing was written by any of them
    pl = relieff()
    try:
        with pytest.raises(ValueError):
            pl.labels_info()
        assert pl.labels_kernel_ms(3) == -1.0
    finally:
        pl.close()


def test_estimator_on_the_planted_case():
    from fastselect_amd import ReliefF
    from test_relieff_permutation import planted_check
    est = planted_check("gpu")
    assert est.effective_backend_ == "gpu" and est.devices_ == [0]
    x, y = model.mixed_case()
    with pytest.raises(ValueError, match="one device"):
        ReliefF(backend="gpu", devices=[0, 0]).permutation_test(x, y, n_permutations=3)
