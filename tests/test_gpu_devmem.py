"""Device-memory ownership of a resident plan (fs_devmem.h): buffers that
grow on demand (the ambiguous-pair list, the pair sums and sort scratch sized
after it, the reference order's temp rows) and the arenas a re-layout or a
re-shard releases.  A plan that grew a buffer, or went through another
feature layout and back, must score bit for bit what a plan that never did
scores.  Shapes: n = 300 (three row blocks, six tiles), p = 96 with a few
discrete columns, unless a test says otherwise.
"""
import numpy as np
import pytest
from sklearn.datasets import make_classification

pytestmark = pytest.mark.gpu
N, P = 300, 96


def _data(n=N, p=P, seed=3):
    X, y = make_classification(n_samples=n, n_features=p, n_informative=8, n_redundant=10,
                               random_state=seed)
    X[:, :3] = np.clip(np.round(X[:, :3]), -2, 2)  # discrete: at most 5 values each
    return X, y


def _multisurf_plan_scores():
    """(score sums, refined pairs) of one MultiSURF step of a fresh plan."""
    import torch

    from fastselect_amd import _lib
    from fastselect_amd.parallel import prepare_inputs
    X, y = _data()
    x, yv, recip, isd = prepare_inputs(X, y, backend="gpu")
    dev = torch.device("cuda", 0)
    rs = torch.zeros(3 * N, dtype=torch.float64, device=dev)
    cnt = torch.zeros(2 * N, dtype=torch.float64, device=dev)
    sc = torch.zeros(P, dtype=torch.float64, device=dev)
    plan = _lib.Plan("gpu", x, yv, recip, isd)
    try:
        torch.cuda.synchronize()  # the plan runs on its own stream
        plan.pass1(rs.data_ptr())
        plan.select(rs.data_ptr(), cnt.data_ptr())
        plan.pass2(cnt.data_ptr(), sc.data_ptr())
        torch.cuda.synchronize()
        return sc.cpu().numpy(), plan.info()[2]
    finally:
        plan.close()


def test_multisurf_pair_list_growth(hooks):
    """A pair list that starts below the step's refined pairs (the list_cap
    hook) grows inside refine_pairs, and the pair sums and the sort scratch
    after it; the scores are those of a list that was large enough at once.
    Where the plan's own 32-bit operands leave fewer than two ambiguous pairs
    at this shape, both runs take 16-bit operands (the q16 hook: 27 pairs)."""
    ref, refined = _multisurf_plan_scores()
    if refined < 2:
        hooks("q16", 1)
        ref, refined = _multisurf_plan_scores()
    cap = max(1, refined // 3)
    print(f"multisurf: {refined} refined pairs, list_cap {cap}")
    assert refined > cap
    hooks("list_cap", cap)
    got, refined2 = _multisurf_plan_scores()
    assert refined2 == refined
    np.testing.assert_array_equal(got, ref)


def _surf_plan_scores():
    """(score sums, refined pairs, float64 route taken) of a fresh SURF plan."""
    import torch

    from fastselect_amd import _lib
    from fastselect_amd.SURF import surf_inputs
    X, y = _data()
    x = np.ascontiguousarray(X, dtype=np.float64)
    isd, recip = surf_inputs(x, 10, "gpu")
    plan = _lib.RowsPlan("gpu", "surf", x, y.astype(np.int32), recip, isd)
    try:
        sums = torch.zeros(P, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        plan.score(sums.data_ptr())
        torch.cuda.synchronize()
        return sums.cpu().numpy(), plan.info()[2], plan.calibration()["surf_f64"]
    finally:
        plan.close()


def test_surf_integer_route_pair_list_growth(hooks):
    """SURF on integer distances (fs_surfint.hip): its list grows to a pair
    per focal row before the row means and again for the decisions."""
    hooks("surf_f64", 0)
    ref, refined, f64 = _surf_plan_scores()
    assert not f64  # the integer route
    cap = max(1, refined // 3)
    print(f"surf: {refined} refined pairs, list_cap {cap}")
    assert refined > cap
    hooks("list_cap", cap)
    got, refined2, f64 = _surf_plan_scores()
    assert not f64 and refined2 == refined
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("kw", [dict(use_star=True), dict(accumulation="reference")],
                         ids=["star_split", "reference"])
def test_resident_job_across_relayouts(kw):
    """A resident job in two tile shards, re-targeted to half the columns and
    back: the layout and shard arenas are released and rebuilt, the growable
    buffers (segment partials, sparse schedule, temp rows) are reused.  The
    first and last steps agree bit for bit, the middle one with a fresh job
    on that subset.  use_star: the star split, sparse pass 2;
    accumulation='reference': the temp rows and decision masks."""
    from fastselect_amd.parallel import ShardedMultiSURF, prepare_inputs
    X, y = _data()
    x, yv, recip, isd = prepare_inputs(X, y, backend="gpu")
    half = np.arange(0, P, 2)

    def job():
        return ShardedMultiSURF(x, yv, recip, isd, backend="gpu", shard=False, shards=2, **kw)

    j = job()
    try:
        first = j.step().cpu().numpy()
        j.set_features(half)
        middle = j.step().cpu().numpy()
        j.set_features(None)
        last = j.step().cpu().numpy()
    finally:
        j.close()
    f = job()
    try:
        f.set_features(half)
        fresh = f.step().cpu().numpy()
    finally:
        f.close()
    assert first.shape == (P,) and middle.shape == (half.size,)
    np.testing.assert_array_equal(last, first)
    np.testing.assert_array_equal(middle, fresh)


def test_relieff_resident_rescore_reference():
    """A resident ReliefF plan in reference order, scored on 40 kept features
    and then on all 300 (p = 300 here: the temp rows are 256-padded, so they
    grow only past 256 kept features): the second score is a fresh plan's."""
    import torch

    from fastselect_amd import _lib
    from fastselect_amd.ReliefF import relieff_inputs
    p = 300
    X, y = _data(p=p, seed=5)
    x, ye, recip, isd, pri = relieff_inputs(X, y, 10, "gpu")

    def plan():
        with _lib.accumulation("reference"):
            return _lib.RowsPlan("gpu", "relieff", x, ye, recip, isd, k=5, class_probs=pri)

    def score(pl):
        sums = torch.zeros(pl.n_kept, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        pl.score(sums.data_ptr())
        torch.cuda.synchronize()
        return sums.cpu().numpy()

    a = plan()
    try:
        a.set_features(np.arange(40))
        narrow = score(a)
        a.set_features(None)
        wide = score(a)
    finally:
        a.close()
    b = plan()
    try:
        fresh = score(b)
    finally:
        b.close()
    assert narrow.shape == (40,) and np.any(narrow != 0)
    np.testing.assert_array_equal(wide, fresh)
