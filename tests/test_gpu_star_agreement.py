"""MultiSURF* jobs whose plans prefer different star forms (ADVICE r6, items 1,
3 and 4).

A GPU MultiSURF* plan scores the far pairs densely (pass 2 weighs every pair
of its tiles) or split (pass 2 weighs the near pairs, the far part of every
pair comes from per-column terms of which a rank adds its column share,
fs_starterm.hip).  The two are one sum only when every plan of a job is in the
same form, and each plan chooses by itself from its device's free memory.
Before this file's change nothing made the plans of a job agree.

The defect, measured once on the parent commit with the plan-level driver
below (two plans, rank 0 split and rank 1 dense, forms set with the star_split
hook before each plan was created), scale-relative error against the oracle:

    mixed 700 x 330, forms (1, 0):        7.04e-01  (top 10 differ)
    three classes 700 x 330, forms (1, 0): 6.91e-01  (top 10 differ)
    (all-split and all-dense, one or two plans: 1.0e-06 .. 1.2e-06)

against the bar of 1e-5: every mixed case below would have failed.

What is checked now (bars: the project's own -- oracle 1e-5 with the same top
10; split against dense 2e-6; plans' sums against the whole 1e-9 split, 1e-6
dense, on the float32 scores as test_split_multisurf_tile_shards and
test_sharded_plans_sum_to_single take them):

  * plans report their form and take the one they are handed
    (fs_plan_star_split / fs_plan_set_star_split), and refuse the split where
    it does not fit;
  * ShardedMultiSURF ranks that prefer different forms end dense, with
    identical bits on every rank;
  * the device workers of a devices= call get one decision made before they
    start (star_dense_ranks hook: the own choice of single plan ranks);
  * stir() / score_labels() still refuse MultiSURF* after a re-targeting;
  * GPU (exact full sort per column) against the CPU backend (binned order) on
    lognormal columns, both against the oracle;
  * empty focal slices in the reference-order rank chain.

Largest errors against the oracle seen on an MI355X:
    part C (agreement), mixed:  1.14e-06 (plans, either form; ranks and device
                                workers 1.14e-06; agreed dense against the
                                one-process split fit 6.7e-08)
    part C (agreement), three:  1.04e-06 (dense against the split fit 1.1e-07)
    part D, lognormal 1500 x 300: GPU 7.43e-07, CPU 7.43e-07, GPU vs CPU 7.4e-08
"""
import os
import warnings

import numpy as np
import pytest

from conftest import assert_parity, scale_rel_err
from test_gpu_starsplit import _data, _fit
from test_refacc import assert_bitexact, verdict_case

pytestmark = pytest.mark.gpu

N, P, SEED = 700, 330, 12
_CACHE = {}


@pytest.fixture(scope="module")
def F():
    import fastselect_amd
    from fastselect_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    return fastselect_amd


def case(kind, oracle):
    """(X, y, prepared inputs, oracle scores) of the 700 x 330 case, once."""
    if kind not in _CACHE:
        from fastselect_amd.parallel import prepare_inputs
        X, y = _data(kind, n=N, p=P, seed=SEED)
        ref = oracle.multisurf_scores(X, y, use_star=True)
        ref.setflags(write=False)
        _CACHE[kind] = (X, y, prepare_inputs(X, y, 10, "gpu", 0), ref)
    return _CACHE[kind]


def one_gpu_fit(F, kind, oracle):
    """The single-process GPU fit of a case (its own choice of form), once."""
    key = ("fit", kind)
    if key not in _CACHE:
        X, y = case(kind, oracle)[:2]
        _CACHE[key] = _fit(F, "multisurf", X, y)
        _CACHE[key].setflags(write=False)
    return _CACHE[key]


def note(what, got, ref):
    print(f"[star agreement] {what}: {scale_rel_err(got, ref):.3e}")


# ---- C1: plan level ---------------------------------------------------------

def run_plans(inputs, world, form, start=None):
    """The step of `world` plans as a caller with its own collective drives it
    (test_gpu.py::test_sharded_plans_sum_to_single): partial row statistics,
    counts and scores summed over the plans.  Every plan is put into `form`
    with set_star_split; `start` (the star_split hook while the plans are
    created) makes that a real re-targeting.  Returns float64 scores."""
    import torch

    from fastselect_amd import _lib
    x, y, recip, isd = inputs
    n, p = x.shape
    if start is not None:
        _lib.set_test_hook("star_split", start)
    try:
        plans = [_lib.Plan("gpu", x, y, recip, isd, use_star=True, rank=rk, world=world)
                 for rk in range(world)]
    finally:
        _lib.set_test_hook("reset")
    try:
        for pl in plans:
            if start is not None:
                assert pl.star_split() == start
            pl.set_star_split(form)
            assert pl.star_split() == form
        rs = [torch.zeros(3 * n, dtype=torch.float64, device="cuda") for _ in plans]
        for pl, b in zip(plans, rs):
            pl.pass1(b.data_ptr())
        rsum = sum(rs)
        cn = [torch.zeros(2 * n, dtype=torch.float64, device="cuda") for _ in plans]
        for pl, b in zip(plans, cn):
            pl.select(rsum.data_ptr(), b.data_ptr())
        csum = sum(cn)
        sc = [torch.zeros(p, dtype=torch.float64, device="cuda") for _ in plans]
        for pl, b in zip(plans, sc):
            pl.pass2(csum.data_ptr(), b.data_ptr())
        torch.cuda.synchronize()
        return (sum(sc) / n).cpu().numpy()
    finally:
        for pl in plans:
            pl.close()


def whole(oracle, form):
    """One plan over every tile, created in `form` by its own hook-free path
    (the split is the plan's own choice at this size; dense through the call)."""
    key = ("whole", form)
    if key not in _CACHE:
        _CACHE[key] = run_plans(case("mixed", oracle)[2], 1, form)
        _CACHE[key].setflags(write=False)
    return _CACHE[key]


def f32(a):
    return np.asarray(a, dtype=np.float32)


@pytest.mark.parametrize("world", [2, 3])
def test_forms_hold_and_are_reported(F, oracle, world):
    ref = case("mixed", oracle)[3]
    out = {}
    for form in (1, 0):
        # created in the other form, so that the call lays the plan out again
        out[form] = run_plans(case("mixed", oracle)[2], world, form, start=1 - form)
        one = whole(oracle, form)
        note(f"world {world} form {form} vs one plan", f32(out[form]), f32(one))
        note(f"world {world} form {form} vs oracle", out[form], ref)
        assert scale_rel_err(f32(out[form]), f32(one)) <= (1e-9 if form else 1e-6)
        assert_parity(out[form], ref, 1e-5, k=10)
    note(f"world {world} split vs dense", out[1], out[0])
    assert scale_rel_err(out[1], out[0]) <= 2e-6
    assert scale_rel_err(whole(oracle, 1), whole(oracle, 0)) <= 2e-6


def test_one_plan_keeps_its_bits_across_forms(F, oracle):
    """split -> dense -> split on one plan returns the first split's bits, and
    the dense step in between is the dense plan's: nothing of the other form
    is left behind."""
    import torch

    from fastselect_amd import _lib
    x, y, recip, isd = case("mixed", oracle)[2]
    n, p = x.shape
    pl = _lib.Plan("gpu", x, y, recip, isd, use_star=True)
    rs = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
    cn = torch.zeros(2 * n, dtype=torch.float64, device="cuda")
    sc = torch.zeros(p, dtype=torch.float64, device="cuda")
    got = []
    try:
        assert pl.star_split() == 1  # the plan's own choice at this size
        for form in (1, 0, 1, 0):
            pl.set_star_split(form)
            assert pl.star_split() == form
            pl.pass1(rs.data_ptr())
            pl.select(rs.data_ptr(), cn.data_ptr())
            pl.pass2(cn.data_ptr(), sc.data_ptr())
            torch.cuda.synchronize()
            got.append((sc / n).cpu().numpy())
    finally:
        pl.close()
    np.testing.assert_array_equal(got[0], got[2])
    np.testing.assert_array_equal(got[1], got[3])
    np.testing.assert_array_equal(got[0], whole(oracle, 1))
    np.testing.assert_array_equal(got[1], whole(oracle, 0))


def test_plans_that_never_split_report_dense(F, oracle):
    from fastselect_amd import _lib
    from fastselect_amd.ReliefF import relieff_inputs
    X, y = case("mixed", oracle)[:2]
    x, yv, recip, isd = case("mixed", oracle)[2]
    pl = _lib.Plan("gpu", x, yv, recip, isd, use_star=False)
    try:
        assert pl.star_split() == 0
        pl.set_star_split(0)
        with pytest.raises(ValueError, match="star split"):
            pl.set_star_split(1)
        assert pl.star_split() == 0
    finally:
        pl.close()
    with _lib.accumulation("reference"):
        pl = _lib.Plan("gpu", x, yv, recip, isd, use_star=True)
    try:
        assert pl.star_split() == 0
        with pytest.raises(ValueError, match="star split"):
            pl.set_star_split(1)
    finally:
        pl.close()
    x32, yenc, rrecip, risd, probs = relieff_inputs(X, y, 10, "gpu")
    pl = _lib.RowsPlan("gpu", "relieff", x32, yenc, rrecip, risd, k=5, class_probs=probs)
    try:
        assert pl.star_split() == 0
        with pytest.raises(ValueError):
            pl.set_star_split(1)
    finally:
        pl.close()


def test_split_where_it_does_not_fit_is_an_error(F):
    """More than 8 classes: the plan is dense by itself and refuses the split
    (an error, not a silent dense plan); it still scores."""
    from fastselect_amd import _lib
    from fastselect_amd.parallel import prepare_inputs
    rng = np.random.default_rng(5)
    X = rng.standard_normal((300, 70))
    y = np.arange(300) % 9
    x, yv, recip, isd = prepare_inputs(X, y, 10, "gpu", 0)
    pl = _lib.Plan("gpu", x, yv, recip, isd, use_star=True)
    try:
        assert pl.star_split() == 0
        with pytest.raises(ValueError, match="star split"):
            pl.set_star_split(1)
        assert pl.star_split() == 0
        pl.set_star_split(0)
    finally:
        pl.close()


def test_dense_ranks_hook_sets_the_own_choice_per_rank(F, oracle, hooks):
    """star_dense_ranks: bit r makes the own choice of a plan created with
    rank r dense -- what lets the threads of one process disagree."""
    from fastselect_amd import _lib
    x, yv, recip, isd = case("mixed", oracle)[2]
    hooks("star_dense_ranks", 0b010)
    got = []
    for rk in range(3):
        pl = _lib.Plan("gpu", x, yv, recip, isd, use_star=True, rank=rk, world=3)
        got.append(pl.star_split())
        pl.close()
    assert got == [1, 0, 1]


# ---- C2: ranks that prefer different forms -----------------------------------

RANK_JOBS = {2: [("mixed", (1, 0)), ("mixed", (0, 1)), ("mixed", (1, 1)), ("three", (1, 0))],
             3: [("mixed", (1, 0, 1))]}


def _forms_rank_worker(rank, world, port, out_path):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from fastselect_amd import _lib
    from fastselect_amd.parallel import ShardedMultiSURF, prepare_inputs
    for kind, forms in RANK_JOBS[world]:
        X, y = _data(kind, n=N, p=P, seed=SEED)
        x, yv, recip, isd = prepare_inputs(X, y, 10, "gpu", 0)
        # this rank's own preference; the hook is process-wide and each rank
        # is a process of its own
        _lib.set_test_hook("star_split", forms[rank])
        try:
            job = ShardedMultiSURF(x, yv, recip, isd, use_star=True, backend="gpu", device=0)
        finally:
            _lib.set_test_hook("reset")
        tag = f"{out_path}.{kind}.{''.join(map(str, forms))}.{rank}"
        np.save(tag + ".form.npy", np.array([job.plan.star_split(), job.star_split]))
        np.save(tag + ".npy", job.step().cpu().numpy())
        job.close()
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def rank_runs(tmp_path_factory):
    """The rank jobs of one world size, all in one spawn; the path prefix."""
    done = {}

    def run(world):
        if world not in done:
            import torch.multiprocessing as mp

            from test_gpu_dist import _port
            out = str(tmp_path_factory.mktemp(f"forms{world}") / "s")
            mp.spawn(_forms_rank_worker, args=(world, _port(), out), nprocs=world, join=True)
            done[world] = out
        return done[world]
    return run


@pytest.mark.parametrize("kind,forms", [(k, f) for w in RANK_JOBS for k, f in RANK_JOBS[w]])
def test_ranks_that_prefer_different_forms(F, oracle, rank_runs, kind, forms):
    """Rank r prefers forms[r]; the job runs in the minimum on every rank."""
    world = len(forms)
    out = rank_runs(world)
    want = min(forms)
    tag = f"{out}.{kind}.{''.join(map(str, forms))}"
    got = [np.load(f"{tag}.{r}.npy") for r in range(world)]
    for r in range(world):
        assert np.load(f"{tag}.{r}.form.npy").tolist() == [want, want], f"rank {r}"
        np.testing.assert_array_equal(got[r], got[0])
    ref = case(kind, oracle)[3]
    one = one_gpu_fit(F, kind, oracle)
    note(f"ranks {kind} {forms} vs one process", got[0], one)
    note(f"ranks {kind} {forms} vs oracle", got[0], ref)
    assert scale_rel_err(got[0], one) <= 2e-6
    assert_parity(got[0], ref, 1e-5, k=10)


# ---- C3: device workers that prefer different forms ---------------------------

def _fit_devices(F, X, y, devices):
    from fastselect_amd import _lib
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        est = F.MultiSURF(backend="gpu", use_star=True, devices=devices).fit(X, y)
    return (np.asarray(est.feature_importances_, dtype=np.float64),
            _lib.multisurf_last_star_split())


@pytest.mark.parametrize("dense_ranks,shards", [(0b10, 0), (0b01, 0), (0b10, 2), (0, 0)])
def test_device_workers_that_prefer_different_forms(F, oracle, hooks, dense_ranks, shards):
    """devices=[0, 0]: one decision before the worker threads start, the
    minimum of the workers' own choices (dense_ranks: the workers whose own
    choice is dense; 0: the control, every worker takes the split)."""
    X, y, _, ref = case("mixed", oracle)
    key = ("devices0",)
    if key not in _CACHE:
        _CACHE[key] = _fit_devices(F, X, y, [0])
        _CACHE[key][0].setflags(write=False)
    one, one_form = _CACHE[key]
    assert one_form == 1  # one device, no hook: the split
    if dense_ranks:
        hooks("star_dense_ranks", dense_ranks)
    if shards:
        hooks("shards", shards)  # two shards per worker: four shard-ranks
    got, form = _fit_devices(F, X, y, [0, 0])
    assert form == (0 if dense_ranks else 1)
    note(f"devices dense_ranks {dense_ranks:#b} shards {shards} vs one device", got, one)
    note(f"devices dense_ranks {dense_ranks:#b} shards {shards} vs oracle", got, ref)
    assert scale_rel_err(got, one) <= 2e-6
    assert_parity(got, ref, 1e-5, k=10)


# ---- C4: stir() and score_labels() after a re-targeting -----------------------

@pytest.mark.parametrize("form", [0, 1])
def test_stir_and_labels_still_refuse_the_star(F, oracle, form):
    import torch

    from fastselect_amd import _lib
    x, yv, recip, isd = case("mixed", oracle)[2]
    n, p = x.shape
    rs = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
    cn = torch.zeros(2 * n, dtype=torch.float64, device="cuda")
    s4 = torch.zeros(4 * p, dtype=torch.float64, device="cuda")
    sl = torch.zeros(2 * p, dtype=torch.float64, device="cuda")
    lab = np.stack([yv.astype(np.int32), 1 - yv.astype(np.int32)])
    torch.cuda.synchronize()  # the plan runs on a stream of its own
    pl = _lib.Plan("gpu", x, yv, recip, isd, use_star=True)
    try:
        pl.set_star_split(1 - form)
        pl.set_star_split(form)
        pl.pass1(rs.data_ptr())
        pl.select(rs.data_ptr(), cn.data_ptr())
        with pytest.raises(RuntimeError, match="MultiSURF\\*"):
            pl.stir(s4.data_ptr())
        with pytest.raises(RuntimeError, match="MultiSURF\\*"):
            pl.score_labels(lab, sl.data_ptr())
    finally:
        pl.close()


# ---- D: GPU (full sort) and CPU (binned order) on crowded columns -------------

def test_gpu_and_cpu_backends_on_lognormal_columns(F, oracle):
    X, y = _data("lognormal")
    ref = oracle.multisurf_scores(X, y, use_star=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        gpu = np.asarray(F.MultiSURF(backend="gpu", use_star=True).fit(X, y)
                         .feature_importances_, dtype=np.float64)
        cpu = np.asarray(F.MultiSURF(backend="cpu", use_star=True).fit(X, y)
                         .feature_importances_, dtype=np.float64)
    note("lognormal GPU vs oracle", gpu, ref)
    note("lognormal CPU vs oracle", cpu, ref)
    note("lognormal GPU vs CPU", gpu, cpu)
    assert_parity(gpu, ref, 1e-5, k=10)
    assert_parity(cpu, ref, 1e-5, k=10)
    assert scale_rel_err(gpu, cpu) <= 2e-5  # the triangle of the two bars


# ---- E: empty focal slices in the reference-order rank chain -------------------

REF_JOBS = {2: [(170, 170), (170, 171)], 3: [(170, 172)]}


def _empty_slice_worker(rank, world, port, out_path):
    """test_gpu_refacc._ref_rank_worker's job and data over several row
    ranges in one process group."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from fastselect_amd.parallel import ShardedMultiSURF, prepare_inputs
    X, y = verdict_case("pareto1", 1300, 200, seed=8)
    x, yv, recip, isd = prepare_inputs(X, y, backend="gpu", device=0)
    for rows in REF_JOBS[world]:
        for star in (False, True):
            job = ShardedMultiSURF(x, yv, recip, isd, use_star=star, backend="gpu", device=0,
                                   rows=rows, accumulation="reference")
            assert job.ref_chain and job.world == world and job.plan.star_split() == 0
            tag = f"{out_path}.{rows[0]}.{rows[1]}.{int(star)}.{rank}"
            np.save(tag + ".npy", job.step().cpu().numpy())
            np.save(tag + ".again.npy", job.step().cpu().numpy())
            job.close()
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def empty_slice_runs(tmp_path_factory):
    done = {}

    def run(world):
        if world not in done:
            import torch.multiprocessing as mp

            from test_gpu_dist import _port
            out = str(tmp_path_factory.mktemp(f"empty{world}") / "r")
            mp.spawn(_empty_slice_worker, args=(world, _port(), out), nprocs=world, join=True)
            done[world] = out
        return done[world]
    return run


@pytest.mark.parametrize("world,rows", [(w, r) for w in REF_JOBS for r in REF_JOBS[w]])
def test_empty_focal_slices_in_the_rank_chain(F, oracle, empty_slice_runs, world, rows):
    """rows=(k, k): no rank has a focal row -- zeros, no error.  One or two
    focal rows over more ranks: the last ranks' slices are empty and still
    take part in the chain and the broadcast; every rank ends with the bits of
    the single-process reference-order job over the same rows."""
    from fastselect_amd import _lib
    from fastselect_amd.parallel import prepare_inputs
    out = empty_slice_runs(world)
    X, y = verdict_case("pareto1", 1300, 200, seed=8)
    x, yv, recip, isd = prepare_inputs(X, y, backend="gpu")
    for star in (False, True):
        if rows[0] == rows[1]:
            one = np.zeros(X.shape[1], dtype=np.float32)
        else:
            with _lib.accumulation("reference"):
                sums = _lib.multisurf_score("gpu", x, yv, recip, None, star, isd, rows=rows)
            one = (sums / X.shape[0]).astype(np.float32)
            assert np.any(one != 0)
            assert_bitexact(one, oracle.multisurf_scores(X, y, use_star=star, i_range=rows))
        for r in range(world):
            for tag in ("", ".again"):
                got = np.load(f"{out}.{rows[0]}.{rows[1]}.{int(star)}.{r}{tag}.npy")
                assert_bitexact(got, one)
