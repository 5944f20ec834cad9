"""CFS on the GPU (fs_cfs.hip) against the CPU backend and the numpy
restatement (cfs_np.py).

Every SU of the GPU (all rows of fs_cfs_row, and r_cf) must equal the CPU
backend's and the restatement's float32 or be the adjacent float32, at most
1 % of a case's values differing at all: the sides run the same IEEE
operations in the same order except log2 (the device's, libm's, numpy's), so a
float64 difference near 1e-16 moves the float32 rounding by one step at most.
The search on a given matrix is IEEE operations only and must agree bit for
bit between the backends (which also shows that the device's float64 division
and square root are correctly rounded in this build).

Shapes are the smallest at which the kernels can go wrong.  k_cfs_row gives a
pair NB^2 lanes (NB = ceil(states / 4)) and a workgroup 256 / NB^2 columns,
and it stages the anchor's planes 64 words (2048 samples) per chunk;
k_cfs_step takes 256 candidates per workgroup.  So:

* n = 33 / 64 / 203: one over a word boundary, whole words, a ragged word;
  n = 2049: the word loop restages the anchor once;
* p = 1 and 2; p = 255 / 256 / 257 at 3 states (256 columns per workgroup; y
  is one more column), 27 / 28 / 29 at 10 states (28 columns, 4 idle lanes),
  3 / 4 / 5 at 32 states (4 columns);
* 2, 3, 5, 10 and 32 states: 1, 1, 4, 9 and 64 lanes per pair;
* mixed columns: per-column state counts (constant, codes {0, 4}, 2 beside
  32), two constant columns paired (hx + hy < 1e-12 gives 0.0);
* y with 4 classes beside 3-state columns;
* 4, 8, 12, 13, 16, 17, 20, 21, 24, 25, 28 and 29 states at n = 97 and 257
  with a 4-class y (mi_np.GEOMETRY): both ends of every NB = ceil(states / 4),
  so 16-, 25-, 36- and 49-lane pairs, T = 4, 3, 2 and 10, 7, 5 columns per
  workgroup with idle lanes, and state counts with no padding plane; per state
  count p = CPW - 1, CPW, CPW + 1 and 2T + 1; mixed columns with the state
  bound at 21 and at 25;
* n = 2048, 4096 and 4097 (mi_np.LONG): whole staging chunks and two restages;
* fs_cfs_search_matrix at p = 1, 64, 65 (one workgroup, a second one) and
  1000 (four, the last ragged), on random matrices and on matrices in
  multiples of 1/8, where equal merits occur.
"""
import ctypes

import numpy as np
import pytest

import cfs_np
import mdr_np
import mi_np

pytestmark = pytest.mark.gpu

SU_CASES = dict(mi_np.ALL_SHAPES)
SU_CASES["p1"] = lambda: mi_np.uniform(65, 1, 3, 31) + (3,)
SU_CASES["p2"] = lambda: mi_np.uniform(65, 2, 3, 32) + (3,)
for _p, _s in ((255, 3), (256, 3), (257, 3), (27, 10), (28, 10), (29, 10), (3, 32), (4, 32),
               (5, 32)):
    SU_CASES[f"wg_p{_p}_s{_s}"] = (lambda p, s: lambda: mi_np.uniform(65, p, s, 40 + p) + (s,))(
        _p, _s)


@pytest.fixture(scope="module")
def L():
    from fastselect_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    return _lib


def check_su(got, want, what):
    steps = cfs_np.f32_steps(got, want)
    print(what, "float32 steps", steps.max(initial=0), "differing share",
          np.count_nonzero(steps) / max(steps.size, 1))
    assert steps.max(initial=0) <= 1, what
    assert np.count_nonzero(steps) <= 0.01 * steps.size, what


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("name", sorted(SU_CASES))
def test_su_equals_cpu_and_restatement(L, name):
    X, y, S, r_cf, r_ff = cfs_np.su_case(name, SU_CASES[name])
    p = X.shape[1]
    with L.Cfs("cpu", X, y, S) as c:
        c_cf = c.relevance()
        c_rows = np.stack([c.row(f) for f in range(p)])
    with L.Cfs("gpu", X, y, S) as g:
        g_cf = g.relevance()
        g_rows = np.stack([g.row(f) for f in range(p)])
        # the orientation rule: SU(a, c) and SU(c, a) are one computation
        assert np.array_equal(bits(g_rows), bits(g_rows.T)) and not np.diag(g_rows).any()
        # rows taken one by one equal the rows the search caches
        sel, _ = g.search(0.0)
        assert sel.size >= 1
        for f in sel:
            assert np.array_equal(bits(g.row(f)), bits(g_rows[f]))
        up, pack, rel, rows_ms, steps_ms = L.cfs_last_timing()
        assert pack >= 0.0 and rel >= 0.0 and rows_ms >= 0.0 and steps_ms >= 0.0
    check_su(g_cf, r_cf, "r_cf against the restatement")
    check_su(g_cf, c_cf, "r_cf against the CPU backend")
    check_su(g_rows, r_ff, "rows against the restatement")
    check_su(g_rows, c_rows, "rows against the CPU backend")
    if name == "mixed":
        assert g_rows[0, 7] == 0.0  # two constant columns


@pytest.mark.parametrize("eighths", [False, True])
@pytest.mark.parametrize("p", [1, 64, 65, 1000])
def test_search_matrix_equals_cpu_bit_for_bit(L, p, eighths):
    r_cf, r_ff = cfs_np.random_matrix(p, 100 + p, eighths)
    c_sel, c_mer = L.cfs_search_matrix("cpu", r_cf, r_ff)
    g_sel, g_mer = L.cfs_search_matrix("gpu", r_cf, r_ff)
    assert c_sel.size >= 1
    assert np.array_equal(g_sel, c_sel)
    assert np.array_equal(g_mer.view(np.int64), c_mer.view(np.int64))


def test_search_matrix_equals_restatement(L):
    for p, seed, eighths in ((33, 7, False), (40, 4, True)):
        r_cf, r_ff = cfs_np.random_matrix(p, seed, eighths)
        sel, mer, _ = cfs_np.best_first(r_cf, r_ff)
        g_sel, g_mer = L.cfs_search_matrix("gpu", r_cf, r_ff)
        assert list(g_sel) == sel and np.array_equal(g_mer, np.array(mer))


def _handle_results(L, X, y, S):
    with L.Cfs("gpu", X, y, S) as g:
        sel, mer = g.search()
        rows = np.stack([g.row(f) for f in sel])
        return sel, mer, g.relevance(), rows


@pytest.mark.parametrize("key", cfs_np.PLANTED)
def test_planted_selection(L, key):
    from fastselect_amd import CFS
    X, y, S, r_cf, r_ff, sel, mer, kept, merit = cfs_np.planted_case(key)
    gpu = CFS(backend="gpu").fit(X, y)
    cpu = CFS(backend="cpu").fit(X, y)
    assert gpu.effective_backend_ == "gpu"
    assert gpu.selected_indices_.tolist() == sorted(kept)
    assert cpu.selected_indices_.tolist() == sorted(kept)
    assert abs(gpu.merit_ - merit) <= 1e-6 * merit
    assert abs(gpu.merit_ - cpu.merit_) <= 1e-6 * merit
    g_sel, g_mer, g_cf, g_rows = _handle_results(L, X, y, S)
    assert list(g_sel) == sel
    np.testing.assert_allclose(g_mer, mer, rtol=1e-6, atol=0)
    # two fits of one case are bit-identical
    sel2, mer2, cf2, rows2 = _handle_results(L, X, y, S)
    assert np.array_equal(sel2, g_sel) and np.array_equal(mer2.view(np.int64), g_mer.view(np.int64))
    assert np.array_equal(bits(cf2), bits(g_cf)) and np.array_equal(bits(rows2), bits(g_rows))
    if len(sel) >= 6:
        # the row cache starts at 2 rows and grows in the middle of the search
        with L.test_hooks(cfs_rows_cap=2):
            sel3, mer3, cf3, rows3 = _handle_results(L, X, y, S)
            small = CFS(backend="gpu").fit(X, y)
        assert np.array_equal(sel3, g_sel)
        assert np.array_equal(mer3.view(np.int64), g_mer.view(np.int64))
        assert np.array_equal(bits(rows3), bits(g_rows))
        assert small.selected_indices_.tolist() == sorted(kept) and small.merit_ == gpu.merit_


def test_auto_and_state_limits(L):
    from fastselect_amd import CFS
    X, y, _, _, _, _, _, kept, _ = cfs_np.planted_case(cfs_np.PLANTED[0])
    est = CFS(backend="auto").fit(X, y)
    assert est.effective_backend_ == "gpu" and est.selected_indices_.tolist() == sorted(kept)
    rng = np.random.default_rng(3)
    X33 = rng.integers(0, 33, size=(300, 6))
    X33[:33, 0] = np.arange(33)
    y33 = (X33[:, 1] > 16).astype(int)
    with pytest.raises(ValueError, match="GPU backend supports up to 32 unique states/bins."):
        CFS(backend="gpu").fit(X33, y33)
    auto = CFS(backend="auto").fit(X33, y33)
    assert auto.effective_backend_ == "cpu"
    assert auto.selected_indices_.tolist() == CFS(backend="cpu").fit(X33, y33).selected_indices_.tolist()


def test_planes_that_cannot_be_allocated_are_out_of_memory(L):
    """2 words x 2^46 columns x 16 bytes of planes: the out-of-memory code on
    the size alone, before any array is read."""
    lib = L.lib()
    u8p = ctypes.POINTER(ctypes.c_uint8)
    x = np.zeros(16, np.uint8)
    h = ctypes.c_void_p()
    rc = lib.fs_cfs_create(ctypes.byref(h), L.BACKEND_GPU, 0, x.ctypes.data_as(u8p),
                           x.ctypes.data_as(u8p), 33, 1 << 46, 3, 1)
    assert rc == L.FS_EOOM and not h.value


def test_readme_pipeline_cfs_then_mdr(L):
    """The README's pipeline CFS -> MDR on mdr_np.planted(160, 60, pair=(7, 41)).

    That family plants a pair with almost no marginal effect (P(case | g) =
    0.36 / 0.37 / 0.38 for g = 0 / 1 / 2): the largest class correlation of its
    60 columns is r_cf = 0.028, so at the reference's fixed threshold of 0.1 CFS
    selects nothing, as the reference would, and no second stage can follow.
    The README pipeline therefore lowers ``min_r_cf`` as it advises for
    genotype data; at 0.02 the restatement selects 7 columns and keeps 5 (step
    margins >= 9.0e-3, prune gap 1.1e-3, far above a float32 step)."""
    from sklearn.pipeline import Pipeline

    from fastselect_amd import CFS, MDR
    X, y = mdr_np.planted(160, 60, pair=(7, 41))
    r_cf, r_ff = cfs_np.matrices(X, y, 3)
    assert float(r_cf.max()) < 0.1
    assert CFS(backend="gpu").fit(X, y).selected_indices_.size == 0  # the reference's threshold
    sel, _, margins = cfs_np.best_first(r_cf, r_ff, 0.02)
    kept, gap = cfs_np.prune(sel, r_cf, r_ff)
    assert min(margins) >= cfs_np.MARGIN and gap >= cfs_np.MARGIN and len(kept) >= 3
    pipe = Pipeline([("cfs", CFS(backend="gpu", min_r_cf=0.02)), ("mdr", MDR(k=2, backend="gpu"))])
    pipe.fit(X, y)
    cfs = pipe.named_steps["cfs"]
    assert cfs.effective_backend_ == "gpu"
    assert cfs.selected_indices_.tolist() == sorted(kept)
    assert len(pipe.named_steps["mdr"].best_interaction_) == 2
