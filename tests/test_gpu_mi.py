"""Mutual information and mRMR on the GPU (fs_mi.hip): every contingency
table must equal the CPU backend's and the numpy restatement's exactly, and
every mutual information must lie within 1e-10 of both (the bound is derived
in test_mi.py: about 25x the worst float64 error of the 1024-term sum; a
wrong count moves MI by about 1/n).  Shapes are the smallest at which the
kernels can go wrong.  The scan's tile is T = 16 / ceil(states / 4) columns
and it stages 64 words (2048 samples) per chunk, so:

* n = 33 / 64 / 203: one over a word boundary, whole words, a ragged word;
* p = 17 and 34 at 3 states (T = 16), p = 9 and 18 at 5 states (T = 8),
  p = 130: diagonal tiles, off-diagonal tiles and a ragged last tile (y is one
  more column);
* 2, 5, 10 and 32 states: 1, 4, 9 and 64 lanes per pair, T = 16, 8, 5, 2;
* mixed columns: per-column state counts (constant, codes {0, 4}, 2 beside 32);
* y with 4 classes beside 3-state columns;
* n = 2049: the word loop restages LDS once;
* 4, 8, 12, 13, 16, 17, 20, 21, 24, 25, 28 and 29 states at n = 97 and 257
  with a 4-class y (mi_np.GEOMETRY): both ends of every NB = ceil(states / 4),
  so 16-, 25-, 36- and 49-lane pairs, T = 4, 3, 2 and 10, 7, 5 columns per
  workgroup with idle lanes, and state counts with no padding plane; per state
  count p = CPW - 1, CPW, CPW + 1 and 2T + 1; mixed columns with the state
  bound at 21 and at 25;
* n = 2048, 4096 and 4097 (mi_np.LONG): whole staging chunks and two restages."""
import ctypes

import numpy as np
import pytest

import mi_np

pytestmark = pytest.mark.gpu

TOL = 1e-10


@pytest.fixture(scope="module")
def L():
    from fastselect_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    return _lib


@pytest.mark.parametrize("name", sorted(mi_np.ALL_SHAPES))
def test_matrices_equal_cpu_and_numpy(L, name):
    X, y, S, rel, red, cnt = mi_np.case(name, mi_np.ALL_SHAPES[name])
    gr, gR, gc = L.mi_matrices("gpu", X, y, S, want_counts=True)
    cr, cR, cc = L.mi_matrices("cpu", X, y, S, want_counts=True)
    print(name, "gpu-numpy", max(np.abs(gr - rel).max(), np.abs(gR - red).max()),
          "gpu-cpu", max(np.abs(gr - cr).max(), np.abs(gR - cR).max()))
    assert np.array_equal(gc, cnt)
    assert np.array_equal(gc, cc)
    assert np.abs(gr - rel).max() <= TOL and np.abs(gR - red).max() <= TOL
    assert np.abs(gr - cr).max() <= TOL and np.abs(gR - cR).max() <= TOL
    assert np.array_equal(gR, gR.T) and not np.diag(gR).any()
    # without counts_out the kernel takes the same path but writes no table
    r2, R2 = L.mi_matrices("gpu", X, y, S)
    assert np.array_equal(r2, gr) and np.array_equal(R2, gR)
    up, pack, scan, down = L.mi_last_timing()
    assert scan >= 0.0 and pack >= 0.0


def test_relevance_only(L):
    """redundancy = NULL: only the tiles that hold y run."""
    X, y, S, rel, _, _ = mi_np.case("p34_tile16", mi_np.SHAPES["p34_tile16"])
    lib = L.lib()
    x8 = np.ascontiguousarray(X, dtype=np.uint8)
    y8 = np.ascontiguousarray(y, dtype=np.uint8)
    r = np.zeros(X.shape[1])
    u8p, f64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_double)
    rc = lib.fs_mi_matrices(L.BACKEND_GPU, 0, x8.ctypes.data_as(u8p), y8.ctypes.data_as(u8p),
                            X.shape[0], X.shape[1], S, 0, 1, r.ctypes.data_as(f64p), None, None)
    assert rc == L.FS_OK
    assert np.array_equal(r, L.mi_matrices("gpu", X, y, S)[0])
    assert np.abs(r - rel).max() <= TOL


@pytest.mark.parametrize("name,tiles", [("states32", 7), ("p130", 10), ("p34_tile16", 1),
                                        ("geo_s16_p17_n257", 4), ("geo_s20_p11_n97", 3),
                                        ("geo_s24_p8_n257", 4), ("geo_s28_p6_n97", 3)])
def test_several_launches(L, name, tiles):
    """The tile range split over launches (the mi_tiles hook: 66 tiles by 7,
    45 by 10, 6 one by one; at NB = 4, 5, 6, 7 15 tiles by 4, 10 by 3, 15 by 4,
    10 by 3) gives the bits and tables of one launch."""
    X, y, S, _, _, cnt = mi_np.case(name, mi_np.ALL_SHAPES[name])
    r1, R1 = L.mi_matrices("gpu", X, y, S)
    with L.test_hooks(mi_tiles=tiles):
        r2, R2, c2 = L.mi_matrices("gpu", X, y, S, want_counts=True)
    assert np.array_equal(r2, r1) and np.array_equal(R2, R1) and np.array_equal(c2, cnt)


def test_identical_columns_and_units(L):
    X, y = mi_np.uniform(203, 6, 3, 41)
    X = X.copy()
    X[:, 2] = X[:, 1]   # neighbours: every third column meets both on the same side
    X[:, 4] = 2         # a constant column
    rel, red = L.mi_matrices("gpu", X, y, 3)
    keep = [0, 3, 4, 5]
    assert np.array_equal(red[1, keep], red[2, keep]) and rel[1] == rel[2]
    assert rel[4] == 0.0 and not red[4].any() and not red[:, 4].any()
    _, cnt = np.unique(X[:, 1], return_counts=True)
    q = cnt / 203.0
    # the eps of the stated expressions lowers I(x; x) by 1.3e-11 at three states
    assert abs(red[1, 2] - float(-(q * np.log2(q)).sum())) <= TOL
    rel_n, red_n = L.mi_matrices("gpu", X, y, 3, unit="nat")
    assert np.abs(rel_n - rel * np.log(2.0)).max() <= TOL
    assert np.abs(red_n - red * np.log(2.0)).max() <= TOL


def test_code_equal_to_n_states_is_rejected(L):
    X, y = mi_np.uniform(64, 5, 3, 42)
    X = X.copy()
    X[63, 4] = 3
    with pytest.raises(ValueError, match=">= n_states"):
        L.mi_matrices("gpu", X, y, 3)
    X[63, 4] = 0
    y = y.copy()
    y[10] = 3
    with pytest.raises(ValueError, match=">= n_states"):
        L.mi_matrices("gpu", X, y, 3)


def test_33_states(L):
    from fastselect_amd import mutual_information as mi
    X, y = mi_np.uniform(90, 3, 33, 33)
    X = X.copy()
    X[0, 0] = 32
    with pytest.raises(ValueError, match="32 states"):
        L.mi_matrices("gpu", X, y, 33)
    with pytest.raises(RuntimeError, match="GPU backend supports ≤32 states"):
        mi.calculate_mi_matrices(X, y, backend="gpu")
    rel, _ = mi.calculate_mi_matrices(X, y, backend="auto")   # answers from the CPU
    assert np.array_equal(rel, mi.calculate_mi_matrices(X, y, backend="cpu")[0])


def test_matrix_that_cannot_be_allocated_is_out_of_memory(L):
    """p^2 * 8 bytes beyond the device: the out-of-memory code, no fault."""
    lib = L.lib()
    u8p, f64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_double)
    p = 1 << 26
    x = np.zeros(16, np.uint8)
    r = np.zeros(1)
    # rejected on its size alone, before any array is read
    rc = lib.fs_mi_matrices(L.BACKEND_GPU, 0, x.ctypes.data_as(u8p), x.ctypes.data_as(u8p), 1, p,
                            3, 0, 1, r.ctypes.data_as(f64p), r.ctypes.data_as(f64p), None)
    assert rc == L.FS_EOOM


def test_single_pair_and_auto(L):
    from fastselect_amd import mutual_information as mi
    X, y = mi_np.uniform(150, 4, 6, 43)
    rel, red = mi.calculate_mi_matrices(X, y)   # 'auto' with a device
    grel, gred = mi.calculate_mi_matrices(X, y, backend="gpu")
    assert np.array_equal(rel, grel) and np.array_equal(red, gred)
    assert mi.calculate_mi_single_pair(X[:, 1], X[:, 3], backend="gpu") == gred[1, 3]
    assert abs(mi.calculate_mi_single_pair(X[:, 1], y, backend="gpu") - grel[1]) <= TOL


@pytest.mark.parametrize("method", ["MID", "MIQ"])
@pytest.mark.parametrize("n,p,states,seed", mi_np.PLANTED)
def test_estimator_gpu_equals_cpu(L, n, p, states, seed, method):
    from fastselect_amd import mRMR
    X, y = mi_np.planted(n, p, states, seed)
    # the restatement's own scores keep every greedy step far from a tie
    S = int(max(X.max(), y.max())) + 1
    _, _, _, rel, red, _ = mi_np.case(("planted", n, p, states, seed), lambda: (X, y, S))
    want, margins = mi_np.greedy(rel, red, 5, method)
    assert margins.min() >= mi_np.PLANT_MARGIN
    g = mRMR(5, method=method, backend="gpu").fit(X, y)
    c = mRMR(5, method=method, backend="cpu").fit(X, y)
    assert g.effective_backend_ == "gpu" and c.effective_backend_ == "cpu"
    assert np.array_equal(g.top_features_, c.top_features_)
    assert np.array_equal(g.top_features_, want)
    assert np.abs(g.relevance_scores_ - c.relevance_scores_).max() <= TOL
    assert np.abs(g.redundancy_matrix_ - c.redundancy_matrix_).max() <= TOL
    assert np.abs(g.redundancy_matrix_ - red).max() <= TOL


def test_readme_pipeline_on_auto(L):
    from sklearn.pipeline import Pipeline
    from fastselect_amd import MDR, mRMR
    import mdr_np
    X, y = mdr_np.planted(160, 60, pair=(7, 41))
    pipe = Pipeline([("mrmr", mRMR(n_features_to_select=40, backend="auto")),
                     ("mdr", MDR(k=2, cv=3))])
    pred = pipe.fit(X, y).predict(X)
    assert pipe.named_steps["mrmr"].effective_backend_ == "gpu"
    assert pipe.named_steps["mdr"].effective_backend_ == "gpu"
    assert pred.shape == (160,)
