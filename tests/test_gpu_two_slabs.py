"""A sample axis of two pack slabs on the GPU: n = 65535 * 32 + 33 = 2097153.

The pack kernels (k_mi_pack; k_mdr_pack from fs_mdr_scan and fs_mdr_scan_top;
k_mdr_pack_cols and k_mdr_pack_labels) put the word index in grid.y, which
holds 65535, and loop over slabs of 65535 words.  Here word 65536 is the first
of a second slab (the pointer and offset arithmetic per slab, w0 > 0) and the
last word is ragged.  The row kernels restage LDS 1025 times (64 words a
chunk).  Three 3-state columns, y the parity of columns 0 and 2 with 20 %
flipped, fold ids i % 3 (mi_np.two_slabs): small enough that numpy's bincount
tables and mdr_np.scan stay the reference.

Every family keeps its own rule: tables exact and values within 1e-10 (MI,
mRMR, JMI; the bound is derived in test_mi.py and test_jmi.py for n < 2^31),
one float32 step and at most 1 % differing (CFS), bit for bit (MDR)."""
import numpy as np
import pytest

import cfs_np
import mdr_np
import mi_np
from mdr_top_np import same, same_bits

pytestmark = pytest.mark.gpu

TOL = 1e-10
SLAB = 65535   # grid.y of a pack launch


@pytest.fixture(scope="module")
def L():
    from fastselect_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    return _lib


@pytest.fixture(scope="module")
def data():
    X, y, fold = mi_np.two_slabs_case()
    n = X.shape[0]
    # a second slab with one whole word and a ragged one, whatever padding a
    # segment layout adds
    assert n == SLAB * 32 + 33 and -(-n // 32) == SLAB + 2 and n % 32 == 1
    return X, y, fold


def bincount_tables(X, y, S):
    """(cxx [p, p, S, S] for i < j, cxy [p, S, S]) by np.bincount."""
    n, p = X.shape
    X = X.astype(np.int64)
    cxx = np.zeros((p, p, S, S), dtype=np.int64)
    cxy = np.zeros((p, S, S), dtype=np.int64)
    for i in range(p):
        cxy[i] = np.bincount(X[:, i] * S + y, minlength=S * S).reshape(S, S)
        for j in range(i + 1, p):
            cxx[i, j] = np.bincount(X[:, i] * S + X[:, j], minlength=S * S).reshape(S, S)
    return cxx, cxy


def test_mi_matrices(L, data):
    X, y, _ = data
    n, p = X.shape
    cxx, cxy = bincount_tables(X, y, 3)
    assert cxy.sum() == p * n and cxx[0, 1].sum() == n
    rel = mi_np.mi_of_tables(cxy, n)
    m = mi_np.mi_of_tables(cxx, n) * np.triu(np.ones((p, p)), 1)
    red = m + m.T
    gr, gR, gc = L.mi_matrices("gpu", X, y, 3, want_counts=True)
    cr, cR, cc = L.mi_matrices("cpu", X, y, 3, want_counts=True)
    print("gpu-numpy", max(np.abs(gr - rel).max(), np.abs(gR - red).max()),
          "gpu-cpu", max(np.abs(gr - cr).max(), np.abs(gR - cR).max()))
    assert np.array_equal(gc, cxx) and np.array_equal(gc, cc)
    assert np.abs(gr - rel).max() <= TOL and np.abs(gR - red).max() <= TOL
    assert np.abs(gr - cr).max() <= TOL and np.abs(gR - cR).max() <= TOL
    assert np.array_equal(gR, gR.T) and not np.diag(gR).any()
    assert gr[0] > 0.01 > gr[1]   # the parity columns carry the signal jointly only


def test_jmi_rows(L, data):
    X, y, _ = data
    got = L.jmi_rows("gpu", X, y, 3, [0, 1, 2])
    cpu = L.jmi_rows("cpu", X, y, 3, [0, 1, 2])
    print("gpu-cpu", np.abs(got - cpu).max())
    assert np.abs(got - cpu).max() <= TOL
    assert np.array_equal(got, got.T) and not np.diag(got).any()
    assert got[0, 2] > 0.2 > got[0, 1]   # the planted pair


def test_cfs_row(L, data):
    X, y, _ = data
    with L.Cfs("cpu", X, y, 3) as c:
        want = np.concatenate([c.relevance(), c.row(1)])
    with L.Cfs("gpu", X, y, 3) as g:
        got = np.concatenate([g.relevance(), g.row(1)])
    steps = cfs_np.f32_steps(got, want)
    print("float32 steps", steps.max(), "differing share", np.count_nonzero(steps) / steps.size)
    assert steps.max(initial=0) <= 1
    assert np.count_nonzero(steps) <= 0.01 * steps.size
    assert got[4] == 0.0 and got[:3].all()


def test_mrmr_select(L, data):
    X, y, _ = data
    rel, red = L.mi_matrices("gpu", X, y, 3)
    sel, r, rows = L.mrmr_select("gpu", X, y, 3, 3)
    want, _ = mi_np.greedy(rel, red, 3, "MID")
    assert np.array_equal(r, rel) and np.array_equal(sel, want)
    assert np.array_equal(rows, red[want])
    cr, cR = L.mi_matrices("cpu", X, y, 3)
    assert np.abs(r - cr).max() <= TOL and np.abs(rows - cR[sel]).max() <= TOL


@pytest.mark.parametrize("folds", [0, 3])
def test_mdr_scan(L, data, folds):
    X, y, fold = data
    fold = fold if folds else None
    want = mdr_np.scan(X, y == 1, 2, fold, folds)
    gb, gr, gba = L.mdr_scan("gpu", X, y == 1, 2, fold, folds, want_ba=True)
    cb, cr, cba = L.mdr_scan("cpu", X, y == 1, 2, fold, folds, want_ba=True)
    assert same_bits(gba, want) and same_bits(gba, cba)
    assert same_bits(gb, cb) and np.array_equal(gr, cr)
    assert gr.tolist() == [1] * max(folds, 1)   # (0, 2), the parity pair


def test_mdr_scan_top(L, data):
    X, y, fold = data
    g = L.mdr_scan_top("gpu", X, y == 1, 2, fold, 3, n_top=2)
    c = L.mdr_scan_top("cpu", X, y == 1, 2, fold, 3, n_top=2)
    assert same(g, c)
    best = L.mdr_scan("gpu", X, y == 1, 2, fold, 3)
    assert same_bits(g[0][:, 0], best[0]) and np.array_equal(g[1][:, 0], best[1])


def test_mdr_scan_labels(L, data):
    X, y, fold = data
    labels = np.stack([y, np.random.default_rng(3).permutation(y)])
    gb, gr, gba = L.mdr_scan_labels("gpu", X, labels, 2, fold, 3, want_ba=True)
    cb, cr, cba = L.mdr_scan_labels("cpu", X, labels, 2, fold, 3, want_ba=True)
    assert same_bits(gba, cba) and same_bits(gb, cb) and np.array_equal(gr, cr)
    sb, sr, sba = L.mdr_scan("gpu", X, y == 1, 2, fold, 3, want_ba=True)
    assert same_bits(gba[0], sba) and same_bits(gb[0], sb) and np.array_equal(gr[0], sr)
