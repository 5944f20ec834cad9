"""fs_mdr_scan_top on the CPU backend: the n_top best combinations of every
fold, ordered by (float32 BA descending, rank ascending), against the numpy
restatement -- ``np.argsort(-ba, kind="stable")[:n_top]`` per fold, with no
tolerance: every quantity is an integer until three float64 operations."""
import ctypes

import numpy as np
import pytest

import mdr_np
from fastselect_amd import _lib
from mdr_top_np import expected, same_bits

TOPS = (1, 7, 300)


@pytest.mark.parametrize("n_top", TOPS)
@pytest.mark.parametrize("n,p,k,cv", mdr_np.SHAPES)
def test_top_equals_numpy(n, p, k, cv, n_top):
    X, y, fold, ba = mdr_np.case(n, p, k, cv)
    want_ba, want_rank = expected(ba, n_top)
    got_ba, got_rank = _lib.mdr_scan_top("cpu", X, y == 1, k, fold, cv, n_top=n_top)
    assert same_bits(got_ba, want_ba)
    assert np.array_equal(got_rank, want_rank)


def test_top_without_folds():
    X, y, _, _ = mdr_np.case(203, 40, 2, 5)
    want_ba, want_rank = expected(mdr_np.scan(X, y == 1, 2), 7)
    got_ba, got_rank = _lib.mdr_scan_top("cpu", X, y == 1, 2, n_top=7)
    assert same_bits(got_ba, want_ba) and np.array_equal(got_rank, want_rank)


@pytest.mark.parametrize("n,p,k,cv", mdr_np.SHAPES)
def test_entry_0_is_mdr_scan(n, p, k, cv):
    X, y, fold, _ = mdr_np.case(n, p, k, cv)
    best_ba, best_rank = _lib.mdr_scan("cpu", X, y == 1, k, fold, cv)
    top_ba, top_rank = _lib.mdr_scan_top("cpu", X, y == 1, k, fold, cv, n_top=7)
    assert same_bits(top_ba[:, 0], best_ba) and np.array_equal(top_rank[:, 0], best_rank)


def test_n_top_above_the_count_pads():
    n, p, k, cv = 33, 5, 1, 2
    X, y, fold, ba = mdr_np.case(n, p, k, cv)
    got_ba, got_rank = _lib.mdr_scan_top("cpu", X, y == 1, k, fold, cv, n_top=7)
    want_ba, want_rank = expected(ba, 7)
    assert same_bits(got_ba, want_ba) and np.array_equal(got_rank, want_rank)
    assert np.all(got_rank[:, 5:] == -1) and not got_ba[:, 5:].any()
    assert np.all(got_rank[:, :5] >= 0)


def test_ties_keep_the_earlier_rank():
    X, y = mdr_np.noise_16x30()
    ba = mdr_np.scan(X, y == 1, 3)
    want_ba, want_rank = expected(ba, 100)
    assert len(np.unique(want_ba[0])) < 100  # masses of equal BAs
    got_ba, got_rank = _lib.mdr_scan_top("cpu", X, y == 1, 3, n_top=100)
    assert same_bits(got_ba, want_ba) and np.array_equal(got_rank, want_rank)


def test_thread_count_does_not_show():
    X, y, fold, _ = mdr_np.case(203, 14, 3, 3)
    one = _lib.mdr_scan_top("cpu", X, y == 1, 3, fold, 3, n_top=300, n_jobs=1)
    many = _lib.mdr_scan_top("cpu", X, y == 1, 3, fold, 3, n_top=300, n_jobs=-1)
    assert same_bits(one[0], many[0]) and np.array_equal(one[1], many[1])
    X, y = mdr_np.noise_16x30()
    one = _lib.mdr_scan_top("cpu", X, y == 1, 3, n_top=100, n_jobs=1)
    many = _lib.mdr_scan_top("cpu", X, y == 1, 3, n_top=100, n_jobs=-1)
    assert same_bits(one[0], many[0]) and np.array_equal(one[1], many[1])


def _raw(x, case, k, fold, n_folds, n_top, top_ba, top_rank):
    p8 = ctypes.POINTER(ctypes.c_uint8)
    return _lib.lib().fs_mdr_scan_top(
        0, 0, x.ctypes.data_as(p8) if x is not None else None, x.shape[0] if x is not None else 4,
        x.shape[1] if x is not None else 4, case.ctypes.data_as(p8) if case is not None else None,
        k, fold.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if fold is not None else None,
        n_folds, n_top, 1,
        top_ba.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if top_ba is not None else None,
        top_rank.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if top_rank is not None else None)


def test_einval():
    X, y, fold, _ = mdr_np.case(33, 5, 1, 2)
    X = np.ascontiguousarray(X)
    case = np.ascontiguousarray(y == 1, dtype=np.uint8)
    fold = np.ascontiguousarray(fold)
    ba = np.zeros((2, 8), dtype=np.float32)
    rank = np.zeros((2, 8), dtype=np.int64)
    ok = _raw(X, case, 1, fold, 2, 8, ba, rank)
    assert ok == 0
    bad = [
        _raw(X, case, 1, fold, 2, 0, ba, rank),       # n_top < 1
        _raw(X, case, 1, fold, 2, -3, ba, rank),
        _raw(X, case, 1, fold, 2, _lib.MDR_MAX_TOP + 1, ba, rank),
        _raw(X, case, 1, fold, 2, 8, None, rank),     # NULL outputs
        _raw(X, case, 1, fold, 2, 8, ba, None),
        _raw(None, case, 1, fold, 2, 8, ba, rank),    # fs_mdr_scan's own checks
        _raw(X, None, 1, fold, 2, 8, ba, rank),
        _raw(X, case, 0, fold, 2, 8, ba, rank),
        _raw(X, case, 7, fold, 2, 8, ba, rank),
        _raw(X, case, 6, fold, 2, 8, ba, rank),       # k > p
        _raw(X, case, 1, fold, 0, 8, ba, rank),       # fold without n_folds
        _raw(X, case, 1, None, 2, 8, ba, rank),
    ]
    assert bad == [_lib.FS_EINVAL] * len(bad)
    with pytest.raises(ValueError, match="n_top"):
        _lib.mdr_scan_top("cpu", X, case, 1, n_top=0)
    with pytest.raises(ValueError, match=str(_lib.MDR_MAX_TOP)):
        _lib.mdr_scan_top("cpu", X, case, 1, n_top=_lib.MDR_MAX_TOP + 1)
    bad_fold = fold.copy()
    bad_fold[3] = 2
    with pytest.raises(ValueError, match="fold id"):
        _lib.mdr_scan_top("cpu", X, case, 1, bad_fold, 2, n_top=3)
    X3 = X.copy()
    X3[0, 0] = 3
    with pytest.raises(ValueError, match="0/1/2"):
        _lib.mdr_scan_top("cpu", X3, case, 1, n_top=3)


def test_timing_without_a_gpu_call_is_unset_or_positive():
    t = _lib.mdr_top_last_timing()
    assert len(t) == 4 and all(v == -1.0 or v >= 0.0 for v in t)
