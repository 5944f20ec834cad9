"""fs_mdr_scan_labels on the CPU backend: row b of every output must equal
what fs_mdr_scan returns for labels[b], bit for bit (no tolerance: all
quantities are integer counts until the three float64 operations of the BA),
and bad arguments are reported the documented way.  No GPU compute here."""
import ctypes

import numpy as np
import pytest

import mdr_np
from fastselect_amd import _lib

CPU = _lib.BACKEND_CPU


def labellings(y, n_labelings, seed=1):
    """Row 0 is y == 1; the others are permutations of it."""
    rng = np.random.default_rng(seed)
    rows = [(y == 1).astype(np.uint8)]
    for _ in range(1, n_labelings):
        rows.append(rng.permutation(rows[0]))
    return np.stack(rows)


def folds(X, y, cv):
    return (mdr_np.fold_ids(X, y, cv)[0], cv) if cv else (None, 0)


def assert_rows_equal_single_scans(backend, X, labels, k, fold, cv, got=None):
    bb, br, ba = got or _lib.mdr_scan_labels(backend, X, labels, k, fold, cv, want_ba=True)
    F = max(cv, 1)
    assert bb.shape == (len(labels), F) and br.shape == (len(labels), F)
    for b, lab in enumerate(labels):
        sb, sr, sa = _lib.mdr_scan("cpu", X, lab, k, fold, cv, want_ba=True)
        assert np.array_equal(ba[b].view(np.uint32), sa.view(np.uint32)), b
        assert np.array_equal(bb[b].view(np.uint32), sb.view(np.uint32)), b
        assert np.array_equal(br[b], sr), b
    return bb, br, ba


@pytest.mark.parametrize("cv", [0, 2, 10, 17])
@pytest.mark.parametrize("p,k", [(7, 1), (7, 2), (7, 3), (24, 1), (24, 2), (24, 3), (8, 6)])
@pytest.mark.parametrize("n", [203, 1100])
def test_rows_equal_fs_mdr_scan(n, p, k, cv):
    """n = 203 with cv = 10: every fold is shorter than one word; n = 1100:
    folds span several words and have unequal sizes."""
    X, y = mdr_np.planted(n, p)
    fold, cv = folds(X, y, cv)
    for B in (1, 5):
        labels = labellings(y, B)
        bb, br, _ = assert_rows_equal_single_scans("cpu", X, labels, k, fold, cv)
        # without ba_out the same bests come back
        bb2, br2 = _lib.mdr_scan_labels("cpu", X, labels, k, fold, cv)
        assert np.array_equal(bb2, bb) and np.array_equal(br2, br)


def test_labellings_need_not_be_permutations():
    X, y = mdr_np.planted(203, 9)
    rng = np.random.default_rng(4)
    labels = (rng.random((4, 203)) < np.array([[0.1], [0.5], [0.9], [0.3]])).astype(np.uint8)
    labels[3] *= 7  # any nonzero byte is a case
    fold, cv = folds(X, y, 5)
    assert_rows_equal_single_scans("cpu", X, labels, 2, fold, cv)


def test_special_labellings():
    X, y = mdr_np.planted(203, 9)
    fold, cv = folds(X, y, 3)
    labels = labellings(y, 4)
    labels[1] = 0                      # all controls
    labels[2] = 1                      # all cases
    labels[3] = (fold == 1)            # fold 1's training set has no cases
    bb, br, ba = assert_rows_equal_single_scans("cpu", X, labels, 2, fold, cv)
    assert not ba[1].any() and not bb[1].any() and not br[1].any()
    assert not ba[2].any() and not br[2].any()
    assert not ba[3, 1].any() and br[3, 1] == 0 and ba[3, 0].any()


def test_duplicated_column_ties_go_to_the_smaller_rank():
    X, y = mdr_np.planted(203, 12, pair=(2, 5))
    X = np.concatenate([X, X[:, 5:6]], axis=1)
    fold, cv = folds(X, y, 3)
    labels = labellings(y, 3)
    _, br, ba = assert_rows_equal_single_scans("cpu", X, labels, 2, fold, cv)
    assert [_lib.mdr_unrank(13, 2, int(r)) for r in br[0]] == [(2, 5)] * 3
    assert np.array_equal(br, np.argmax(ba, axis=2))


@pytest.mark.parametrize("cv", [0, 10])
def test_result_does_not_depend_on_the_thread_count(cv):
    X, y = mdr_np.planted(203, 24)
    fold, cv = folds(X, y, cv)
    labels = labellings(y, 5)
    one = _lib.mdr_scan_labels("cpu", X, labels, 2, fold, cv, n_jobs=1, want_ba=True)
    four = _lib.mdr_scan_labels("cpu", X, labels, 2, fold, cv, n_jobs=4, want_ba=True)
    for a, b in zip(one, four):
        assert a.tobytes() == b.tobytes()


def _raw(n=12, p=4, k=2, x=None, labels=None, n_labelings=2, fold=None, n_folds=0, best=True,
         rank=True):
    """fs_mdr_scan_labels through raw ctypes; returns (rc, message)."""
    lib = _lib.lib()
    rng = np.random.default_rng(3)
    xa = rng.integers(0, 3, size=(n, p)).astype(np.uint8) if x is None else x
    la = (np.arange(2 * n).reshape(2, n) % 2).astype(np.uint8) if labels is None else labels
    F = max(n_folds, 1)
    ba = np.zeros((2, F), np.float32)
    rk = np.zeros((2, F), np.int64)
    u8p, i32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int32)
    rc = lib.fs_mdr_scan_labels(
        CPU, 0, None if x is False else xa.ctypes.data_as(u8p), n, p,
        None if labels is False else la.ctypes.data_as(u8p), n_labelings, k,
        None if fold is None else fold.ctypes.data_as(i32p), n_folds, 1,
        ba.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if best else None,
        rk.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if rank else None, None)
    return rc, lib.fs_last_error().decode()


def test_valid_raw_call_is_ok():
    assert _raw()[0] == _lib.FS_OK
    assert _raw(fold=(np.arange(12) % 3).astype(np.int32), n_folds=3)[0] == _lib.FS_OK


@pytest.mark.parametrize("n_labelings", [0, -1, 65536])
def test_n_labelings_outside_1_to_65535(n_labelings):
    rc, msg = _raw(n_labelings=n_labelings)  # rejected before labels is read
    assert rc == _lib.FS_EINVAL and "n_labelings" in msg


def test_genotype_above_two():
    x = np.zeros((12, 4), np.uint8)
    x[11, 3] = 3
    rc, msg = _raw(x=x)
    assert rc == _lib.FS_EINVAL and "0/1/2" in msg


@pytest.mark.parametrize("bad", [-1, 3])
def test_fold_id_out_of_range(bad):
    fold = (np.arange(12) % 3).astype(np.int32)
    fold[5] = bad
    rc, msg = _raw(fold=fold, n_folds=3)
    assert rc == _lib.FS_EINVAL and "fold id" in msg


def test_null_pointers():
    for kw in ({"x": False}, {"labels": False}, {"best": False}, {"rank": False}):
        rc, msg = _raw(**kw)
        assert rc == _lib.FS_EINVAL and "NULL" in msg, kw
    assert _lib.lib().fs_mdr_labels_last_timing(None) == _lib.FS_EINVAL


def test_other_argument_rules_of_fs_mdr_scan():
    assert _raw(p=8, k=7)[0] == _lib.FS_EINVAL
    assert _raw(p=3, k=4)[0] == _lib.FS_EINVAL
    assert _raw(fold=None, n_folds=2)[0] == _lib.FS_EINVAL
