"""The MDR entry points of the C ABI report bad arguments the documented way
(CPU only; no GPU compute here)."""
import ctypes

import numpy as np
import pytest

from fastselect_amd import _lib

CPU, GPU = _lib.BACKEND_CPU, _lib.BACKEND_GPU


def _scan(backend=CPU, n=12, p=4, k=2, x=None, is_case=None, fold=None, n_folds=0, best=True,
          rank=True, n_arg=None):
    """fs_mdr_scan through raw ctypes; returns (rc, message)."""
    lib = _lib.lib()
    rng = np.random.default_rng(3)
    xa = rng.integers(0, 3, size=(n, p)).astype(np.uint8) if x is None else x
    ca = (np.arange(n) % 2).astype(np.uint8) if is_case is None else is_case
    ba = np.zeros(max(n_folds, 1), np.float32)
    rk = np.zeros(max(n_folds, 1), np.int64)
    u8p, i32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int32)
    rc = lib.fs_mdr_scan(
        backend, 0, None if x is False else xa.ctypes.data_as(u8p), n if n_arg is None else n_arg,
        p, None if is_case is False else ca.ctypes.data_as(u8p), k,
        None if fold is None else fold.ctypes.data_as(i32p), n_folds, 1,
        ba.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if best else None,
        rk.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if rank else None, None)
    return rc, lib.fs_last_error().decode()


def test_valid_call_is_ok():
    rc, _ = _scan()
    assert rc == _lib.FS_OK
    rc, _ = _scan(fold=(np.arange(12) % 3).astype(np.int32), n_folds=3)
    assert rc == _lib.FS_OK


@pytest.mark.parametrize("k", [0, -1, 7])
def test_k_outside_1_to_6(k):
    rc, msg = _scan(p=8, k=k)
    assert rc == _lib.FS_EINVAL and "k must be in 1..6" in msg


def test_k_above_p():
    rc, msg = _scan(p=3, k=4)
    assert rc == _lib.FS_EINVAL and "columns" in msg


@pytest.mark.parametrize("n_arg", [0, -5, 1 << 25])
def test_n_out_of_range(n_arg):
    rc, msg = _scan(n_arg=n_arg)  # rejected before any array is read
    assert rc == _lib.FS_EINVAL and "2^25" in msg


def test_genotype_above_two():
    x = np.zeros((12, 4), np.uint8)
    x[11, 3] = 3
    rc, msg = _scan(x=x)
    assert rc == _lib.FS_EINVAL and "0/1/2" in msg
    x[11, 3] = 255
    rc, msg = _scan(x=x, fold=(np.arange(12) % 2).astype(np.int32), n_folds=2)
    assert rc == _lib.FS_EINVAL and "0/1/2" in msg


@pytest.mark.parametrize("bad", [-1, 3])
def test_fold_id_out_of_range(bad):
    fold = (np.arange(12) % 3).astype(np.int32)
    fold[5] = bad
    rc, msg = _scan(fold=fold, n_folds=3)
    assert rc == _lib.FS_EINVAL and "fold id" in msg


def test_fold_and_n_folds_go_together():
    rc, _ = _scan(fold=np.zeros(12, np.int32), n_folds=0)
    assert rc == _lib.FS_EINVAL
    rc, _ = _scan(fold=None, n_folds=2)
    assert rc == _lib.FS_EINVAL


def test_overflowing_combination_count():
    lib = _lib.lib()
    c = ctypes.c_int64(0)
    assert lib.fs_mdr_combinations(1 << 20, 6, ctypes.byref(c)) == _lib.FS_EINVAL
    assert "2^62" in lib.fs_last_error().decode()
    assert lib.fs_mdr_combinations(3000, 6, ctypes.byref(c)) == _lib.FS_OK
    assert c.value == 3000 * 2999 * 2998 * 2997 * 2996 * 2995 // 720
    # the scan rejects it before it reads x (n x p would not exist)
    rc, msg = _scan(n=12, p=1 << 20, k=6, x=np.zeros((1, 1), np.uint8))
    assert rc == _lib.FS_EINVAL and "2^62" in msg
    f = (ctypes.c_int32 * 6)()
    assert lib.fs_mdr_unrank(1 << 20, 6, 0, f) == _lib.FS_EINVAL
    assert lib.fs_mdr_unrank(9, 4, -1, f) == _lib.FS_EINVAL
    assert lib.fs_mdr_unrank(9, 4, 126, f) == _lib.FS_EINVAL
    assert lib.fs_mdr_unrank(9, 4, 125, f) == _lib.FS_OK and list(f)[:4] == [5, 6, 7, 8]


def test_null_pointers():
    for kw in ({"x": False}, {"is_case": False}, {"best": False}, {"rank": False}):
        rc, msg = _scan(**kw)
        assert rc == _lib.FS_EINVAL and "NULL" in msg, kw
    lib = _lib.lib()
    assert lib.fs_mdr_combinations(5, 2, None) == _lib.FS_EINVAL
    assert lib.fs_mdr_unrank(5, 2, 0, None) == _lib.FS_EINVAL


def test_bad_backend_code():
    rc, msg = _scan(backend=7)
    assert rc == _lib.FS_EINVAL and "backend" in msg


def test_gpu_backend_without_a_device_is_enodev():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    rc, msg = _scan(backend=GPU)
    assert rc == _lib.FS_ENODEV and "no HIP device" in msg
    with pytest.raises(RuntimeError, match="no HIP device"):
        _lib.mdr_scan("gpu", np.zeros((4, 2), np.uint8), [0, 1, 0, 1], 2)
