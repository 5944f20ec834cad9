"""fs_mi_matrices reports bad arguments the documented way (CPU only; no GPU
compute here).  The checks are shared by both backends and come before the
device check, so the GPU backend's own limit is tested without a device."""
import ctypes

import numpy as np
import pytest

from fastselect_amd import _lib

CPU, GPU = _lib.BACKEND_CPU, _lib.BACKEND_GPU
_u8p = ctypes.POINTER(ctypes.c_uint8)
_f64p = ctypes.POINTER(ctypes.c_double)
_i32p = ctypes.POINTER(ctypes.c_int32)


def _call(backend=CPU, n=12, p=4, states=3, unit=0, x=None, y=None, rel=True, red=True,
          n_arg=None, p_arg=None):
    """fs_mi_matrices through raw ctypes; returns (rc, message, rel, red)."""
    lib = _lib.lib()
    rng = np.random.default_rng(3)
    xa = rng.integers(0, min(states, 3), size=(n, p)).astype(np.uint8) if x is None else x
    ya = (np.arange(n) % 2).astype(np.uint8) if y is None else y
    r = np.zeros(p)
    R = np.full((p, p), -1.0)
    rc = lib.fs_mi_matrices(
        backend, 0, None if x is False else xa.ctypes.data_as(_u8p),
        None if y is False else ya.ctypes.data_as(_u8p), n if n_arg is None else n_arg,
        p if p_arg is None else p_arg, states, unit, 1, r.ctypes.data_as(_f64p) if rel else None,
        R.ctypes.data_as(_f64p) if red else None, None)
    return rc, lib.fs_last_error().decode(), r, R


def test_valid_call_is_ok():
    rc, _, r, R = _call()
    assert rc == _lib.FS_OK
    assert np.array_equal(R, R.T) and not np.diag(R).any() and (r >= -1e-15).all()


def test_null_redundancy_is_accepted():
    rc, _, r, _ = _call(red=False)
    assert rc == _lib.FS_OK
    assert np.array_equal(r, _call()[2])


@pytest.mark.parametrize("n_arg", [0, -3, 1 << 31])
def test_n_out_of_range(n_arg):
    rc, msg, _, _ = _call(n_arg=n_arg)   # rejected before any array is read
    assert rc == _lib.FS_EINVAL and "2^31" in msg


@pytest.mark.parametrize("p_arg", [0, -1])
def test_p_out_of_range(p_arg):
    rc, msg, _, _ = _call(p_arg=p_arg)
    assert rc == _lib.FS_EINVAL and "p must be >= 1" in msg


@pytest.mark.parametrize("states", [0, -1, 257])
def test_n_states_out_of_range(states):
    rc, msg, _, _ = _call(states=states, x=np.zeros((12, 4), np.uint8))
    assert rc == _lib.FS_EINVAL and "1..256" in msg


def test_256_states_are_accepted():
    x = np.zeros((12, 4), np.uint8)
    x[3, 1] = 255
    rc, _, _, _ = _call(states=256, x=x)
    assert rc == _lib.FS_OK


def test_code_equal_to_n_states():
    x = np.zeros((12, 4), np.uint8)
    x[11, 3] = 3
    rc, msg, _, _ = _call(x=x)
    assert rc == _lib.FS_EINVAL and ">= n_states" in msg
    y = np.zeros(12, np.uint8)
    y[5] = 3
    rc, msg, _, _ = _call(y=y)
    assert rc == _lib.FS_EINVAL and ">= n_states" in msg
    with pytest.raises(ValueError, match=">= n_states"):
        _lib.mi_matrices("cpu", x, np.zeros(12, np.uint8), 3)


def test_gpu_backend_rejects_more_than_32_states():
    rc, msg, _, _ = _call(backend=GPU, states=33)   # with or without a device
    assert rc == _lib.FS_EINVAL and "32 states" in msg


def test_bad_unit():
    rc, msg, _, _ = _call(unit=2)
    assert rc == _lib.FS_EINVAL and "unit" in msg


def test_null_pointers():
    for kw in ({"x": False}, {"y": False}, {"rel": False}):
        rc, msg, _, _ = _call(**kw)
        assert rc == _lib.FS_EINVAL and "NULL" in msg, kw
    assert _lib.lib().fs_mi_last_timing(None) == _lib.FS_EINVAL


def test_bad_backend_code():
    rc, msg, _, _ = _call(backend=7)
    assert rc == _lib.FS_EINVAL and "backend" in msg


def test_gpu_backend_without_a_device_is_enodev():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    rc, msg, _, _ = _call(backend=GPU)
    assert rc == _lib.FS_ENODEV and "no HIP device" in msg
