"""fs_jmi_* report bad arguments the documented way (CPU only; no GPU compute
here).  The checks are shared by both backends and come before the device
check, so the GPU backend's state limit is tested without a device."""
import ctypes

import numpy as np
import pytest

from fastselect_amd import _lib

CPU, GPU = _lib.BACKEND_CPU, _lib.BACKEND_GPU
_u8p = ctypes.POINTER(ctypes.c_uint8)
_f64p = ctypes.POINTER(ctypes.c_double)
_i64p = ctypes.POINTER(ctypes.c_int64)


def _data(n, p, states, x, y):
    rng = np.random.default_rng(5)
    xa = rng.integers(0, min(states, 3), size=(n, p)).astype(np.uint8) if x is None else x
    ya = (np.arange(n) % 2).astype(np.uint8) if y is None else y
    return xa, ya


def _select(backend=CPU, n=24, p=6, states=3, unit=0, method=0, k=3, x=None, y=None, rel=True,
            sel=True, rows=True):
    """fs_jmi_select through raw ctypes; returns (rc, message, selected, relevance, rows)."""
    lib = _lib.lib()
    xa, ya = _data(n, p, states, x, y)
    r = np.zeros(p)
    s = np.full(max(k, 1), -7, dtype=np.int64)
    R = np.full((max(k, 1), p), -1.0)
    rc = lib.fs_jmi_select(
        backend, 0, None if x is False else xa.ctypes.data_as(_u8p),
        None if y is False else ya.ctypes.data_as(_u8p), n, p, states, unit, method, k, 1,
        r.ctypes.data_as(_f64p) if rel else None, s.ctypes.data_as(_i64p) if sel else None,
        R.ctypes.data_as(_f64p) if rows else None)
    return rc, lib.fs_last_error().decode(), s, r, R


def _rows(backend=CPU, n=24, p=6, states=3, unit=0, anchors=(0, 5), x=None, y=None, out=True):
    """fs_jmi_rows through raw ctypes; returns (rc, message, rows)."""
    lib = _lib.lib()
    xa, ya = _data(n, p, states, x, y)
    m = 0 if anchors is None else len(anchors)
    anc = np.array(anchors if anchors else [0], dtype=np.int64)
    R = np.full((max(m, 1), p), -1.0)
    rc = lib.fs_jmi_rows(
        backend, 0, None if x is False else xa.ctypes.data_as(_u8p),
        None if y is False else ya.ctypes.data_as(_u8p), n, p, states, unit,
        None if anchors is None else anc.ctypes.data_as(_i64p), m, 1,
        R.ctypes.data_as(_f64p) if out else None)
    return rc, lib.fs_last_error().decode(), R


def test_symbols_are_exported():
    lib = _lib.lib()
    for name in ("fs_jmi_select", "fs_jmi_rows", "fs_jmi_search_matrix", "fs_jmi_last_timing"):
        assert name in _lib.EXPORTED
        assert getattr(lib, name) is not None


def test_valid_calls_are_ok():
    rc, _, s, r, R = _select()
    assert rc == _lib.FS_OK
    assert len(set(s.tolist())) == 3 and s.min() >= 0 and s.max() < 6
    assert s[0] == int(np.argmax(r))
    assert all(R[t, s[t]] == 0.0 for t in range(3))
    rc, _, A = _rows(anchors=tuple(s.tolist()))
    assert rc == _lib.FS_OK and np.array_equal(A, R)


def test_null_rows_give_the_same_selection():
    for method in (0, 1):
        _, _, s1, r1, _ = _select(method=method, k=6)
        rc, _, s2, r2, _ = _select(method=method, k=6, rows=False)
        assert rc == _lib.FS_OK
        assert np.array_equal(s1, s2) and np.array_equal(r1, r2)


@pytest.mark.parametrize("k", [0, 7, -1])
def test_k_out_of_range(k):
    rc, msg, _, _, _ = _select(k=k)
    assert rc == _lib.FS_EINVAL and "k must be in 1..p" in msg


@pytest.mark.parametrize("method", [2, -1])
def test_bad_method(method):
    rc, msg, _, _, _ = _select(method=method)
    assert rc == _lib.FS_EINVAL and "method" in msg


def test_null_pointers():
    for kw in ({"x": False}, {"y": False}, {"rel": False}, {"sel": False}):
        rc, msg, _, _, _ = _select(**kw)
        assert rc == _lib.FS_EINVAL and "NULL" in msg, kw
    for kw in ({"x": False}, {"y": False}, {"anchors": None}, {"out": False}):
        rc, msg, _ = _rows(**kw)
        assert rc == _lib.FS_EINVAL and "NULL" in msg, kw
    assert _lib.lib().fs_jmi_last_timing(None) == _lib.FS_EINVAL


@pytest.mark.parametrize("anchors", [(6,), (0, -1), (2, 3, 100)])
def test_anchor_out_of_range(anchors):
    rc, msg, _ = _rows(anchors=anchors)
    assert rc == _lib.FS_EINVAL and "anchor" in msg
    with pytest.raises(ValueError, match="anchor"):
        _lib.jmi_rows("cpu", np.zeros((24, 6), np.uint8), np.zeros(24, np.uint8), 3, anchors)


def test_no_anchor():
    rc, msg, _ = _rows(anchors=())
    assert rc == _lib.FS_EINVAL and "m must be" in msg


def test_code_equal_to_n_states():
    x = np.zeros((24, 6), np.uint8)
    x[23, 5] = 3
    y = np.zeros(24, np.uint8)
    y[5] = 3
    for rc, msg in (_select(x=x)[:2], _select(y=y)[:2], _rows(x=x)[:2], _rows(y=y)[:2]):
        assert rc == _lib.FS_EINVAL and ">= n_states" in msg
    with pytest.raises(ValueError, match=">= n_states"):
        _lib.jmi_select("cpu", x, np.zeros(24, np.uint8), 3, 2)


def test_as_mi_check():
    for call in (_select, _rows):
        assert call(n=0)[0] == _lib.FS_EINVAL and "2^31" in call(n=0)[1]
        rc, msg = call(states=257, x=np.zeros((24, 6), np.uint8))[:2]
        assert rc == _lib.FS_EINVAL and "1..256" in msg
        rc, msg = call(unit=2)[:2]
        assert rc == _lib.FS_EINVAL and "unit" in msg
        rc, msg = call(backend=7)[:2]
        assert rc == _lib.FS_EINVAL and "backend" in msg
    assert _select(p=0, k=1)[0] == _lib.FS_EINVAL


def test_gpu_backend_rejects_more_than_32_states():
    for call in (_select, _rows):                      # with or without a device
        rc, msg = call(backend=GPU, states=33)[:2]
        assert rc == _lib.FS_EINVAL and "32 states" in msg


def test_cpu_backend_rejects_a_joint_table_beyond_2_pow_20_cells():
    """256 states of one column, squared, times 17 classes of y."""
    n = 300
    x = np.zeros((n, 2), np.uint8)
    x[:256, 0] = np.arange(256)
    y = (np.arange(n) % 17).astype(np.uint8)
    rc, msg, _, _, _ = _select(n=n, p=2, states=256, k=1, x=x, y=y)
    assert rc == _lib.FS_EINVAL and "2^20" in msg
    rc, msg, _ = _rows(n=n, p=2, states=256, anchors=(0,), x=x, y=y)
    assert rc == _lib.FS_EINVAL and "2^20" in msg
    # 16 classes are exactly 2^20 cells
    y16 = (np.arange(n) % 16).astype(np.uint8)
    rc, _, R = _rows(n=n, p=2, states=256, anchors=(0,), x=x, y=y16)
    assert rc == _lib.FS_OK and R[0, 0] == 0.0 and R[0, 1] >= 0.0


def test_search_matrix_rejections():
    lib = _lib.lib()
    rel = np.array([0.3, 0.2, 0.1])
    joint = np.zeros((3, 3))
    sel = np.zeros(3, dtype=np.int64)
    args = (rel.ctypes.data_as(_f64p), joint.ctypes.data_as(_f64p))
    s = sel.ctypes.data_as(_i64p)
    for method in (0, 1):
        assert lib.fs_jmi_search_matrix(CPU, 0, *args, 3, method, 3, s) == _lib.FS_OK
        assert sel.tolist() == [0, 1, 2]
    assert lib.fs_jmi_search_matrix(CPU, 0, *args, 3, 0, 0, s) == _lib.FS_EINVAL
    assert lib.fs_jmi_search_matrix(CPU, 0, *args, 3, 0, 4, s) == _lib.FS_EINVAL
    assert lib.fs_jmi_search_matrix(CPU, 0, *args, 3, 2, 3, s) == _lib.FS_EINVAL
    assert lib.fs_jmi_search_matrix(CPU, 0, *args, 3, 0, 3, None) == _lib.FS_EINVAL
    assert lib.fs_jmi_search_matrix(CPU, 0, None, args[1], 3, 0, 3, s) == _lib.FS_EINVAL
    assert lib.fs_jmi_search_matrix(CPU, 0, args[0], None, 3, 0, 3, s) == _lib.FS_EINVAL
    assert lib.fs_jmi_search_matrix(CPU, 0, *args, 0, 0, 1, s) == _lib.FS_EINVAL
    assert lib.fs_jmi_search_matrix(7, 0, *args, 3, 0, 3, s) == _lib.FS_EINVAL
