"""fs_pair_screen reports bad arguments the documented way (CPU only; no GPU
compute here).  The checks are shared by both backends and come before the
device check, so the GPU backend's are tested with or without a device."""
import ctypes

import numpy as np
import pytest

from fastselect_amd import _lib

CPU, GPU = _lib.BACKEND_CPU, _lib.BACKEND_GPU
_u8p = ctypes.POINTER(ctypes.c_uint8)
_f64p = ctypes.POINTER(ctypes.c_double)
_i64p = ctypes.POINTER(ctypes.c_int64)


def _screen(backend=CPU, n=24, p=6, states=3, unit=0, kind=0, n_top=4, x=None, y=None, rel=True,
            ts=True, ti=True, tj=True, fb=True):
    """fs_pair_screen through raw ctypes; returns (rc, message, relevance,
    top_score, top_i, top_j, feature_best)."""
    lib = _lib.lib()
    rng = np.random.default_rng(5)
    rows = max(n, 1)
    xa = (rng.integers(0, min(max(states, 1), 3), size=(rows, max(p, 1))).astype(np.uint8)
          if x is None else x)
    ya = (np.arange(rows) % 2).astype(np.uint8) if y is None else y
    size = min(max(n_top, 1), 70000)
    r = np.zeros(max(p, 1))
    s = np.full(size, -7.0)
    i = np.full(size, -7, dtype=np.int64)
    j = np.full(size, -7, dtype=np.int64)
    b = np.full(max(p, 1), -7.0)
    rc = lib.fs_pair_screen(
        backend, 0, None if x is False else xa.ctypes.data_as(_u8p),
        None if y is False else ya.ctypes.data_as(_u8p), n, p, states, unit, kind, n_top, 1,
        r.ctypes.data_as(_f64p) if rel else None, s.ctypes.data_as(_f64p) if ts else None,
        i.ctypes.data_as(_i64p) if ti else None, j.ctypes.data_as(_i64p) if tj else None,
        b.ctypes.data_as(_f64p) if fb else None)
    return rc, lib.fs_last_error().decode(), r, s, i, j, b


def test_symbols_are_exported():
    lib = _lib.lib()
    for name in ("fs_pair_screen", "fs_pair_screen_last_timing"):
        assert name in _lib.EXPORTED
        assert getattr(lib, name) is not None


def test_valid_call_and_null_feature_best():
    rc, _, r, s, i, j, b = _screen()
    assert rc == _lib.FS_OK
    assert (i >= 0).all() and (i < j).all() and (j < 6).all()
    assert np.all(np.diff(s) <= 0.0) and b.max() == s[0]
    rc, _, r2, s2, i2, j2, b2 = _screen(fb=False)
    assert rc == _lib.FS_OK
    assert np.array_equal(r, r2) and np.array_equal(s, s2)
    assert np.array_equal(i, i2) and np.array_equal(j, j2)
    assert (b2 == -7.0).all()


@pytest.mark.parametrize("backend", [CPU, GPU])
def test_einval_of_both_backends(backend):
    """Every check that reads no array: the same answer with or without a device."""
    for kw in ({"x": False}, {"y": False}, {"rel": False}, {"ts": False}, {"ti": False},
               {"tj": False}):
        rc, msg = _screen(backend=backend, **kw)[:2]
        assert rc == _lib.FS_EINVAL and "NULL" in msg, kw
    for p in (1, 0, -3):
        rc, msg = _screen(backend=backend, p=p)[:2]
        assert rc == _lib.FS_EINVAL and "p must be >=" in msg, p
    rc, msg = _screen(backend=backend, p=1)[:2]
    assert "p must be >= 2" in msg
    for n_top in (0, -1, 65537):
        rc, msg = _screen(backend=backend, n_top=n_top)[:2]
        assert rc == _lib.FS_EINVAL and "n_top must be in 1..65536" in msg, n_top
    for kind in (2, -1):
        rc, msg = _screen(backend=backend, kind=kind)[:2]
        assert rc == _lib.FS_EINVAL and "score_kind" in msg, kind
    rc, msg = _screen(backend=backend, n=0)[:2]
    assert rc == _lib.FS_EINVAL and "2^31" in msg
    rc, msg = _screen(backend=backend, states=257, x=np.zeros((24, 6), np.uint8))[:2]
    assert rc == _lib.FS_EINVAL and "1..256" in msg
    rc, msg = _screen(backend=backend, states=0)[:2]
    assert rc == _lib.FS_EINVAL and "1..256" in msg
    rc, msg = _screen(backend=backend, unit=2)[:2]
    assert rc == _lib.FS_EINVAL and "unit" in msg


def test_bad_backend():
    rc, msg = _screen(backend=7)[:2]
    assert rc == _lib.FS_EINVAL and "backend" in msg


def test_gpu_backend_rejects_more_than_32_states():
    rc, msg = _screen(backend=GPU, states=33)[:2]       # with or without a device
    assert rc == _lib.FS_EINVAL and "32 states" in msg


def test_gpu_backend_rejects_more_than_4_classes():
    y = (np.arange(24) % 5).astype(np.uint8)
    rc, msg = _screen(backend=GPU, states=5, y=y)[:2]    # with or without a device
    assert rc == _lib.FS_EINVAL and "4 classes" in msg
    y[3] = 7
    rc, msg = _screen(backend=GPU, states=5, y=y)[:2]
    assert rc == _lib.FS_EINVAL and ">= n_states" in msg
    assert _screen(backend=CPU, states=5, y=(np.arange(24) % 5).astype(np.uint8))[0] == _lib.FS_OK


def test_gpu_backend_out_of_memory_is_decided_on_the_sizes():
    """2^31 - 1 samples x 2^20 columns, planes of 2^50 bytes, behind arrays of
    24 rows: FS_EOOM before any array is read, with or without a device."""
    rc, msg = _screen(backend=GPU, n=2 ** 31 - 1, p=1 << 20, x=np.zeros((24, 6), np.uint8),
                      y=np.zeros(24, np.uint8))[:2]
    assert rc == _lib.FS_EOOM and "do not fit" in msg


def test_n_top_65536_is_accepted():
    rc, _, _, s, i, j, _ = _screen(n_top=65536)
    assert rc == _lib.FS_OK
    assert (i[:15] >= 0).all() and (i[15:] == -1).all() and (j[15:] == -1).all()
    assert not s[15:].any()


def test_code_equal_to_n_states():
    x = np.zeros((24, 6), np.uint8)
    x[23, 5] = 3
    y = np.zeros(24, np.uint8)
    y[5] = 3
    for rc, msg in (_screen(x=x)[:2], _screen(y=y)[:2]):
        assert rc == _lib.FS_EINVAL and ">= n_states" in msg
    with pytest.raises(ValueError, match=">= n_states"):
        _lib.pair_screen("cpu", x, np.zeros(24, np.uint8), 3)


def test_cpu_backend_rejects_a_joint_table_beyond_2_pow_20_cells():
    """256 states of one column, squared, times 17 classes of y."""
    n = 300
    x = np.zeros((n, 2), np.uint8)
    x[:256, 0] = np.arange(256)
    y = (np.arange(n) % 17).astype(np.uint8)
    rc, msg = _screen(n=n, p=2, states=256, x=x, y=y)[:2]
    assert rc == _lib.FS_EINVAL and "2^20" in msg
    y16 = (np.arange(n) % 16).astype(np.uint8)             # exactly 2^20 cells
    rc, _, _, s, i, j, _ = _screen(n=n, p=2, states=256, n_top=1, x=x, y=y16)
    assert rc == _lib.FS_OK and (i[0], j[0]) == (0, 1) and s[0] >= 0.0


def test_wrapper_rejections():
    x = np.zeros((24, 6), np.uint8)
    y = np.zeros(24, np.uint8)
    with pytest.raises(ValueError, match="score"):
        _lib.pair_screen("cpu", x, y, 3, score="sum")
    with pytest.raises(ValueError, match="unit"):
        _lib.pair_screen("cpu", x, y, 3, unit="ban")
    with pytest.raises(ValueError, match="n_top"):
        _lib.pair_screen("cpu", x, y, 3, n_top=0)
    with pytest.raises(ValueError, match="2-D"):
        _lib.pair_screen("cpu", x[:, 0], y, 3)


def test_timing_and_hooks():
    assert _lib.lib().fs_pair_screen_last_timing(None) == _lib.FS_EINVAL
    assert len(_lib.pair_screen_last_timing()) == 5
    with _lib.test_hooks(pair_tiles=1, pair_cap=64):
        pass
    lib = _lib.lib()
    assert lib.fs_test_hook(b"pair_tile", 1) == _lib.FS_EINVAL
    assert "unknown hook 'pair_tile'" in lib.fs_last_error().decode()
    assert lib.fs_test_hook(b"pair_caps", 1) == _lib.FS_EINVAL
    # the hooks do not touch the CPU backend
    x, y = np.random.default_rng(1).integers(0, 3, (40, 9)).astype(np.uint8), np.arange(40) % 2
    want = _lib.pair_screen("cpu", x, y, 3, n_top=9)
    with _lib.test_hooks(pair_tiles=1, pair_cap=64):
        got = _lib.pair_screen("cpu", x, y, 3, n_top=9)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
