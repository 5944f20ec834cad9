"""fs_pair_screen_labels on the CPU backend: the documented rejections (shared
by both backends and placed before the device check, so the GPU backend's are
tested with or without a device), and the identity that defines the call, with
no tolerance: row b is the first entry and the relevance of
fs_pair_screen(codes, labels[b], n_top = 1) on the same backend."""
import ctypes

import numpy as np
import pytest

import mi_np
import pairscan_np
from fastselect_amd import _lib

CPU, GPU = _lib.BACKEND_CPU, _lib.BACKEND_GPU
_u8p = ctypes.POINTER(ctypes.c_uint8)
_f64p = ctypes.POINTER(ctypes.c_double)
_i64p = ctypes.POINTER(ctypes.c_int64)
SCORES = ("joint", "gain")


def _call(backend=CPU, n=24, p=6, states=3, unit=0, kind=0, B=3, x=None, labels=None, bs=True,
          bi=True, bj=True, rel=True):
    """fs_pair_screen_labels through raw ctypes; returns (rc, message,
    best_score, best_i, best_j, relevance)."""
    lib = _lib.lib()
    rng = np.random.default_rng(5)
    rows, nb = max(n, 1), min(max(B, 1), 70000)
    xa = (rng.integers(0, min(max(states, 1), 3), size=(rows, max(p, 1))).astype(np.uint8)
          if x is None else x)
    la = (rng.integers(0, 2, size=(nb, rows)).astype(np.uint8) if labels is None else labels)
    s = np.full(nb, -7.0)
    i = np.full(nb, -7, dtype=np.int64)
    j = np.full(nb, -7, dtype=np.int64)
    r = np.full((nb, max(p, 1)), -7.0)
    rc = lib.fs_pair_screen_labels(
        backend, 0, None if x is False else xa.ctypes.data_as(_u8p),
        None if labels is False else la.ctypes.data_as(_u8p), B, n, p, states, unit, kind, 1,
        s.ctypes.data_as(_f64p) if bs else None, i.ctypes.data_as(_i64p) if bi else None,
        j.ctypes.data_as(_i64p) if bj else None, r.ctypes.data_as(_f64p) if rel else None)
    return rc, lib.fs_last_error().decode(), s, i, j, r


def test_symbols_are_exported():
    lib = _lib.lib()
    for name in ("fs_pair_screen_labels", "fs_pair_labels_last_timing"):
        assert name in _lib.EXPORTED
        assert getattr(lib, name) is not None


def test_valid_call_and_null_relevance():
    rc, _, s, i, j, r = _call()
    assert rc == _lib.FS_OK
    assert (i >= 0).all() and (i < j).all() and (j < 6).all() and (r != -7.0).all()
    rc, _, s2, i2, j2, r2 = _call(rel=False)
    assert rc == _lib.FS_OK
    assert np.array_equal(s, s2) and np.array_equal(i, i2) and np.array_equal(j, j2)
    assert (r2 == -7.0).all()


@pytest.mark.parametrize("backend", [CPU, GPU])
def test_einval_of_both_backends(backend):
    """Every check that reads no array: the same answer with or without a device."""
    for kw in ({"x": False}, {"labels": False}, {"bs": False}, {"bi": False}, {"bj": False}):
        rc, msg = _call(backend=backend, **kw)[:2]
        assert rc == _lib.FS_EINVAL and "NULL" in msg, kw
    for B in (0, -1, 65536):
        rc, msg = _call(backend=backend, B=B)[:2]
        assert rc == _lib.FS_EINVAL and "n_labelings must be in 1..65535" in msg, B
    for p in (1, 0, -3):
        rc, msg = _call(backend=backend, p=p)[:2]
        assert rc == _lib.FS_EINVAL and "p must be >=" in msg, p
    assert "p must be >= 2" in _call(backend=backend, p=1)[1]
    for kind in (2, -1):
        rc, msg = _call(backend=backend, kind=kind)[:2]
        assert rc == _lib.FS_EINVAL and "score_kind" in msg, kind
    rc, msg = _call(backend=backend, n=0)[:2]
    assert rc == _lib.FS_EINVAL and "2^31" in msg
    for states in (0, 257):
        rc, msg = _call(backend=backend, states=states, x=np.zeros((24, 6), np.uint8))[:2]
        assert rc == _lib.FS_EINVAL and "1..256" in msg
    rc, msg = _call(backend=backend, unit=2)[:2]
    assert rc == _lib.FS_EINVAL and "unit" in msg


def test_bad_backend():
    rc, msg = _call(backend=7)[:2]
    assert rc == _lib.FS_EINVAL and "backend" in msg


@pytest.mark.parametrize("backend", [CPU, GPU])
def test_label_code_equal_to_n_states(backend):
    labels = np.zeros((3, 24), np.uint8)
    labels[2, 23] = 3                       # the last entry of the last row
    rc, msg = _call(backend=backend, labels=labels)[:2]
    assert rc == _lib.FS_EINVAL and ">= n_states" in msg
    if backend == CPU:
        with pytest.raises(ValueError, match=">= n_states"):
            _lib.pair_screen_labels("cpu", np.zeros((24, 6), np.uint8), labels, 3)


def test_column_code_equal_to_n_states():
    x = np.zeros((24, 6), np.uint8)
    x[23, 5] = 3
    rc, msg = _call(x=x)[:2]
    assert rc == _lib.FS_EINVAL and ">= n_states" in msg


def test_gpu_backend_limits_need_no_device():
    rc, msg = _call(backend=GPU, states=33)[:2]
    assert rc == _lib.FS_EINVAL and "32 states" in msg
    # five classes over all rows: no single row has more than three
    labels = np.zeros((3, 24), np.uint8)
    labels[0] = np.arange(24) % 3
    labels[1, :4] = (3, 4, 3, 4)
    rc, msg = _call(backend=GPU, states=5, labels=labels)[:2]
    assert rc == _lib.FS_EINVAL and "4 classes" in msg
    assert _call(backend=CPU, states=5, labels=labels)[0] == _lib.FS_OK
    # 2^31 - 1 samples x 2^20 columns behind arrays of 24 rows: no array is read
    for states in (3, 9):
        rc, msg = _call(backend=GPU, n=2 ** 31 - 1, p=1 << 20, states=states,
                        x=np.zeros((24, 6), np.uint8), labels=np.zeros((3, 24), np.uint8))[:2]
        assert rc == _lib.FS_EOOM and "do not fit" in msg


def test_gpu_backend_without_a_device_is_the_usual_error():
    if _lib.device_count() > 0:
        assert _call(backend=GPU)[0] == _lib.FS_OK
        return
    rc, msg = _call(backend=GPU)[:2]
    assert rc == _lib.FS_ENODEV and "no HIP device" in msg
    with pytest.raises(RuntimeError, match="no HIP device"):
        _lib.pair_screen_labels("gpu", np.zeros((24, 6), np.uint8), np.zeros((2, 24), np.uint8), 3)


def test_timing_and_hooks():
    assert _lib.lib().fs_pair_labels_last_timing(None) == _lib.FS_EINVAL
    assert len(_lib.pair_labels_last_timing()) == 5
    lib = _lib.lib()
    assert lib.fs_test_hook(b"pair_label", 64) == _lib.FS_EINVAL
    # the hooks do not touch the CPU backend
    x = np.random.default_rng(1).integers(0, 3, (40, 9)).astype(np.uint8)
    labels = np.random.default_rng(2).integers(0, 2, (5, 40)).astype(np.uint8)
    want = _lib.pair_screen_labels("cpu", x, labels, 3, want_relevance=True)
    with _lib.test_hooks(pair_labels=64, pair_lab_ranks=8):
        got = _lib.pair_screen_labels("cpu", x, labels, 3, want_relevance=True)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_wrapper_rejections():
    x = np.zeros((24, 6), np.uint8)
    labels = np.zeros((2, 24), np.uint8)
    with pytest.raises(ValueError, match="score"):
        _lib.pair_screen_labels("cpu", x, labels, 3, score="sum")
    with pytest.raises(ValueError, match="unit"):
        _lib.pair_screen_labels("cpu", x, labels, 3, unit="ban")
    with pytest.raises(ValueError, match="2-D"):
        _lib.pair_screen_labels("cpu", x, labels[0], 3)
    with pytest.raises(ValueError, match="2-D"):
        _lib.pair_screen_labels("cpu", x, labels[:, :5], 3)
    with pytest.raises(ValueError, match="labellings"):
        _lib.pair_screen_labels("cpu", x, labels[:0], 3)


# ---- the identity ----------------------------------------------------------

def _perms(y, B, seed):
    """Row 0 is y, the others are permutations of it."""
    rng = np.random.default_rng(seed)
    return np.stack([y] + [rng.permutation(y) for _ in range(B - 1)]).astype(np.uint8)


def _planted():
    X, y = pairscan_np.pure(*pairscan_np.PLANTED[0][0])
    return X[:, :20].astype(np.uint8), _perms(y, 6, 1), 2


def _tied():
    X, y, S = pairscan_np.tied()
    labels = _perms(y, 5, 2)
    labels[1] = labels[0]
    labels[3] = 0                           # a one-class row
    return X, labels, S


def _all_constant():
    X, y, S = pairscan_np.all_constant()
    return X, _perms(y, 4, 3), S


def _mixed():
    """Columns of 2..5 states and four classes; one row takes two of them."""
    rng = np.random.default_rng(77)
    X = np.stack([rng.integers(0, 2 + f % 4, 120) for f in range(9)], axis=1).astype(np.uint8)
    y = rng.integers(0, 4, 120)
    labels = _perms(y, 5, 4)
    labels[2] = labels[2] % 2
    return X, labels, 5


def _single():
    X, y = mi_np.uniform(65, 7, 3, 31, 2)
    return X, _perms(y, 1, 5), 3


CASES = {"planted": _planted, "tied": _tied, "all_constant": _all_constant, "mixed": _mixed,
         "single": _single}


def _assert_rows_are_single_calls(L, backend, X, labels, S, score, got):
    best, pairs, rel = got
    for b in range(labels.shape[0]):
        r1, s1, p1, _ = L.pair_screen(backend, X, labels[b], S, n_top=1, score=score,
                                      want_feature_best=False)
        assert np.array_equal(best[b:b + 1], s1), (b, best[b], s1)
        assert np.array_equal(pairs[b:b + 1], p1), (b, pairs[b], p1)
        assert np.array_equal(rel[b], r1), b
        assert not np.signbit(best[b])


@pytest.mark.parametrize("score", SCORES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_rows_are_the_single_calls(case, score):
    X, labels, S = CASES[case]()
    got = _lib.pair_screen_labels("cpu", X, labels, S, score=score, want_relevance=True)
    assert got[0].shape == (labels.shape[0],) and got[1].shape == (labels.shape[0], 2)
    _assert_rows_are_single_calls(_lib, "cpu", X, labels, S, score, got)
    if case == "all_constant":
        assert not got[0].any() and (got[1] == (0, 1)).all() and not got[2].any()
    if case == "tied":
        assert got[0][3] == 0.0 and tuple(got[1][3]) == (0, 1) and not got[2][3].any()
        assert got[0][1] == got[0][0] and tuple(got[1][1]) == tuple(got[1][0])


@pytest.mark.parametrize("score", SCORES)
def test_n_jobs_changes_no_bit(score):
    X, y = pairscan_np.pure(*pairscan_np.PLANTED[0][0])
    X = X.astype(np.uint8)                  # 780 pairs: several runs of ranks
    labels = _perms(y, 4, 6)
    want = _lib.pair_screen_labels("cpu", X, labels, 2, score=score, n_jobs=1, want_relevance=True)
    for n_jobs in (3, -1):
        got = _lib.pair_screen_labels("cpu", X, labels, 2, score=score, n_jobs=n_jobs,
                                      want_relevance=True)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), n_jobs
