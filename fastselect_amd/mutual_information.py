"""Discrete mutual information (reference: src/fast_select/mutual_information.py).

``calculate_mi_matrices`` returns the relevance vector I(X_f; y) and the
p x p redundancy matrix I(X_i; X_j) of integer-coded data;
``calculate_mi_single_pair`` one value.  Both keep the reference's shape
checks (mutual_information.py:128-129, 171-172) and ``_validate_discrete``
(mutual_information.py:13-22), then make one call to ``fs_mi_matrices``, which
replaces ``_batch_mi_cpu`` and ``_mi_pair_gpu_kernel``
(mutual_information.py:49-115).

Differences from the reference, on purpose:

* backend='gpu' computes the whole matrix on the GPU.  The reference's GPU
  path computes only the relevance there, with a kernel that strides the
  samples by ``blockIdx`` and accumulates in float32
  (mutual_information.py:84-90, 184-190), and hands the matrix to the CPU
  (mutual_information.py:191-193).  Here both backends evaluate the float64
  expressions of ``_mi_pair_cpu`` (mutual_information.py:31-46) on exact
  integer tables.
* More than 256 states is a ``ValueError``: codes travel as bytes.  The
  reference's CPU path has no cap.
* ``_mi_pair_cpu`` is ``@njit(fastmath=True)``, which lets LLVM reassociate its
  float64 sums; no reference-produced fixture pins numba's own bits, so parity
  with them is unpinned (as for MDR).
"""
from __future__ import annotations

import numpy as np

from . import _lib

_MAX_STATES_GPU = 32   # mutual_information.py:66
_MAX_STATES = 256      # state codes are bytes at the native boundary


def _validate_discrete(arr: np.ndarray, name: str) -> np.ndarray:
    """Integer dtype and no negative entry (mutual_information.py:13-22)."""
    if not np.issubdtype(arr.dtype, np.integer):
        raise ValueError(
            f"{name} must be an integer‑coded array (got {arr.dtype}). "
            "Discretise continuous data before calling this function."
        )
    if arr.min() < 0:
        raise ValueError(f"{name} contains negative values; expected 0..K‑1 codes.")
    return arr


def _choose_backend(backend: str, max_state: int) -> str:
    """The reference's dispatch (mutual_information.py:137-154, 180-182):
    'gpu' as asked, 'auto' on the GPU when a device is visible and the states
    fit; 'gpu' never falls back."""
    if max_state > _MAX_STATES:
        raise ValueError(
            f"at most {_MAX_STATES} states are supported (got {max_state}): "
            "state codes are stored as bytes")
    if backend == "auto":
        return "gpu" if _lib.gpu_available() and max_state <= _MAX_STATES_GPU else "cpu"
    if backend == "gpu":
        if not _lib.gpu_available():
            raise RuntimeError("backend='gpu' requested but no HIP device is visible")
        if max_state > _MAX_STATES_GPU:
            raise RuntimeError(
                f"GPU backend supports ≤{_MAX_STATES_GPU} states (got {max_state}); "
                "try backend='cpu'")
        return "gpu"
    if backend != "cpu":
        raise ValueError("backend must be 'auto', 'cpu' or 'gpu'")
    return "cpu"


def calculate_mi_single_pair(x1, x2, *, backend="auto", unit="bit", n_jobs=-1, device=0) -> float:
    """Mutual information I(x1; x2) of two integer-coded 1-D arrays
    (mutual_information.py:117-155)."""
    x1 = np.asarray(x1)
    x2 = np.asarray(x2)
    if x1.ndim != 1 or x2.ndim != 1 or x1.shape != x2.shape:
        raise ValueError("x1 and x2 must be 1‑D arrays of equal length")
    x1_d = _validate_discrete(x1.ravel(), "x1")
    x2_d = _validate_discrete(x2.ravel(), "x2")
    max_state = int(max(x1_d.max(), x2_d.max())) + 1
    where = _choose_backend(backend, max_state)
    rel, _ = _lib.mi_matrices(where, x1_d.reshape(-1, 1), x2_d, max_state, unit=unit,
                              n_jobs=n_jobs, device=device)
    return float(rel[0])


def calculate_mi_matrices(X, y, *, backend="auto", unit="bit", n_jobs=-1, device=0):
    """(relevance, redundancy) of integer-coded X (n x p) and y (n)
    (mutual_information.py:158-196).  ``n_jobs`` and ``device`` are not
    reference parameters."""
    X = np.asarray(X)
    y = np.asarray(y)
    if X.ndim != 2 or y.ndim != 1 or X.shape[0] != y.shape[0]:
        raise ValueError("X must be 2‑D and y 1‑D with matching sample size")
    X_d = _validate_discrete(X, "X")
    y_d = _validate_discrete(y, "y")
    max_state = int(max(X_d.max(), y_d.max())) + 1
    where = _choose_backend(backend, max_state)
    return _lib.mi_matrices(where, X_d, y_d, max_state, unit=unit, n_jobs=n_jobs, device=device)


_MAX_CLASSES_GPU = 4   # fs_jmi.h kJmiMaxClassesGpu: classes of y in the joint-relevance kernel


def _choose_backend_joint(backend: str, max_state: int, n_classes: int) -> str:
    """``_choose_backend`` extended by the joint-relevance kernel's class limit:
    'auto' takes the CPU beyond either GPU limit, 'gpu' raises."""
    if backend == "auto" and n_classes > _MAX_CLASSES_GPU:
        return _choose_backend("cpu", max_state)
    where = _choose_backend(backend, max_state)
    if where == "gpu" and n_classes > _MAX_CLASSES_GPU:
        raise RuntimeError(
            f"GPU backend supports ≤{_MAX_CLASSES_GPU} classes of y for joint relevance "
            f"(got {n_classes}); try backend='cpu'")
    return where


def calculate_joint_relevance(X, y, anchors, *, backend="auto", unit="bit", n_jobs=-1, device=0):
    """Joint relevance ``I(X_c, X_a; y)`` of every column c with each anchor
    column a of integer-coded X (n x p) and y (n): float64 [len(anchors), p],
    0.0 where c == a (``fs_jmi_rows``).  Not a reference function: it is the
    quantity the ``JMI`` estimator selects by."""
    X = np.asarray(X)
    y = np.asarray(y)
    if X.ndim != 2 or y.ndim != 1 or X.shape[0] != y.shape[0]:
        raise ValueError("X must be 2‑D and y 1‑D with matching sample size")
    X_d = _validate_discrete(X, "X")
    y_d = _validate_discrete(y, "y")
    anchors = np.atleast_1d(np.asarray(anchors))
    if anchors.ndim != 1 or anchors.size < 1 or not np.issubdtype(anchors.dtype, np.integer):
        raise ValueError("anchors must be a non-empty vector of column indices")
    if anchors.min() < 0 or anchors.max() >= X.shape[1]:
        raise ValueError("an anchor is outside 0..p-1")
    max_state = int(max(X_d.max(), y_d.max())) + 1
    where = _choose_backend_joint(backend, max_state, int(y_d.max()) + 1)
    return _lib.jmi_rows(where, X_d, y_d, max_state, anchors, unit=unit, n_jobs=n_jobs,
                         device=device)


def rank_pair_interactions(X, y, n_top=100, *, score="gain", backend="auto", unit="bit", n_jobs=-1,
                           device=0):
    """The ``n_top`` best of all C(p,2) column pairs of integer-coded X (n x p)
    by what they say about y (n) together (``fs_pair_screen``): an exhaustive
    scan, returned as a ranked list and never as a p x p matrix.

    ``score="joint"`` ranks by the joint relevance ``J(i, j) = I(X_i, X_j; y)``,
    the quantity of ``calculate_joint_relevance``; ``score="gain"`` by the
    interaction information ``(J(i, j) - I(X_i; y)) - I(X_j; y)``, positive for
    a pair that says more together than apart.  The list is ordered by (score
    descending, place in ``itertools.combinations(range(p), 2)`` ascending).

    Returns (top_pairs int64 [m, 2] with i < j, top_scores float64 [m],
    relevance float64 [p], feature_best float64 [p]: the largest score of any
    pair that contains the feature), ``m = min(n_top, C(p,2))``.  Not a
    reference function."""
    X = np.asarray(X)
    y = np.asarray(y)
    if X.ndim != 2 or y.ndim != 1 or X.shape[0] != y.shape[0]:
        raise ValueError("X must be 2‑D and y 1‑D with matching sample size")
    X_d = _validate_discrete(X, "X")
    y_d = _validate_discrete(y, "y")
    if X.shape[1] < 2:
        raise ValueError("X must have at least two columns")
    if not (1 <= int(n_top) <= _lib.PAIR_MAX_TOP):
        raise ValueError(f"n_top must be in 1..{_lib.PAIR_MAX_TOP}")
    max_state = int(max(X_d.max(), y_d.max())) + 1
    where = _choose_backend_joint(backend, max_state, int(y_d.max()) + 1)
    rel, top_s, top_p, best = _lib.pair_screen(where, X_d, y_d, max_state, n_top=n_top, score=score,
                                               unit=unit, n_jobs=n_jobs, device=device)
    return top_p, top_s, rel, best


def pair_screen_null(X, labels, *, score="gain", backend="auto", unit="bit", n_jobs=-1, device=0):
    """The best pair of ``rank_pair_interactions(X, labels[b], n_top=1)`` for
    every row b of integer-coded ``labels`` (B x n) in one pass
    (``fs_pair_screen_labels``): several traits at once, or the null of a
    caller's own permutation scheme.  The rows are arbitrary.

    Returns (best_pairs int64 [B, 2] with i < j, best_scores float64 [B],
    relevance float64 [B, p]).  Not a reference function."""
    X = np.asarray(X)
    labels = np.asarray(labels)
    if X.ndim != 2 or labels.ndim != 2 or X.shape[0] != labels.shape[1]:
        raise ValueError("X must be 2‑D and labels 2‑D with one column per sample")
    X_d = _validate_discrete(X, "X")
    l_d = _validate_discrete(labels, "labels")
    if X.shape[1] < 2:
        raise ValueError("X must have at least two columns")
    if not (1 <= labels.shape[0] <= _lib.PAIR_MAX_LABELINGS):
        raise ValueError(f"labels must have 1..{_lib.PAIR_MAX_LABELINGS} rows")
    max_state = int(max(X_d.max(), l_d.max())) + 1
    where = _choose_backend_joint(backend, max_state, int(l_d.max()) + 1)
    best_s, best_p, rel = _lib.pair_screen_labels(where, X_d, l_d, max_state, score=score,
                                                  unit=unit, n_jobs=n_jobs, device=device,
                                                  want_relevance=True)
    return best_p, best_s, rel
