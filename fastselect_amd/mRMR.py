"""mRMR estimator (reference: src/fast_select/mRMR.py:30-152).

Minimum redundancy, maximum relevance selection on discrete data: the first
feature is the most relevant one, and each further feature maximises
``I(f; y) - mean(I(f; S))`` (MID) or ``I(f; y) / (mean(I(f; S)) + 1e-9)`` (MIQ)
over the features S selected so far.

``fit`` validates and encodes as the reference (mRMR.py:82-92), makes one call
to ``fs_mi_matrices`` through ``mutual_information.calculate_mi_matrices``
(mRMR.py:94-96), and runs the greedy loop on the host in numpy exactly as
written (mRMR.py:102-134); the loop is O(k p).  It reads only the k selected
columns of the redundancy matrix; the full matrix is computed because
``redundancy_matrix_`` is a fitted attribute of the reference.

``redundancy="selected"`` is the path for callers who do not need that
attribute: after the same validation and encoding, one call to
``fs_mrmr_select`` computes the relevance and one row of mutual information per
selected feature and runs the same greedy loop natively (on the GPU: every
step queued on one stream, one synchronisation per fit).  That is k p pairs
instead of p^2 / 2 and k p float64 of results instead of p^2, so a width whose
matrix cannot be allocated (80 GB at p = 100000) still fits.

With backend='gpu' the whole redundancy matrix is computed on the GPU (the
reference computes it on the CPU whatever the backend,
mutual_information.py:191-193).
"""
from __future__ import annotations

import numpy as np
from sklearn.base import BaseEstimator, TransformerMixin
from sklearn.utils.validation import check_is_fitted, validate_data

from . import _base, _lib
from . import mutual_information as mi


class mRMR(TransformerMixin, BaseEstimator):
    """mRMR feature selection for discrete data on the MI355X or the CPU.

    Parameters
    ----------
    n_features_to_select : int
        Number of features to select.
    method : {'MID', 'MIQ'}, default='MID'
        Difference or quotient of relevance and mean redundancy.
    backend : {'cpu', 'gpu', 'auto'}, default='cpu'
        'gpu' without a visible HIP device raises; it never falls back.
        'auto' (not a reference value) uses the GPU when one is visible and
        the data has at most 32 states.
    n_jobs : int, default=-1
        CPU threads for backend='cpu' (-1 = all).  Not a reference parameter.
    device : int, default=0
        GPU ordinal for the GPU backend.  Not a reference parameter.
    redundancy : {'matrix', 'selected'}, default='matrix'
        Not a reference parameter.  'matrix' computes the whole p x p
        redundancy matrix (p^2 / 2 pairs, 8 p^2 bytes on the device and the
        host) and keeps it as ``redundancy_matrix_``, as the reference does.
        'selected' computes only the rows of the selected features (k p pairs,
        8 k p bytes), selects the same features from the same values, and sets
        ``redundancy_rows_`` instead of ``redundancy_matrix_``.

    Attributes
    ----------
    relevance_scores_ : ndarray of float64, shape (n_features,)
    redundancy_matrix_ : ndarray of float64, shape (n_features, n_features)
        With redundancy='matrix' only.
    redundancy_rows_ : ndarray of float64, shape (n_features_to_select, n_features)
        With redundancy='selected' only: ``redundancy_rows_[s]`` is row
        ``top_features_[s]`` of the matrix.
    top_features_ : ndarray of int32, shape (n_features_to_select,)
    feature_importances_ : ndarray (the relevance scores)
    n_features_in_, unique_vals_, effective_backend_
    """

    def __init__(self, n_features_to_select: int, method: str = "MID", backend: str = "cpu",
                 n_jobs: int = -1, device: int = 0, redundancy: str = "matrix"):
        self.n_features_to_select = n_features_to_select
        self.method = method
        self.backend = backend
        self.n_jobs = n_jobs
        self.device = device
        self.redundancy = redundancy
        if self.method not in ["MID", "MIQ"]:
            raise ValueError("Method must be either 'MID' or 'MIQ'.")
        if self.backend not in ["cpu", "gpu", "auto"]:
            raise ValueError("Backend must be either 'cpu' or 'gpu' (or 'auto').")
        if self.redundancy not in ["matrix", "selected"]:
            raise ValueError("redundancy must be either 'matrix' or 'selected'.")
        if self.backend == "gpu" and not _lib.gpu_available():
            raise RuntimeError(_base.GPU_MISSING)

    def fit(self, X, y):
        """Select ``n_features_to_select`` features of the discrete X."""
        X, y = validate_data(self, X, y, dtype=None, y_numeric=True, ensure_2d=True)
        self.n_features_in_ = X.shape[1]
        if not (0 < self.n_features_to_select <= self.n_features_in_):
            raise ValueError(
                "n_features_to_select must be a positive integer less "
                "than or equal to the number of features."
            )
        unique_vals = np.unique(np.concatenate([np.unique(X), np.unique(y)]))
        self.unique_vals_ = unique_vals
        # _encode_data_numba (mRMR.py:9-27): searchsorted codes in the inputs'
        # own dtypes, so a float X stays float and is rejected below
        X_encoded = np.searchsorted(unique_vals, X).astype(X.dtype)
        y_encoded = np.searchsorted(unique_vals, y).astype(y.dtype)

        backend = self.backend
        if backend == "auto" and unique_vals.size > mi._MAX_STATES_GPU:
            backend = "cpu"
        self.effective_backend_ = _base.effective_backend(backend)
        if self.redundancy == "selected":
            return self._fit_selected(X_encoded, y_encoded)
        relevance, redundancy = mi.calculate_mi_matrices(
            X_encoded, y_encoded, backend=self.effective_backend_, unit="bit",
            n_jobs=self.n_jobs, device=self.device)
        self.relevance_scores_ = relevance
        self.redundancy_matrix_ = redundancy

        selected_indices = np.zeros(self.n_features_to_select, dtype=np.int32)
        remaining_mask = np.ones(self.n_features_in_, dtype=bool)
        first_idx = np.argmax(self.relevance_scores_)
        selected_indices[0] = first_idx
        remaining_mask[first_idx] = False
        redundancy_sum = self.redundancy_matrix_[:, first_idx].copy()
        for i in range(1, self.n_features_to_select):
            remaining = np.where(remaining_mask)[0]
            if self.method == "MID":
                scores = self.relevance_scores_[remaining] - (redundancy_sum[remaining] / i)
            else:
                scores = self.relevance_scores_[remaining] / ((redundancy_sum[remaining] / i) + 1e-9)
            max_score = np.max(scores)
            top_candidates = remaining[np.isclose(scores, max_score, atol=1e-12)]
            if top_candidates.size > 1:
                avg_redundancy = redundancy_sum[top_candidates] / i
                best = top_candidates[np.argmin(avg_redundancy)]
            else:
                best = top_candidates[0]
            selected_indices[i] = best
            remaining_mask[best] = False
            redundancy_sum += self.redundancy_matrix_[:, best]

        self.top_features_ = selected_indices
        self.feature_importances_ = self.relevance_scores_
        return self

    def _fit_selected(self, X_encoded, y_encoded):
        """The relevance, the selection and the selected features' rows in one
        ``fs_mrmr_select`` call, behind calculate_mi_matrices' own checks
        (mutual_information.py:171-182)."""
        if X_encoded.ndim != 2 or y_encoded.ndim != 1 or X_encoded.shape[0] != y_encoded.shape[0]:
            raise ValueError("X must be 2‑D and y 1‑D with matching sample size")
        X_d = mi._validate_discrete(X_encoded, "X")
        y_d = mi._validate_discrete(y_encoded, "y")
        max_state = int(max(X_d.max(), y_d.max())) + 1
        where = mi._choose_backend(self.effective_backend_, max_state)
        selected, relevance, rows = _lib.mrmr_select(
            where, X_d, y_d, max_state, self.n_features_to_select, method=self.method,
            unit="bit", n_jobs=self.n_jobs, device=self.device)
        self.relevance_scores_ = relevance
        self.redundancy_rows_ = rows
        self.top_features_ = selected.astype(np.int32)
        self.feature_importances_ = self.relevance_scores_
        return self

    def transform(self, X):
        """Reduce X to the selected features."""
        check_is_fitted(self)
        X = validate_data(self, X, reset=False, dtype=None)
        return X[:, self.top_features_]

    def fit_transform(self, X, y):
        self.fit(X, y)
        return self.transform(X)
