"""JMI and CMIM estimators: interaction-aware selection on discrete data.

``mRMR`` and ``CFS`` rank a candidate by its own relevance and penalise what it
shares with the selected set, so a feature that matters only together with
another one (an epistatic SNP) never reaches the top.  The criteria here score
a candidate f by its joint relevance with the features S selected so far:

* JMI (Yang & Moody): ``sum_{s in S} I(X_f, X_s; y)``;
* CMIM (Fleuret): ``min_{s in S} I(X_f; y | X_s)``, which is
  ``I(X_f, X_s; y) - I(X_s; y)``.

The first feature is the most relevant one; every later step takes the
unselected feature with the largest score, the lowest index among exact
equals.  There is no reference implementation of these two in ``fast_select``;
the definitions are in ``csrc/fs_jmi.h``.

``fit`` encodes every column and y by their own sorted unique values and makes
one call to ``fs_jmi_select``, which computes the relevance and one row of
joint relevance per selected feature (k p three-way tables, nothing of size
p x p) and runs the greedy loop natively: on the GPU every step is queued on
one stream with one synchronisation per fit.
"""
from __future__ import annotations

import numpy as np
from sklearn.base import BaseEstimator, TransformerMixin
from sklearn.utils.validation import check_is_fitted, validate_data

from . import _base, _lib
from . import mutual_information as mi


class JMI(TransformerMixin, BaseEstimator):
    """JMI / CMIM feature selection for discrete data on the MI355X or the CPU.

    Parameters
    ----------
    n_features_to_select : int
        Number of features to select.
    method : {'JMI', 'CMIM'}, default='JMI'
        Sum of the joint relevances with the selected features, or minimum of
        the conditional relevances given each of them.
    backend : {'auto', 'cpu', 'gpu'}, default='auto'
        'gpu' without a visible HIP device, with more than 32 states in a
        column or more than 4 classes of y raises; it never falls back.
        'auto' uses the GPU when one is visible and the data is within both
        limits, else the CPU.
    n_jobs : int, default=-1
        CPU threads for the CPU backend (-1 = all).
    device : int, default=0
        GPU ordinal for the GPU backend.
    unit : {'bit', 'nat'}, default='bit'

    Attributes
    ----------
    top_features_ : ndarray of int32, shape (n_features_to_select,)
        In selection order.
    relevance_scores_ : ndarray of float64, shape (n_features,)
        ``I(X_f; y)``, the values ``mRMR`` computes.
    feature_importances_ : ndarray (the relevance scores)
    joint_relevance_rows_ : ndarray of float64, shape (n_features_to_select, n_features)
        ``joint_relevance_rows_[s, c] = I(X_c, X_top_features_[s]; y)``, 0 at
        ``c == top_features_[s]``.
    n_features_in_, effective_backend_
    """

    def __init__(self, n_features_to_select: int, method: str = "JMI", backend: str = "auto",
                 n_jobs: int = -1, device: int = 0, unit: str = "bit"):
        self.n_features_to_select = n_features_to_select
        self.method = method
        self.backend = backend
        self.n_jobs = n_jobs
        self.device = device
        self.unit = unit

    def fit(self, X, y):
        """Select ``n_features_to_select`` features of the discrete X."""
        if self.method not in _lib.JMI_METHODS:
            raise ValueError("method must be either 'JMI' or 'CMIM'.")
        if self.backend not in ("auto", "cpu", "gpu"):
            raise ValueError("backend must be 'auto', 'cpu' or 'gpu'")
        if self.unit not in _lib.MI_UNITS:
            raise ValueError("unit must be 'bit' or 'nat'")
        X, y = validate_data(self, X, y, dtype=None, ensure_2d=True)
        n, p = X.shape
        self.n_features_in_ = p
        if not (0 < self.n_features_to_select <= p):
            raise ValueError(
                "n_features_to_select must be a positive integer less "
                "than or equal to the number of features."
            )
        # every column and y by their own sorted unique values
        codes = np.empty((n, p), dtype=np.uint8)
        max_state = 1
        for f in range(p):
            vals, inv = np.unique(X[:, f], return_inverse=True)
            if vals.size > mi._MAX_STATES:
                raise ValueError(
                    f"column {f} takes {vals.size} values; at most {mi._MAX_STATES} are "
                    "supported: discretise continuous data first")
            codes[:, f] = inv.reshape(n)
            max_state = max(max_state, int(vals.size))
        yvals, yinv = np.unique(y, return_inverse=True)
        if yvals.size > mi._MAX_STATES:
            raise ValueError(
                f"y takes {yvals.size} values; at most {mi._MAX_STATES} are supported: "
                "discretise it first")
        ycodes = yinv.reshape(n).astype(np.uint8)
        n_states = max(max_state, int(yvals.size))

        where = mi._choose_backend_joint(self.backend, n_states, int(yvals.size))
        self.effective_backend_ = where
        selected, relevance, rows = _lib.jmi_select(
            where, codes, ycodes, n_states, self.n_features_to_select, method=self.method,
            unit=self.unit, n_jobs=self.n_jobs, device=self.device)
        self.relevance_scores_ = relevance
        self.joint_relevance_rows_ = rows
        self.top_features_ = selected.astype(np.int32)
        self.feature_importances_ = self.relevance_scores_
        return self

    def transform(self, X):
        """Reduce X to the selected features."""
        check_is_fitted(self)
        X = validate_data(self, X, reset=False, dtype=None)
        return X[:, self.top_features_]
