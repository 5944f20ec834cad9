"""CFS estimator (reference: src/fast_select/CFS.py:246-429).

Correlation-based feature selection: a subset is good when its features
correlate with the class and not with each other.  The correlation is the
symmetrical uncertainty ``SU(x, y) = 2 I(x; y) / (H(x) + H(y))`` of the
discretised columns, the merit of a subset of k features is
``k r_cf / sqrt(k + k (k - 1) r_ff)`` over its mean class correlation and
mean pairwise correlation, and a greedy best-first search adds the feature that
raises the merit most until none does.

``fit`` validates and encodes as the reference (CFS.py:313-337) and hands the
codes to one native handle (``_lib.Cfs``).  The reference computes the whole
p x p matrix of SU before it searches (CFS.py:345-374); the search reads only
the class correlations and one row per selected feature, so the handle
computes each row when the search selects its feature, with the same bits.
The search runs natively (CFS.py:115-162); the prune and the final merit stay
in numpy as written (CFS.py:106-112, 379-399) on the rows the search holds.

Deviations, all stated: ``device`` and ``min_r_cf`` are not reference
parameters (the reference's search has ``min_r_cf=0.1`` as a default that its
estimator never overrides, CFS.py:115, 377; the default here is the same);
``backend='auto'`` answers from the CPU above 32 states, where the reference
would raise; the CPU backend takes at most 256 states (the codes are bytes).
"""
from __future__ import annotations

import math

import numpy as np
from sklearn.base import BaseEstimator
from sklearn.feature_selection import SelectorMixin
from sklearn.preprocessing import KBinsDiscretizer
from sklearn.utils.validation import check_is_fitted, check_X_y

from . import _lib
from .SURF import SURF_GPU_MISSING

_MAX_STATES_GPU = 32
_MAX_STATES_CPU = 256


def _cfs_merit(sum_r_cf, k, sum_r_ff):
    """CFS.py:11-23 on Python floats (numba's float64 typing)."""
    if k == 0:
        return 0.0
    r_cf_avg = sum_r_cf / k
    r_ff_avg = (2.0 * sum_r_ff) / (k * (k - 1)) if k > 1 else 0.0
    denom = math.sqrt(k + k * (k - 1) * r_ff_avg)
    return (k * r_cf_avg / denom) if denom > 1e-12 else 0.0


def _prune_redundant(selected, r_cf, r_ff_row):
    """CFS.py:106-112: in descending r_cf order, drop a feature as correlated
    with an already kept one as with the class.  ``r_ff_row(i)`` is row i."""
    kept = []
    for idx in sorted(selected, key=lambda i: -r_cf[i]):
        row = r_ff_row(idx)
        if not any(row[j] >= r_cf[idx] for j in kept):
            kept.append(idx)
    return kept


class CFS(SelectorMixin, BaseEstimator):
    """Correlation-based feature selection on the MI355X or the CPU.

    Parameters
    ----------
    n_bins : int, default=10
        Bins for discretising a floating-point X.
    strategy : {'uniform', 'quantile', 'kmeans'}, default='uniform'
        Binning strategy (``KBinsDiscretizer``).
    backend : {'auto', 'gpu', 'cpu'}, default='auto'
        'auto' uses the GPU when one is visible and the data has at most 32
        states.  'gpu' without a visible HIP device raises; it never falls back.
    n_jobs : int, default=-1
        CPU threads for backend='cpu' (-1 = all).
    device : int, default=0
        GPU ordinal for the GPU backend.  Not a reference parameter.
    min_r_cf : float, default=0.1
        The search ignores features whose class correlation is below this, and
        selects nothing when the best one is (``_best_first_search``'s
        ``min_r_cf``, which the reference's estimator leaves at 0.1).  Not a
        reference parameter: genotype data, whose single-SNP effects rarely
        reach a symmetrical uncertainty of 0.1, needs a lower value.

    Attributes
    ----------
    selected_indices_ : ndarray of int, sorted
    support_mask_ : ndarray of bool, shape (n_features_in_,)
    merit_ : float
    n_features_in_, feature_names_in_ (DataFrame input), effective_backend_
    """

    def __init__(self, n_bins=10, strategy="uniform", backend="auto", n_jobs=-1, device=0,
                 min_r_cf=0.1):
        self.n_bins = n_bins
        self.strategy = strategy
        self.backend = backend
        self.n_jobs = n_jobs
        self.device = device
        self.min_r_cf = min_r_cf

    def fit(self, X, y):
        """Find the feature subset of the highest merit."""
        if self.backend not in ("auto", "gpu", "cpu"):
            raise ValueError("backend must be 'auto', 'gpu' or 'cpu'.")
        min_r_cf = float(self.min_r_cf)
        if not 0.0 <= min_r_cf <= 1.0:
            raise ValueError("min_r_cf must be in [0, 1].")
        if self.backend == "gpu" and not _lib.gpu_available():
            raise RuntimeError(SURF_GPU_MISSING)
        feature_names = np.asarray(X.columns) if hasattr(X, "columns") else None
        X, y = check_X_y(X, y, dtype=None, ensure_min_samples=2)
        self.n_features_in_ = X.shape[1]
        if feature_names is not None:
            self.feature_names_in_ = feature_names

        # CFS.py:319-337
        p = self.n_features_in_
        is_continuous = np.array([np.issubdtype(X[:, i].dtype, np.floating) for i in range(p)])
        continuous_indices = np.where(is_continuous)[0]
        X_encoded = np.zeros(X.shape, dtype=np.int32)
        n_states_features = np.zeros(p, dtype=np.int32)
        if len(continuous_indices) > 0:
            discretizer = KBinsDiscretizer(n_bins=self.n_bins, encode="ordinal",
                                           strategy=self.strategy, subsample=None)
            X_encoded[:, continuous_indices] = discretizer.fit_transform(
                X[:, continuous_indices]).astype(np.int32)
            n_states_features[continuous_indices] = self.n_bins
        for i in np.where(~is_continuous)[0]:
            unique_vals, encoded_col = np.unique(X[:, i], return_inverse=True)
            X_encoded[:, i] = encoded_col.reshape(-1)
            n_states_features[i] = len(unique_vals)
        unique_y, y_encoded = np.unique(y, return_inverse=True)
        n_states = int(max(int(np.max(n_states_features)), len(unique_y)))

        if self.backend == "gpu" and n_states > _MAX_STATES_GPU:
            raise ValueError("GPU backend supports up to 32 unique states/bins.")
        if self.backend == "gpu" or (self.backend == "auto" and _lib.gpu_available()
                                     and n_states <= _MAX_STATES_GPU):
            effective_backend = "gpu"
        else:
            effective_backend = "cpu"
        if n_states > _MAX_STATES_CPU:
            raise ValueError(f"CPU backend supports up to {_MAX_STATES_CPU} unique states/bins.")
        self.effective_backend_ = effective_backend

        with _lib.Cfs(effective_backend, X_encoded.astype(np.uint8),
                      y_encoded.reshape(-1).astype(np.uint8), n_states, n_jobs=self.n_jobs,
                      device=self.device) as h:
            r_cf_all = h.relevance()
            selected, _ = h.search(min_r_cf)
            # CFS.py:379-399 on the rows the search holds
            rows = {}

            def r_ff_row(i):
                if i not in rows:
                    rows[i] = h.row(i)
                return rows[i]

            selected = np.sort(np.array(selected, dtype=int))
            self.selected_indices_ = np.sort(np.array(
                _prune_redundant(selected, r_cf_all, r_ff_row), dtype=int))
            self.support_mask_ = np.zeros(p, dtype=bool)
            k = len(self.selected_indices_)
            if k == 0:
                self.merit_ = 0.0
            else:
                self.support_mask_[self.selected_indices_] = True
                sub = np.stack([r_ff_row(i)[self.selected_indices_]
                                for i in self.selected_indices_])
                sum_r_cf = np.sum(r_cf_all[self.selected_indices_])
                sum_r_ff = np.sum(np.triu(sub, k=1))
                self.merit_ = _cfs_merit(float(sum_r_cf), k, float(sum_r_ff))
        return self

    def _get_support_mask(self):
        check_is_fitted(self)
        return self.support_mask_

    def transform(self, X):
        """Reduce X to the selected features; a DataFrame stays a DataFrame."""
        check_is_fitted(self)
        if hasattr(X, "iloc"):
            return X.iloc[:, self.support_mask_]
        return np.asarray(X)[:, self.support_mask_]
