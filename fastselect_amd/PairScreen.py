"""PairScreen: an exhaustive screen of all feature pairs on discrete data.

Every other filter here ranks a feature by what it says about y on its own
(``mRMR``, ``CFS``) or grows greedily from the most relevant feature (``JMI``:
it only ever looks at pairs that contain a feature it has picked).  A pair that
acts purely together, ``y = x_a XOR x_b`` with no main effect, is what ``MDR``
exists for, and none of them finds it.  This estimator scans the joint relevance
``J(i, j) = I(X_i, X_j; y)`` of all C(p,2) pairs and keeps the ``n_top`` best:

* ``score="joint"``: ``J(i, j)`` itself;
* ``score="gain"``: the interaction information
  ``(J(i, j) - I(X_i; y)) - I(X_j; y)``, positive for a pair that says more
  together than apart, negative for a redundant one.

A feature is scored by the best pair it belongs to, and the
``n_features_to_select`` best features are kept, so the estimator can stand in
front of ``MDR`` in a ``Pipeline``.  The definitions are in
``csrc/fs_pairscan.h``; there is no reference implementation in ``fast_select``.

``fit`` encodes every column and y by their own sorted unique values, as
``JMI.fit`` does, and makes one call to ``fs_pair_screen``: one tiled scan on
the GPU, a ranked list back, nothing of size p x p anywhere.
"""
from __future__ import annotations

import numpy as np
from sklearn.base import BaseEstimator, TransformerMixin
from sklearn.utils.validation import check_is_fitted, validate_data

from . import _lib
from . import mutual_information as mi


class PairScreen(TransformerMixin, BaseEstimator):
    """All-pairs interaction screen for discrete data on the MI355X or the CPU.

    Parameters
    ----------
    n_features_to_select : int
        Number of features to keep.
    n_top : int, default=100
        Length of the ranked list of pairs (1..65536).
    score : {'gain', 'joint'}, default='gain'
        Interaction information, or the joint relevance itself.
    backend : {'auto', 'cpu', 'gpu'}, default='auto'
        'gpu' without a visible HIP device, with more than 32 states in a
        column or more than 4 classes of y raises; it never falls back.
        'auto' uses the GPU when one is visible and the data is within both
        limits, else the CPU.
    unit : {'bit', 'nat'}, default='bit'
    n_jobs : int, default=-1
        CPU threads for the CPU backend (-1 = all).
    device : int, default=0
        GPU ordinal for the GPU backend.

    Attributes
    ----------
    top_pairs_ : ndarray of int64, shape (min(n_top, C(p,2)), 2)
        The best pairs (i < j), by score descending and, among equal scores,
        in the order of ``itertools.combinations``.
    top_scores_ : ndarray of float64
        Their scores.
    relevance_scores_ : ndarray of float64, shape (n_features,)
        ``I(X_f; y)``, the values ``mRMR`` and ``JMI`` compute.
    interaction_scores_ : ndarray of float64, shape (n_features,)
        The largest score of any pair that contains the feature.
    feature_importances_ : ndarray (the interaction scores)
    top_features_ : ndarray of int32, shape (n_features_to_select,)
        The first of ``np.argsort(-interaction_scores_, kind="stable")``.
    n_features_in_, effective_backend_
    null_max_scores_, null_best_pairs_, n_permutations_, p_value_, top_p_values_
        After ``permutation_test`` only: see there.
    """

    def __init__(self, n_features_to_select: int, n_top: int = 100, score: str = "gain",
                 backend: str = "auto", unit: str = "bit", n_jobs: int = -1, device: int = 0):
        self.n_features_to_select = n_features_to_select
        self.n_top = n_top
        self.score = score
        self.backend = backend
        self.unit = unit
        self.n_jobs = n_jobs
        self.device = device

    def fit(self, X, y):
        """Screen all pairs of the discrete X and keep the best features."""
        self._fit_codes(X, y)
        return self

    def _fit_codes(self, X, y):
        """``fit``; returns what it made of X and y: (codes, ycodes, n_states)."""
        if self.score not in _lib.PAIR_SCORES:
            raise ValueError("score must be either 'gain' or 'joint'.")
        if self.backend not in ("auto", "cpu", "gpu"):
            raise ValueError("backend must be 'auto', 'cpu' or 'gpu'")
        if self.unit not in _lib.MI_UNITS:
            raise ValueError("unit must be 'bit' or 'nat'")
        if not (1 <= self.n_top <= _lib.PAIR_MAX_TOP):
            raise ValueError(f"n_top must be in 1..{_lib.PAIR_MAX_TOP}")
        X, y = validate_data(self, X, y, dtype=None, ensure_2d=True)
        n, p = X.shape
        self.n_features_in_ = p
        if not (0 < self.n_features_to_select <= p):
            raise ValueError(
                "n_features_to_select must be a positive integer less "
                "than or equal to the number of features."
            )
        if p < 2:
            raise ValueError("PairScreen needs at least two features.")
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
        relevance, top_scores, top_pairs, best = _lib.pair_screen(
            where, codes, ycodes, n_states, n_top=self.n_top, score=self.score, unit=self.unit,
            n_jobs=self.n_jobs, device=self.device)
        self.relevance_scores_ = relevance
        self.top_scores_ = top_scores
        self.top_pairs_ = top_pairs
        self.interaction_scores_ = best
        self.feature_importances_ = self.interaction_scores_
        order = np.argsort(-self.interaction_scores_, kind="stable")
        self.top_features_ = order[:self.n_features_to_select].astype(np.int32)
        return codes, ycodes, n_states

    def permutation_test(self, X, y, n_permutations=1000, random_state=None):
        """``fit``, then the max-T (Westfall-Young single-step) permutation test
        of the ranked list: an exhaustive screen finds a best pair in pure
        noise too, and this says how large the best score of a screen gets
        when y has nothing to do with X.

        The screen of y and of ``n_permutations`` shuffles of y
        (``np.random.default_rng(random_state).permutation``, in order) is one
        pass over the pairs (``fs_pair_screen_labels``); the null statistic of
        a shuffle is the best score of its whole screen.  Every attribute of
        ``fit`` is set as ``fit`` sets it, and

        * ``null_max_scores_`` (n_permutations,), ``null_best_pairs_``
          (n_permutations, 2), ``n_permutations_``;
        * ``p_value_``: ``(1 + #{null_max >= top_scores_[0]}) / (1 + n_permutations)``;
        * ``top_p_values_``: the same for every listed pair, the max-T adjusted
          p-value of each; non-decreasing down the list.
        """
        if not (isinstance(n_permutations, (int, np.integer)) and
                1 <= n_permutations < _lib.PAIR_MAX_LABELINGS):
            raise ValueError(f"n_permutations must be in 1..{_lib.PAIR_MAX_LABELINGS - 1}")
        n_perm = int(n_permutations)
        codes, ycodes, n_states = self._fit_codes(X, y)
        rng = np.random.default_rng(random_state)
        labels = np.empty((n_perm + 1, ycodes.size), dtype=np.uint8)
        labels[0] = ycodes
        for b in range(1, n_perm + 1):
            labels[b] = rng.permutation(ycodes)
        best, pairs, _ = _lib.pair_screen_labels(
            self.effective_backend_, codes, labels, n_states, score=self.score, unit=self.unit,
            n_jobs=self.n_jobs, device=self.device)
        # row 0 is the data's own y: the batch and the single call agree bit for bit
        if best[0] != self.top_scores_[0] or tuple(pairs[0]) != tuple(self.top_pairs_[0]):
            raise AssertionError(
                "fs_pair_screen_labels disagrees with fs_pair_screen on the unpermuted y")
        self.null_max_scores_ = best[1:].copy()
        self.null_best_pairs_ = pairs[1:].copy()
        self.n_permutations_ = n_perm
        null_sorted = np.sort(self.null_max_scores_)
        at_least = n_perm - np.searchsorted(null_sorted, self.top_scores_, side="left")
        self.top_p_values_ = (1.0 + at_least) / (1.0 + n_perm)
        self.p_value_ = float(self.top_p_values_[0])
        return self

    def transform(self, X):
        """Reduce X to the selected features."""
        check_is_fitted(self)
        X = validate_data(self, X, reset=False, dtype=None)
        return X[:, self.top_features_]
