"""RReliefF estimator: Relief for a continuous target (Robnik-Sikonja and
Kononenko, 1997; Machine Learning 53, 2003).  The reference project has no
implementation; ``csrc/fs_rrelieff.h`` is the specification.

``fit`` validates and preprocesses X exactly as ``ReliefF.fit`` does
(validation, discrete detection, reciprocal ranges) and then scores on a
ReliefF plan with ONE class: the neighbours of a sample are its k nearest
other samples and do not read y, so ``fs_plan_score_targets`` runs the
distance pass and the selection once for any number of targets -- which is
what makes ``permutation_test`` nearly free.
"""
from __future__ import annotations

import numpy as np
from sklearn.base import BaseEstimator, TransformerMixin
from sklearn.utils.validation import check_is_fitted, validate_data

from . import _base, _lib


def rrelieff_inputs(x, discrete_limit, where, device=0, n_jobs=-1):
    """ReliefF.fit's preprocessing of X (``relieff_inputs`` without the class
    part): (x32, recip f32, is_discrete)."""
    is_discrete, col_min, col_max = _base.column_preprocess(x, discrete_limit, where, device)
    feature_ranges = col_max - col_min
    feature_ranges[is_discrete] = 1.0
    feature_ranges[feature_ranges == 0] = 1.0
    recip = (1.0 / feature_ranges).astype(np.float32)
    return _base.to_float32(x, n_jobs, pinned=where == "gpu"), recip, is_discrete


class RReliefF(TransformerMixin, BaseEstimator):
    """MI355X-accelerated feature scoring for a continuous target (RReliefF).

    For each sample i and each of its ``n_neighbors`` nearest other samples j
    (the float32 distance keys and tie order of ``ReliefF`` with one class),
    with d_f the per-feature diff and dy = |y_i - y_j| / (max y - min y)::

        W[f] = S_CA[f] / S_C - (S_A[f] - S_CA[f]) / (M - S_C)

    where S_A = sum d_f, S_CA = sum dy d_f, S_C = sum dy over the M = n k
    pairs, in float64.  Every neighbour has the same weight; the paper's
    rank-weighted neighbours are not built.

    Parameters
    ----------
    n_features_to_select : int or float, default=0.2
        Number (int) or fraction (float in (0, 1]) of top features to select.
    discrete_limit : int, default=10
        Features with at most this many distinct values are discrete.
    n_neighbors : int, default=10
        Nearest samples used per sample; 0 < n_neighbors < n_samples.
    backend : {'auto', 'gpu', 'cpu'}, default='auto'
        Compute backend (see ``MultiSURF``).  The GPU backend runs on device 0.
    verbose : bool, default=False
        Print progress messages.
    n_jobs : int, default=-1
        CPU threads for backend='cpu' (-1 = all).
    """

    def __init__(
        self,
        n_features_to_select: int | float = 0.2,
        discrete_limit: int = 10,
        n_neighbors: int = 10,
        backend: str = "auto",
        verbose: bool = False,
        n_jobs: int = -1,
    ):
        self.n_features_to_select = n_features_to_select
        self.discrete_limit = discrete_limit
        self.n_neighbors = n_neighbors
        self.backend = backend
        self.verbose = verbose
        self.n_jobs = n_jobs

    def _validate_parameters(self, n_samples, n_features):
        if self.backend not in ["auto", "gpu", "cpu"]:
            raise ValueError("backend must be one of 'auto', 'gpu', or 'cpu'")
        if n_samples < 2:
            raise ValueError(
                f"RReliefF requires at least 2 samples, but got n_samples = {n_samples}")
        if not (0 < self.n_neighbors < n_samples):
            raise ValueError(
                f"n_neighbors ({self.n_neighbors}) must be an integer "
                f"between 1 and n_samples - 1 ({n_samples - 1}).")
        return _base.n_select_from(self.n_features_to_select, n_features)

    def _scorer(self, x, y):
        """(ResidentTargets or None for a constant y, validated x's shape)."""
        from ._resident import ResidentTargets
        x, y = _base.validate_xy(self, x, y, np.float64, self.n_jobs)
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        if not np.all(np.isfinite(y)):
            raise ValueError("Input y contains NaN or infinity.")
        n, p = x.shape
        self.n_features_in_ = p
        self._validate_parameters(n, p)
        if y.max() == y.min():
            self.effective_backend_ = "cpu" if self.backend != "gpu" else "gpu"
            return None, (n, p)
        where = "gpu" if self.backend != "cpu" and _lib.gpu_available() else "cpu"
        x32, recip, is_discrete = rrelieff_inputs(x, self.discrete_limit, where,
                                                  n_jobs=self.n_jobs)
        self.effective_backend_ = _base.effective_backend(self.backend)
        with _lib.accumulation("fast"):  # the plan keeps its creation mode
            plan = _lib.RowsPlan(self.effective_backend_, "relieff", x32,
                                 np.zeros(n, dtype=np.int32), recip, is_discrete,
                                 k=self.n_neighbors, class_probs=np.ones(1, dtype=np.float32),
                                 n_jobs=self.n_jobs)
        return ResidentTargets(self, plan, n, self.n_neighbors, y, is_discrete,
                               self.effective_backend_), (n, p)

    def _constant(self, p):
        n_select = _base.n_select_from(self.n_features_to_select, p)
        self.feature_importances_ = np.zeros(p, dtype=np.float32)
        self.top_features_ = np.arange(n_select)
        return self

    def fit(self, x: np.ndarray, y: np.ndarray):
        """Score every feature with RReliefF.  A constant y gives zero scores
        (as ReliefF's single-class shortcut)."""
        scorer, (_, p) = self._scorer(x, y)
        if scorer is None:
            return self._constant(p)
        try:
            # a new plan scores every column: nothing to re-target
            scorer.active = np.arange(p, dtype=np.int64)
            scorer.refit(scorer.active)
        finally:
            scorer.close()
        return self

    def _resident_scorer(self, x, y):
        """A scorer for TuRF that keeps X resident and re-scores column
        subsets (``ResidentTargets``); None for a constant y (TuRF then
        refits, which yields zeros)."""
        return self._scorer(x, y)[0]

    def permutation_test(self, x: np.ndarray, y: np.ndarray, n_permutations=1000,
                         random_state=None, keep_null=False):
        """Score every feature and give each score a permutation p-value: y
        itself (row 0) and ``n_permutations`` uniform permutations of it
        (``np.random.default_rng(random_state).permutation(y)``) are scored in
        one ``score_targets`` call.  The neighbours do not read y, so the
        distance pass and the selection run once for the whole test and a
        permutation costs one more weight per (sample, neighbour) pair.

        Sets the attributes ``fit`` sets and, with ``obs`` the scores of row 0
        and ``null`` those of the permutations, ``p_values_``
        ((1 + #{null_f >= obs_f}) / (1 + n_permutations)), ``p_values_maxT_``
        (Westfall-Young: the same against each permutation's largest score),
        ``null_max_scores_``, ``null_mean_``, ``null_std_``,
        ``n_permutations_`` and, with ``keep_null=True``, ``null_scores_`` --
        defined exactly as ``ReliefF.permutation_test`` defines them.
        ValueError for a constant y and for ``n_permutations < 1``."""
        n_permutations = int(n_permutations)
        if n_permutations < 1:
            raise ValueError(f"n_permutations must be >= 1; got {n_permutations}")
        scorer, (n, p) = self._scorer(x, y)
        if scorer is None:
            raise ValueError("a permutation of y is y itself: y is constant")
        try:
            n_select = _base.n_select_from(self.n_features_to_select, p)
            rng = np.random.default_rng(random_state)
            targets = np.empty((n_permutations + 1, n), dtype=np.float64)
            targets[0] = scorer.y
            for b in range(n_permutations):
                targets[b + 1] = rng.permutation(scorer.y)
            if self.verbose:
                print(f"Running RReliefF on the {self.effective_backend_.upper()} now...")
            scores32 = scorer.score_targets(targets)
        finally:
            scorer.close()
        self.is_discrete_ = scorer.is_discrete
        self.feature_importances_ = scores32[0].copy()
        self.top_features_ = _base.top_features(self.feature_importances_, n_select)
        scores = scores32.astype(np.float64)
        obs, null = scores[0], scores[1:]
        null_max = null.max(axis=1)
        self.n_permutations_ = n_permutations
        self.p_values_ = (1.0 + (null >= obs[None, :]).sum(axis=0)) / (1.0 + n_permutations)
        self.p_values_maxT_ = ((1.0 + (null_max[:, None] >= obs[None, :]).sum(axis=0))
                               / (1.0 + n_permutations))
        self.null_max_scores_ = null_max
        self.null_mean_ = null.mean(axis=0)
        self.null_std_ = null.std(axis=0)
        if keep_null:
            self.null_scores_ = null
        elif hasattr(self, "null_scores_"):
            del self.null_scores_
        return self

    def transform(self, x: np.ndarray) -> np.ndarray:
        """Reduce x to the selected features."""
        check_is_fitted(self)
        x = validate_data(self, x, reset=False, dtype=[np.float64, np.float32])
        return x[:, self.top_features_]

    def fit_transform(self, x: np.ndarray, y: np.ndarray) -> np.ndarray:
        """Fit to data, then transform it."""
        self.fit(x, y)
        return self.transform(x)
