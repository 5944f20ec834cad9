"""ReliefF estimator (reference: src/fast_select/ReliefF.py:239-453).

``fit`` validates and preprocesses exactly as the reference
(ReliefF.py:343-380: float64 validation, single-class shortcut, neighbour
warning, discrete detection, class priors, ranges) and then makes one call to
``fs_relieff_score``, which replaces ``_relieff_{cpu,gpu}_host_caller``.
"""
from __future__ import annotations

import warnings

import numpy as np
from sklearn.base import BaseEstimator, TransformerMixin
from sklearn.utils.validation import check_is_fitted, validate_data

from . import _base, _lib


def relieff_inputs(x, y, discrete_limit, where, device=0, n_jobs=-1):
    """ReliefF.fit's preprocessing after validation (ReliefF.py:366-380, 400):
    discrete detection and column ranges (computed on ``where``), class priors,
    class codes, reciprocal ranges (discrete and constant columns -> 1) and the
    float32 cast.  Returns (x32, y_enc int32, recip f32, is_discrete, priors f32)."""
    is_discrete, col_min, col_max = _base.column_preprocess(x, discrete_limit, where, device)
    class_labels, class_counts = np.unique(y, return_counts=True)
    class_probs = class_counts / len(y)
    y_enc = np.searchsorted(class_labels, y)
    feature_ranges = col_max - col_min
    feature_ranges[is_discrete] = 1.0
    feature_ranges[feature_ranges == 0] = 1.0
    recip = (1.0 / feature_ranges).astype(np.float32)
    return (_base.to_float32(x, n_jobs, pinned=where == "gpu"), y_enc.astype(np.int32), recip, is_discrete,
            class_probs.astype(np.float32))


class ReliefF(TransformerMixin, BaseEstimator):
    """MI355X-accelerated feature selection with the ReliefF algorithm.

    Parameters
    ----------
    n_features_to_select : int or float, default=0.2
        Number (int) or fraction (float in (0, 1]) of top features to select.
    discrete_limit : int, default=10
        Features with at most this many distinct values are discrete.
    n_neighbors : int, default=3
        Nearest hits, and nearest misses per other class, used per sample.
    backend : {'auto', 'gpu', 'cpu'}, default='auto'
        Compute backend (see ``MultiSURF``).
    verbose : bool, default=False
        Print progress messages.
    n_jobs : int, default=-1
        CPU threads for backend='cpu' (-1 = all).
    devices : None, 'all', int or sequence of int, default=None
        GPU ordinals the GPU backend scores on, one host thread each (whole
        128-sample blocks of the focal samples per thread, X moved over the
        host link once and shared by peer copies, the score sums added on
        the host).  None: device 0, as the reference; 'all': every visible
        device the job has work for (one per 4096 samples).  Not a reference
        parameter; ignored by backend='cpu'.
    accumulation : {'fast', 'reference'}, default='fast'
        'reference': each sample's neighbours in the reference's argsort
        order, its float64 update rounded to a float32 row, and each
        feature's float32 sequential column sum (ReliefF.py:181-220) -- the
        reference's scores bit for bit.  'fast': the update summed in
        float64 throughout.  Not a reference parameter; 'reference' runs on
        one device.
    """

    def __init__(
        self,
        n_features_to_select: int | float = 0.2,
        discrete_limit: int = 10,
        n_neighbors: int = 3,
        backend: str = "auto",
        verbose: bool = False,
        n_jobs: int = -1,
        devices=None,
        accumulation: str = "fast",
    ):
        self.n_features_to_select = n_features_to_select
        self.discrete_limit = discrete_limit
        self.n_neighbors = n_neighbors
        self.backend = backend
        self.verbose = verbose
        self.n_jobs = n_jobs
        self.devices = devices
        self.accumulation = accumulation

    def _validate_parameters(self, n_samples, n_features):
        _lib.accumulation_code(self.accumulation)
        if self.backend not in ["auto", "gpu", "cpu"]:
            raise ValueError("backend must be one of 'auto', 'gpu', or 'cpu'")
        if n_samples < 2:
            raise ValueError(
                f"ReliefF requires at least 2 samples, but got n_samples = {n_samples}")
        if not (0 < self.n_neighbors < n_samples):
            raise ValueError(
                f"n_neighbors ({self.n_neighbors}) must be an integer "
                f"between 1 and n_samples - 1 ({n_samples - 1}).")
        return _base.n_select_from(self.n_features_to_select, n_features)

    def fit(self, x: np.ndarray, y: np.ndarray):
        """Score every feature with ReliefF."""
        x, y = _base.validate_xy(self, x, y, np.float64, self.n_jobs)
        self.n_features_in_ = x.shape[1]
        n_samples = x.shape[0]
        n_select = self._validate_parameters(n_samples, self.n_features_in_)

        self.classes_, y_encoded = np.unique(y, return_inverse=True)
        if len(self.classes_) < 2:
            self.feature_importances_ = np.zeros(self.n_features_in_, dtype=np.float32)
            self.top_features_ = np.arange(n_select)
            self.effective_backend_ = "cpu" if self.backend != "gpu" else "gpu"
            return self

        min_class_size = np.min(np.bincount(y_encoded))
        if self.n_neighbors >= min_class_size:
            warnings.warn(
                f"n_neighbors ({self.n_neighbors}) is greater than or equal to the "
                f"smallest class size ({min_class_size}).",
                UserWarning,
            )

        # preprocessing runs where the scoring will (the backend itself is
        # resolved below, after these steps, as in the reference)
        where = "gpu" if self.backend != "cpu" and _lib.gpu_available() else "cpu"
        sd = _base.stage_device(self.backend, self.devices, n_samples)
        x32, y_enc, recip_full, is_discrete, class_probs = relieff_inputs(
            x, y, self.discrete_limit, where, 0 if sd is None else sd, n_jobs=self.n_jobs)
        self.is_discrete_ = is_discrete

        self.effective_backend_ = _base.effective_backend(self.backend)
        self.devices_ = _base.fit_devices(self.devices, self.effective_backend_, n_samples)
        _base.check_accumulation_devices(self.accumulation, self.devices_)
        if self.verbose:
            where = "GPU" if self.effective_backend_ == "gpu" else "CPU"
            print(f"Running ReliefF on the {where} now...")
        with _lib.accumulation(self.accumulation):
            scores = _lib.relieff_score(self.effective_backend_, x32, y_enc, recip_full,
                                        is_discrete, self.n_neighbors, class_probs, self.n_jobs,
                                        devices=self.devices_)
        self.feature_importances_ = scores
        self.top_features_ = _base.top_features(scores, n_select)
        return self

    def _resident_scorer(self, x, y):
        """A scorer for TuRF that keeps X resident and re-scores column
        subsets (``ResidentRows``); None when there is nothing to score
        (a single class: TuRF then refits, which yields zeros)."""
        from ._resident import ResidentRows
        x, y = _base.validate_xy(self, x, y, np.float64, self.n_jobs)
        n = x.shape[0]
        self._validate_parameters(n, x.shape[1])
        classes, y_encoded = np.unique(y, return_inverse=True)
        if len(classes) < 2:
            return None
        self.classes_ = classes
        min_class_size = np.min(np.bincount(y_encoded))

        def warn_small_class():
            if self.n_neighbors >= min_class_size:
                warnings.warn(
                    f"n_neighbors ({self.n_neighbors}) is greater than or equal to the "
                    f"smallest class size ({min_class_size}).",
                    UserWarning,
                )

        where = "gpu" if self.backend != "cpu" and _lib.gpu_available() else "cpu"
        x32, y_enc, recip, is_discrete, class_probs = relieff_inputs(
            x, y, self.discrete_limit, where, n_jobs=self.n_jobs)
        self.effective_backend_ = _base.effective_backend(self.backend)
        with _lib.accumulation(self.accumulation):  # the plan keeps its creation mode
            plan = _lib.RowsPlan(self.effective_backend_, "relieff", x32, y_enc, recip,
                                 is_discrete, k=self.n_neighbors, class_probs=class_probs,
                                 n_jobs=self.n_jobs)
        return ResidentRows(self, "ReliefF", plan, n, is_discrete, self.effective_backend_,
                            before_score=warn_small_class)

    def stir_test(self, x: np.ndarray, y: np.ndarray, adjust="fdr_bh"):
        """Score every feature on the resident plan (the one TuRF re-scores
        through) and test each score against zero with STIR (Le et al.,
        Bioinformatics 2019): per feature a pooled two-sample t-test of the
        diffs over the nearest-miss pairs against those over the nearest-hit
        pairs, the pairs being (sample, neighbour) over the very
        ``n_neighbors`` lists the score weighs.  The misses of all other
        classes are pooled, unweighted (for two classes the published test;
        for more this project's generalisation), and the reference's self-hit
        of a class with fewer than ``n_neighbors`` other members is not a
        pair.  The test treats the pairs as independent, which they are not:
        the p-values are the method's approximation, not calibrated on noise
        features.

        adjust : {'fdr_bh', 'bonferroni', None}
            Multiple-testing adjustment of ``stir_p_values_`` into
            ``stir_p_adjusted_`` (None: a copy).

        Sets the attributes the resident scorer's ``refit`` sets
        (``feature_importances_``, ``top_features_``, ...) and ``stir_t_``,
        ``stir_p_values_`` (P(T_df >= t)), ``stir_p_adjusted_``,
        ``stir_hit_mean_`` / ``stir_miss_mean_``, ``stir_df_``
        (|H| + |M| - 2), ``stir_n_hit_pairs_`` and ``stir_n_miss_pairs_``.
        The resident plan runs on device 0 (``devices_`` says so); ValueError
        when ``devices`` names more than one device.  ValueError
        for a single class, and when there are fewer than 2 hit or fewer
        than 2 miss pairs."""
        from .MultiSURF import adjust_p_values, stir_p_values
        if adjust not in ("fdr_bh", "bonferroni", None):
            raise ValueError(f"adjust must be 'fdr_bh', 'bonferroni' or None; got {adjust!r}")
        devs = _base.fit_devices(self.devices, _base.effective_backend(self.backend),
                                 _base.rows_hint(x) or 0)
        if devs is not None and len(devs) > 1:
            raise ValueError(f"ReliefF.stir_test runs on one device; got devices={list(devs)!r}")
        scorer = self._resident_scorer(x, y)
        if scorer is None:
            raise ValueError("STIR compares hit pairs with miss pairs: y has a single class, "
                             "so there are no misses")
        try:
            self.devices_ = [0] if self.effective_backend_ == "gpu" else None
            # a new plan scores every column: nothing to re-target
            scorer.active = np.arange(scorer.is_discrete.size, dtype=np.int64)
            scorer.refit(scorer.active, stir=True)
            sums, n_hit, n_miss = scorer.stir_
        finally:
            scorer.close()
        hit_mean, miss_mean, t, df, sp = _lib.stir_statistics_ex(sums, n_hit, n_miss)
        self.stir_t_ = t
        self.stir_df_ = df
        self.stir_hit_mean_ = hit_mean
        self.stir_miss_mean_ = miss_mean
        self.stir_n_hit_pairs_ = int(n_hit)
        self.stir_n_miss_pairs_ = int(n_miss)
        self.stir_p_values_ = stir_p_values(t, df, sp)
        self.stir_p_adjusted_ = adjust_p_values(self.stir_p_values_, adjust)
        return self

    def permutation_test(self, x: np.ndarray, y: np.ndarray, n_permutations=1000,
                         random_state=None, keep_null=False):
        """Score every feature on the resident plan (as ``stir_test`` does)
        and give each score a permutation p-value: y itself and
        ``n_permutations`` uniform permutations of it (drawn from
        ``np.random.default_rng(random_state)``) are scored in one
        ``score_labels`` call, which runs the distance pass once and then
        selects neighbours and updates per labelling.  Row 0 of that call is
        y, so the observed scores and the null share one arithmetic; a
        permutation keeps the class sizes, so every labelling has y's priors.

        Sets the attributes the resident scorer's ``refit`` sets
        (``feature_importances_``, ``top_features_``, ...) and, with ``obs``
        the scores of row 0 and ``null`` those of the permutations,
        ``p_values_`` ((1 + #{null_f >= obs_f}) / (1 + n_permutations)),
        ``p_values_maxT_`` (Westfall-Young: the same against each
        permutation's largest score), ``null_max_scores_``, ``null_mean_``,
        ``null_std_``, ``n_permutations_`` and, with ``keep_null=True``,
        ``null_scores_`` -- defined exactly as ``MultiSURF.permutation_test``
        defines them.  The resident plan runs on device 0 (``devices_`` says
        so).  ValueError for a single class, for ``accumulation='reference'``,
        for ``n_permutations < 1`` and when ``devices`` names more than one
        device; the small-class UserWarning as ``fit``."""
        _lib.accumulation_code(self.accumulation)
        if self.accumulation != "fast":
            raise ValueError("the permutation test runs in accumulation='fast' (the null is not "
                             "accumulated in reference order)")
        n_permutations = int(n_permutations)
        if n_permutations < 1:
            raise ValueError(f"n_permutations must be >= 1; got {n_permutations}")
        devs = _base.fit_devices(self.devices, _base.effective_backend(self.backend),
                                 _base.rows_hint(x) or 0)
        if devs is not None and len(devs) > 1:
            raise ValueError("ReliefF.permutation_test runs on one device; got "
                             f"devices={list(devs)!r}")
        y_enc = np.unique(np.asarray(y).reshape(-1), return_inverse=True)[1]
        y_enc = y_enc.astype(np.int32).reshape(-1)
        if y_enc.size and int(y_enc.max()) >= 64:
            raise ValueError("ReliefF.permutation_test scores at most 64 classes")
        # validates X and y as fit does; its refit below emits fit's small-class
        # UserWarning (before_score)
        scorer = self._resident_scorer(x, y)
        if scorer is None:
            raise ValueError("a permutation of y is y itself: y has a single class")
        try:
            self.devices_ = [0] if self.effective_backend_ == "gpu" else None
            # a new plan scores every column: nothing to re-target
            scorer.active = np.arange(scorer.is_discrete.size, dtype=np.int64)
            scorer.refit(scorer.active)
            rng = np.random.default_rng(random_state)
            labels = np.empty((n_permutations + 1, y_enc.size), dtype=np.int32)
            labels[0] = y_enc
            for b in range(n_permutations):
                labels[b + 1] = rng.permutation(y_enc)
            sums = scorer.score_labels(labels)
        finally:
            scorer.close()
        scores = (sums / scorer.n).astype(np.float32).astype(np.float64)
        return _base.set_permutation_attributes(self, scores, n_permutations, keep_null)

    def transform(self, x: np.ndarray) -> np.ndarray:
        """Reduce x to the selected features."""
        check_is_fitted(self)
        x = validate_data(self, x, reset=False, dtype=[np.float64, np.float32])
        return x[:, self.top_features_]

    def fit_transform(self, x: np.ndarray, y: np.ndarray) -> np.ndarray:
        """Fit to data, then transform it."""
        self.fit(x, y)
        return self.transform(x)
