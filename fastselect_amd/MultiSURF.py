"""MultiSURF / MultiSURF* estimator (reference: src/fast_select/MultiSURF.py).

Same scikit-learn surface as the reference class (MultiSURF.py:273-489):
constructor parameters, ``fit`` / ``transform`` / ``fit_transform``, fitted
attributes ``n_features_in_``, ``feature_importances_``, ``top_features_``,
``is_discrete_``, ``effective_backend_``.  ``fit`` validates and preprocesses
exactly as the reference (MultiSURF.py:384-420) and then makes ONE call into
the native library (``fs_multisurf_score``), which replaces the reference's
host callers.
"""
from __future__ import annotations

import contextlib

import numpy as np
from sklearn.base import BaseEstimator, TransformerMixin
from sklearn.utils.validation import check_is_fitted, validate_data

from . import _base, _lib


def stir_p_values(t, df, pooled_sd):
    """One-sided p-values P(T_df >= t) of the STIR statistics (scipy's
    Student t survival function).  Where the pooled deviation
    (``_lib.stir_statistics_ex``) is zero, t is +inf, -inf or 0 and p is 0, 1
    or 1 (fs_stir.h): only the last differs from the survival function."""
    from scipy.stats import t as student_t
    t = np.asarray(t, dtype=np.float64)
    p = student_t.sf(t, df)
    p[(np.asarray(pooled_sd) == 0.0) & (t == 0.0)] = 1.0
    return p


def adjust_p_values(p, method="fdr_bh"):
    """Multiple-testing adjustment of a p-value vector: 'fdr_bh' (Benjamini
    and Hochberg's step-up adjusted p-values: p_(i) m / i, made monotone from
    the largest down, capped at 1), 'bonferroni' (p m, capped at 1) or None
    (a copy)."""
    p = np.asarray(p, dtype=np.float64)
    m = p.size
    if method is None:
        return p.copy()
    if method == "bonferroni":
        return np.minimum(p * m, 1.0)
    if method != "fdr_bh":
        raise ValueError(f"adjust must be 'fdr_bh', 'bonferroni' or None; got {method!r}")
    order = np.argsort(p, kind="stable")
    scaled = p[order] * m / np.arange(1, m + 1)
    scaled = np.minimum.accumulate(scaled[::-1])[::-1]
    out = np.empty(m, dtype=np.float64)
    out[order] = np.minimum(scaled, 1.0)
    return out


class MultiSURF(TransformerMixin, BaseEstimator):
    """MI355X-accelerated feature selection with the MultiSURF algorithm.

    Parameters
    ----------
    n_features_to_select : int or float, default=0.2
        Number (int) or fraction (float in (0, 1]) of top features to select.
    backend : {'auto', 'gpu', 'cpu'}, default='auto'
        'gpu' runs the HIP kernels on an AMD Instinct GPU (raises RuntimeError
        when none is visible), 'cpu' the native multithreaded CPU backend,
        'auto' the GPU when one is visible.
    use_star : bool, default=False
        Run MultiSURF* (far misses are subtracted).
    discrete_limit : int, default=10
        Features with at most this many distinct values are discrete.
    n_jobs : int, default=-1
        CPU threads for backend='cpu' (-1 = all).
    verbose : bool, default=False
        Print progress messages.
    devices : None, 'all', int or sequence of int, default=None
        GPU ordinals the GPU backend scores on, one host thread each (the
        pair tiles dealt round-robin; X crosses the host link once, 1/N of
        the rows per device and the rest by peer copies; the exchange
        vectors are summed device-side).  None: device 0, as the reference;
        'all': every visible device the job has work for (one per 4096
        samples).  Not a reference parameter (the reference is
        single-device); ignored by backend='cpu'.
    accumulation : {'fast', 'reference'}, default='fast'
        'reference' replays the reference's float32 arithmetic: each focal
        sample's near-hit / near-miss diffs summed in float32 in sample
        order, then each feature's float32 sequential column sum
        (MultiSURF.py:198-253), on 32-bit pass-1 operands with exact
        thresholds -- the reference's scores bit for bit, at roughly the
        cost of a second pass 2 (DESIGN.md §Reference-order accumulation).
        'fast' (the default) sums each pair once in float32 streams and
        float64 partials: closer to the exact sums than the reference's own
        float32 sums, not equal to them.  Not a reference parameter;
        'reference' runs on one device.

    Significance of the scores (``stir_test``)
    ------------------------------------------
    A Relief score has no scale of its own, so ``feature_importances_`` does
    not say which scores differ from zero.  ``stir_test(X, y)`` scores as
    ``fit`` does and adds STIR ("STatistical Inference Relief", Le,
    Urbanowicz, Moore and McKinney, Bioinformatics 35(8), 2019): it pools
    every (focal sample, near hit) pair and every (focal sample, near miss)
    pair of the fit -- MultiSURF's own neighbourhoods, a pair that is near
    from both sides counted twice -- and compares, per feature, the diffs of
    the two populations with a pooled two-sample t-test, one-sided (misses
    further apart than hits).  The test treats the pairs as independent
    draws, which they are not, because every sample occurs in many pairs:
    this is the published method's approximation, and its p-values are not
    calibrated on noise features (on pure noise expect some very small ones).
    Read them as a scale for the scores, not as exact error rates.

    Attributes set by ``stir_test`` beside those of ``fit``:
    ``stir_t_`` (the t statistic per feature), ``stir_p_values_``
    (P(T_df >= t)), ``stir_p_adjusted_`` (``adjust``: Benjamini-Hochberg,
    Bonferroni or none), ``stir_hit_mean_`` / ``stir_miss_mean_`` (mean diff
    over the near-hit / near-miss pairs), ``stir_df_`` (|H| + |M| - 2),
    ``stir_n_hit_pairs_`` and ``stir_n_miss_pairs_`` (|H|, |M|).  MultiSURF*
    (``use_star=True``) has no STIR statistic.

    Calibrated significance (``permutation_test``)
    ----------------------------------------------
    ``permutation_test(X, y)`` scores as ``fit`` does and compares every
    score with its null distribution under permuted labels.  MultiSURF's
    distances, thresholds and near sets do not read the labels, so they are
    computed once and all labellings are scored in one pass over the near
    pairs (``ShardedMultiSURF.score_labels``).  Attributes set beside those
    of ``fit``: ``p_values_`` (per feature, (1 + #{null >= observed}) /
    (1 + B)), ``p_values_maxT_`` (Westfall-Young single step: against the
    largest null score of each permutation over all features, which controls
    the family-wise error rate), ``null_max_scores_`` (B,), ``null_mean_``
    and ``null_std_`` (p,), ``null_scores_`` (B, p) with ``keep_null=True``,
    ``n_permutations_``.
    """

    def __init__(
        self,
        n_features_to_select: int | float = 0.2,
        backend: str = "auto",
        use_star: bool = False,
        discrete_limit: int = 10,
        n_jobs: int = -1,
        verbose: bool = False,
        devices=None,
        accumulation: str = "fast",
    ):
        self.n_features_to_select = n_features_to_select
        self.backend = backend
        self.use_star = use_star
        self.discrete_limit = discrete_limit
        self.n_jobs = n_jobs
        self.verbose = verbose
        self.devices = devices
        self.accumulation = accumulation

    def _validate_parameters(self, n_samples, n_features):
        _lib.accumulation_code(self.accumulation)
        return _base.resolve_n_select("MultiSURF", self.backend, self.n_features_to_select,
                                      n_samples, n_features)

    def fit(self, x: np.ndarray, y: np.ndarray):
        """Score every feature with MultiSURF (or MultiSURF*)."""
        # float64 X: cast, finiteness scan and upload in one native pass
        sd = _base.stage_device(self.backend, self.devices, _base.rows_hint(x))
        x, y, staged = _base.validate_xy_staged(self, x, y, np.float32, self.n_jobs, sd)
        with _lib.unstaged(staged):
            self.n_features_in_ = x.shape[1]
            n_samples = x.shape[0]
            n_select = self._validate_parameters(n_samples, self.n_features_in_)
            self.effective_backend_ = _base.effective_backend(self.backend)
            self.devices_ = _base.fit_devices(self.devices, self.effective_backend_, n_samples)
            _base.check_accumulation_devices(self.accumulation, self.devices_)
            x = np.ascontiguousarray(x)
            # one upload of X for the whole fit (already done when staged);
            # a multi-device fit uploads X per device
            multi = self.devices_ is not None and len(self.devices_) > 1
            with contextlib.nullcontext() if staged or multi else _lib.staged_x(
                    self.effective_backend_, x, self.devices_[0] if self.devices_ else 0):
                scores = self._score(x, y)
        self.feature_importances_ = scores
        self.top_features_ = _base.top_features(scores, n_select)
        return self

    def _score(self, x, y):
        dev0 = self.devices_[0] if self.devices_ else 0
        is_discrete, col_min, col_max = _base.column_preprocess(x, self.discrete_limit,
                                                                self.effective_backend_, dev0)
        feature_ranges = (col_max - col_min).astype(np.float32)  # _compute_ranges
        feature_ranges[feature_ranges == 0] = 1
        recip_full = (1.0 / feature_ranges).astype(np.float32)
        all_feature_indices = np.arange(self.n_features_in_, dtype=np.int64)
        self.is_discrete_ = is_discrete

        if self.verbose:
            name = "MultiSURF*" if self.use_star else "MultiSURF"
            where = "GPU" if self.effective_backend_ == "gpu" else "CPU"
            print(f"Running {name} on the {where} now...")
        with _lib.accumulation(self.accumulation):
            return _lib.multisurf_score(self.effective_backend_, x, y, recip_full,
                                        all_feature_indices, self.use_star, is_discrete,
                                        self.n_jobs, devices=self.devices_)

    def stir_test(self, x: np.ndarray, y: np.ndarray, adjust="fdr_bh"):
        """Score every feature as ``fit`` does and test each score against
        zero with STIR (see the class docstring): one resident scoring step
        (the plan TuRF re-scores through), then one extra pass over its near
        pairs for the four sums per feature and the float64 epilogue.

        adjust : {'fdr_bh', 'bonferroni', None}
            Multiple-testing adjustment of ``stir_p_values_`` into
            ``stir_p_adjusted_`` (None: a copy).

        Sets the attributes ``fit`` sets (``feature_importances_`` are the
        resident step's scores) and the ``stir_*_`` ones.  The resident job
        (the one TuRF re-scores through) runs on device 0 with the library's
        default host threads: ``devices`` and ``n_jobs`` are not honoured here
        as ``fit`` honours them, and ``devices_`` says so.  MultiSURF* has no
        STIR definition: ValueError.  ValueError too when the fit has fewer
        than 2 near-hit or fewer than 2 near-miss pairs."""
        if adjust not in ("fdr_bh", "bonferroni", None):
            raise ValueError(f"adjust must be 'fdr_bh', 'bonferroni' or None; got {adjust!r}")
        if self.use_star:
            raise ValueError("STIR is defined for MultiSURF's near hits and near misses; "
                             "MultiSURF* (use_star=True) has no STIR statistic")
        scorer = _ResidentMultiSURF(self, x, y)
        try:
            self.devices_ = [0] if self.effective_backend_ == "gpu" else None
            # a new plan scores every column: nothing to re-target
            scorer.active = np.arange(scorer.is_discrete.size, dtype=np.int64)
            scorer.refit(scorer.active)
            sums, n_hit, n_miss = scorer.job.stir()
            sums = sums.cpu().numpy()
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
        """Score every feature as ``fit`` does and give each score a
        permutation p-value: one resident scoring step, then y itself and
        ``n_permutations`` uniform permutations of it (drawn from
        ``np.random.default_rng(random_state)``) scored in one
        ``score_labels`` call on the step's distances, thresholds and near
        sets.  Row 0 of that call is y, so the observed scores and the null
        share one arithmetic.

        Sets the attributes ``fit`` sets (``feature_importances_`` are the
        resident step's scores) and ``p_values_``, ``p_values_maxT_``,
        ``null_max_scores_``, ``null_mean_``, ``null_std_``,
        ``n_permutations_`` and, with ``keep_null=True``, ``null_scores_``
        (see the class docstring).  The resident job runs on device 0 with the
        library's default host threads: ``devices`` and ``n_jobs`` are not
        honoured here as ``fit`` honours them, and ``devices_`` says so.
        ValueError for ``use_star=True`` (the star's far misses read the
        labels), for ``accumulation='reference'`` and for
        ``n_permutations < 1``."""
        if self.use_star:
            raise ValueError("the permutation test scores MultiSURF's near pairs on "
                             "label-independent decisions; MultiSURF* (use_star=True) is not "
                             "built")
        _lib.accumulation_code(self.accumulation)
        if self.accumulation != "fast":
            raise ValueError("the permutation test runs in accumulation='fast' (the null is not "
                             "accumulated in reference order)")
        n_permutations = int(n_permutations)
        if n_permutations < 1:
            raise ValueError(f"n_permutations must be >= 1; got {n_permutations}")
        scorer = _ResidentMultiSURF(self, x, y)
        try:
            self.devices_ = [0] if self.effective_backend_ == "gpu" else None
            scorer.active = np.arange(scorer.is_discrete.size, dtype=np.int64)
            scorer.refit(scorer.active)
            y_enc = np.unique(scorer.y, return_inverse=True)[1].astype(np.int32).reshape(-1)
            rng = np.random.default_rng(random_state)
            labels = np.empty((n_permutations + 1, y_enc.size), dtype=np.int32)
            labels[0] = y_enc
            for b in range(n_permutations):
                labels[b + 1] = rng.permutation(y_enc)
            scores = scorer.job.score_labels(labels).cpu().numpy().astype(np.float64)
        finally:
            scorer.close()
        return _base.set_permutation_attributes(self, scores, n_permutations, keep_null)

    def _resident_scorer(self, x, y):
        """A scorer for TuRF that keeps X resident (on the GPU for the GPU
        backend) and re-scores column subsets through feat_idx, which the
        reference's kernels support for exactly this (MultiSURF.py:147,256):
        ``refit(active)`` leaves this estimator as ``fit(X[:, active], y)``
        would, without copying or re-uploading X."""
        return _ResidentMultiSURF(self, x, y)

    def transform(self, x: np.ndarray) -> np.ndarray:
        """Reduce x to the selected features."""
        check_is_fitted(self)
        x = validate_data(self, x, reset=False, dtype=[np.float64, np.float32])
        return x[:, self.top_features_]

    def fit_transform(self, x: np.ndarray, y: np.ndarray) -> np.ndarray:
        """Fit to data, then transform it."""
        self.fit(x, y)
        return self.transform(x)


class _ResidentMultiSURF:
    """See ``MultiSURF._resident_scorer``."""

    def __init__(self, est: MultiSURF, x, y):
        self.est = est
        _lib.accumulation_code(est.accumulation)
        x, y = _base.validate_xy(est, x, y, np.float32, est.n_jobs,
                                 pinned=_base.stage_device(est.backend) is not None)
        est.effective_backend_ = _base.effective_backend(est.backend)
        self.n = x.shape[0]
        self.y = np.asarray(y)
        self.is_discrete, col_min, col_max = _base.column_preprocess(
            x, est.discrete_limit, est.effective_backend_)
        ranges = (col_max - col_min).astype(np.float32)
        ranges[ranges == 0] = 1
        recip = (1.0 / ranges).astype(np.float32)
        from .parallel import ShardedMultiSURF
        self.job = ShardedMultiSURF(x, y, recip, self.is_discrete, use_star=est.use_star,
                                    backend=est.effective_backend_, shard=False,
                                    accumulation=est.accumulation)
        self.active = None

    def refit(self, active: np.ndarray):
        est = self.est
        active = np.asarray(active, dtype=np.int64)
        n_select = est._validate_parameters(self.n, active.size)
        est.n_features_in_ = active.size
        if est.verbose:
            name = "MultiSURF*" if est.use_star else "MultiSURF"
            where = "GPU" if est.effective_backend_ == "gpu" else "CPU"
            print(f"Running {name} on the {where} now...")
        if self.active is None or not np.array_equal(active, self.active):
            self.job.set_features(active)
            self.active = active
        scores = self.job.step().cpu().numpy()
        est.is_discrete_ = self.is_discrete[active]
        est.feature_importances_ = scores
        est.top_features_ = _base.top_features(scores, n_select)
        return est

    def close(self):
        self.job.close()
