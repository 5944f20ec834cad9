"""MDR estimator (reference: src/fast_select/MDR.py:148-357).

Multifactor dimensionality reduction: score every k-column combination of a
0/1/2 genotype matrix by the balanced accuracy of its high/low-risk table,
pick each cross-validation fold's best model, and keep the model with the
highest cross-validation consistency.

``fit`` validates as the reference (MDR.py:220-244), draws the reference's
folds on the host, and makes one call to ``fs_mdr_scan``, which replaces the
per-fold ``mdr_kernel`` / ``_batch_balanced_accuracy_cpu`` launches and the
host-built combination list (MDR.py:246-283): all folds come out of one pass
over bit-plane genotypes, and combinations are addressed by rank.  The per-fold
lookup tables, test accuracies and the model choice (MDR.py:286-333) stay on
the host in numpy; they are O(n) per fold.

Arithmetic: cell counts are integers; the risk decision is the integer form
of the reference's float64 comparison (identical for n < 2^25, and larger n
is rejected); BA is ``(tp / total_case + tn / total_control) / 2.0`` in IEEE
float64, rounded to float32.  CPU and GPU backends agree bit for bit.  The
reference's CPU kernel is ``@njit(fastmath=True)``, which allows LLVM to
reassociate those three float64 operations; no reference-produced fixture
pins numba's own bits, so parity with them is unpinned (as for the Relief
kernels).
"""
from __future__ import annotations

from collections import Counter

import numpy as np
from sklearn.base import BaseEstimator, ClassifierMixin
from sklearn.model_selection import StratifiedKFold
from sklearn.utils.multiclass import unique_labels
from sklearn.utils.validation import check_array, check_is_fitted, check_X_y

from . import _base, _lib

MAX_K_FOR_KERNEL = 6


def cell_index(X, interaction):
    """``cell = cell * 3 + genotype`` over the interaction's columns, first
    column most significant (MDR.py:41-45)."""
    cell = np.zeros(X.shape[0], dtype=np.int64)
    for j in interaction:
        cell = cell * 3 + X[:, j]
    return cell


def lookup_table(X, y, interaction):
    """The 3^k high-risk table of ``_create_lookup_table`` (MDR.py:176-195):
    ``case / (control + 1e-9) > total_case / total_control`` in float64 (an
    empty cell is low risk here, unlike in the scan)."""
    n_cells = 3 ** len(interaction)
    cell = cell_index(X, interaction)
    case = np.bincount(cell[y == 1], minlength=n_cells).astype(np.int32)
    control = np.bincount(cell[y != 1], minlength=n_cells).astype(np.int32)
    total_cases = case.sum()
    total_controls = control.sum()
    threshold = np.inf if total_controls == 0 else total_cases / total_controls
    ratios = case / (control + 1e-9)
    return (ratios > threshold).astype(np.uint8)


def fold_test_ba(Xc, y, train_idx, test_idx):
    """Test balanced accuracy of one model in one fold (MDR.py:296-313): the
    lookup table of the model's columns ``Xc`` on the training rows, applied
    to the test rows."""
    own = tuple(range(Xc.shape[1]))
    lookup = lookup_table(Xc[train_idx], y[train_idx], own)
    y_test = y[test_idx]
    y_pred_test = lookup[cell_index(Xc[test_idx], own)]
    tp = np.sum((y_test == 1) & (y_pred_test == 1))
    tn = np.sum((y_test == 0) & (y_pred_test == 0))
    n_pos = np.sum(y_test == 1)
    n_neg = np.sum(y_test == 0)
    sens = tp / n_pos if n_pos else 0
    spec = tn / n_neg if n_neg else 0
    return (sens + spec) / 2.0


def summarise_folds(X, y, splits, best_rank, k, verbose=False):
    """From every fold's best combination rank to the fitted model: the fold's
    lookup table on its training rows, its test balanced accuracy, the
    cross-validation consistency and the model choice (MDR.py:286-333).
    ``fit`` and ``permutation_test`` both end here.  Only the k columns of a
    fold's model are touched (``X[:, combo]`` before any row selection), so a
    labelling costs O(folds * n * k).  Returns (best model, its CVC, its mean
    test BA)."""
    n_features = X.shape[1]
    fold_best_models = []
    fold_test_bas = []
    for fold_i, (train_idx, test_idx) in enumerate(splits):
        best_combo = _lib.mdr_unrank(n_features, k, int(best_rank[fold_i]))
        fold_best_models.append(best_combo)
        test_ba = fold_test_ba(X[:, best_combo], y, train_idx, test_idx)
        fold_test_bas.append(test_ba)
        if verbose:
            print(f"  Fold {fold_i + 1}/{len(splits)}: best {best_combo}, Test BA = {test_ba:.4f}")

    counts = Counter(fold_best_models)
    max_cvc = counts.most_common(1)[0][1]
    best_model, best_avg_ba = None, -1.0
    for model in (m for m, c in counts.items() if c == max_cvc):
        avg_ba = float(np.mean([fold_test_bas[i] for i, m in enumerate(fold_best_models)
                                if m == model]))
        if avg_ba > best_avg_ba:
            best_avg_ba, best_model = avg_ba, model
    return best_model, max_cvc, best_avg_ba


class MDR(ClassifierMixin, BaseEstimator):
    """Multifactor dimensionality reduction on the MI355X or the CPU.

    All features must be SNP genotypes coded 0, 1, 2; ``y`` must hold two
    labels, and a sample is a case iff its label equals 1.

    Parameters
    ----------
    k : int, default=2
        Interaction order to search (at most 6).
    cv : int, default=10
        Stratified folds for model selection (shuffled, random_state=42).
    backend : {'auto', 'cpu', 'gpu'}, default='auto'
        Execution backend, case-insensitive.  'gpu' without a visible HIP
        device raises; it never falls back.
    verbose : bool, default=False
        Print progress information during training.
    n_jobs : int, default=-1
        CPU threads for backend='cpu' (-1 = all).  Not a reference parameter.
    device : int, default=0
        GPU ordinal for the GPU backend.  Not a reference parameter.

    Attributes
    ----------
    best_interaction_ : tuple of int
    best_cvc_ : int
    best_mean_testing_ba_ : float
    best_model_lookup_table_ : ndarray of uint8, shape (3**k,)
    classes_, n_features_in_, effective_backend_

    ``permutation_test`` fits and adds the permutation null: ``p_value_``,
    ``cvc_p_value_``, ``null_testing_ba_``, ``null_cvc_``, ``n_permutations_``.
    ``rank_interactions`` fits and adds the ranked list of the search:
    ``top_interactions_``, ``top_training_ba_``, ``top_mean_testing_ba_``,
    ``top_cvc_``, ``top_fold_hits_``.
    """

    def __init__(self, k: int = 2, cv: int = 10, backend: str = "auto", verbose: bool = False,
                 n_jobs: int = -1, device: int = 0):
        self.k = k
        self.cv = cv
        self.backend = backend
        self.verbose = verbose
        self.n_jobs = n_jobs
        self.device = device

    def _validate(self, X, y):
        """The checks of ``fit`` (MDR.py:220-244) and the reference's folds:
        (X, y, k, fold ids, splits)."""
        X, y = check_X_y(X, y, dtype=np.uint8)
        self.classes_ = unique_labels(y)
        if len(self.classes_) != 2:
            raise ValueError("MDR only supports binary classification.")
        if np.max(X) > 2 or np.min(X) < 0:
            raise ValueError("Genotypes must be coded 0/1/2.")
        if self.k > MAX_K_FOR_KERNEL:
            raise ValueError(f"k={self.k} exceeds MAX_K_FOR_KERNEL={MAX_K_FOR_KERNEL}.")
        n_samples, n_features = X.shape
        if self.k > n_features:
            raise ValueError(f"k must be ≤ n_features. Got k={self.k}, n_features={n_features}")
        backend = self.backend.lower() if isinstance(self.backend, str) else self.backend
        if backend not in ("auto", "cpu", "gpu"):
            raise ValueError("backend must be 'auto', 'CPU', or 'GPU'.")
        self.effective_backend_ = _base.effective_backend(backend)
        self.n_features_in_ = n_features
        k = int(self.k)

        X = np.ascontiguousarray(X)
        skf = StratifiedKFold(n_splits=self.cv, shuffle=True, random_state=42)
        splits = list(skf.split(X, y))
        fold = np.empty(n_samples, dtype=np.int32)
        for i, (_, test_idx) in enumerate(splits):
            fold[test_idx] = i
        if self.verbose:
            print(f"CV with backend={self.effective_backend_.upper()}: {k}-way search over "
                  f"{_lib.mdr_combinations(n_features, k)} combos")
        return X, y, k, fold, splits

    def _set_model(self, X, y, model, cvc, mean_ba):
        self.best_interaction_ = model
        self.best_cvc_ = cvc
        self.best_mean_testing_ba_ = mean_ba
        if self.verbose:
            print("\nFit Complete")
            print(f"Best interaction: {self.best_interaction_}")
            print(f"CVC: {self.best_cvc_}/{self.cv}")
            print(f"Mean testing BA: {self.best_mean_testing_ba_:.4f}")
        self.best_model_lookup_table_ = lookup_table(X, y, self.best_interaction_)

    def fit(self, X, y):
        """Find the best k-way interaction by cross-validated MDR."""
        X, y, k, fold, splits = self._validate(X, y)
        _, best_rank = _lib.mdr_scan(self.effective_backend_, X, y == 1, k, fold, len(splits),
                                     device=self.device, n_jobs=self.n_jobs)
        self._set_model(X, y, *summarise_folds(X, y, splits, best_rank, k, self.verbose))
        return self

    def permutation_test(self, X, y, n_permutations=1000, random_state=None):
        """``fit`` plus the permutation null of its two statistics.

        The whole search runs on the observed phenotype and on
        ``n_permutations`` permuted ones in one ``fs_mdr_scan_labels`` call.
        The case flags are permuted *within each fold* (``rng =
        np.random.default_rng(random_state)``; labellings in order, folds in
        order, ``rng.permutation`` of the fold's flags), so every fold keeps
        its class counts, the folds stay stratified for every labelling and
        are the ones ``fit`` draws.  Sets every attribute ``fit`` sets, with
        the same values, and

        null_testing_ba_ : ndarray of float64, shape (n_permutations,)
            ``best_mean_testing_ba_`` of each permuted labelling.
        null_cvc_ : ndarray of int, shape (n_permutations,)
        p_value_ : float
            ``(1 + #{null_testing_ba_ >= best_mean_testing_ba_}) / (1 + n_permutations)``.
        cvc_p_value_ : float
            The same on the cross-validation consistency.
        n_permutations_ : int
        """
        n_perm = int(n_permutations)
        if n_perm < 1:
            raise ValueError(f"n_permutations must be >= 1. Got {n_permutations}")
        X, y, k, fold, splits = self._validate(X, y)
        rng = np.random.default_rng(random_state)
        labels = np.empty((n_perm + 1, X.shape[0]), dtype=np.uint8)
        labels[0] = y == 1
        for b in range(1, n_perm + 1):
            for _, test_idx in splits:
                labels[b, test_idx] = rng.permutation(labels[0, test_idx])
        _, best_rank = _lib.mdr_scan_labels(self.effective_backend_, X, labels, k, fold,
                                            len(splits), device=self.device, n_jobs=self.n_jobs)

        self._set_model(X, y, *summarise_folds(X, y, splits, best_rank[0], k, self.verbose))
        # a permuted phenotype in y's own two labels: 1 for a case
        others = self.classes_[self.classes_ != 1]
        control = others[0] if len(others) else self.classes_[0]
        null_ba = np.empty(n_perm, dtype=np.float64)
        null_cvc = np.empty(n_perm, dtype=np.int64)
        for b in range(1, n_perm + 1):
            yb = np.where(labels[b] != 0, np.asarray(1, dtype=y.dtype), control)
            _, null_cvc[b - 1], null_ba[b - 1] = summarise_folds(X, yb, splits, best_rank[b], k)
        self.null_testing_ba_ = null_ba
        self.null_cvc_ = null_cvc
        self.n_permutations_ = n_perm
        self.p_value_ = (1 + int(np.sum(null_ba >= self.best_mean_testing_ba_))) / (1 + n_perm)
        self.cvc_p_value_ = (1 + int(np.sum(null_cvc >= self.best_cvc_))) / (1 + n_perm)
        return self

    def rank_interactions(self, X, y, n_top=100):
        """``fit`` plus the ranked list of the search: the ``n_top`` best
        k-way interactions by balanced accuracy on all samples, and how each
        fares under cross-validation.

        Two ``fs_mdr_scan_top`` calls, one without folds and one with the
        folds ``fit`` draws; the per-model test accuracies are host numpy,
        O(m * folds * n * k).  Sets every attribute ``fit`` sets, with the same
        values, and with m = min(n_top, C(p, k))

        top_interactions_ : ndarray of int, shape (m, k)
            Ordered by BA on all samples, ties by combination rank.
        top_training_ba_ : ndarray of float32, shape (m,)
            That BA (the scan without folds).
        top_mean_testing_ba_ : ndarray of float64, shape (m,)
            Mean over all cv folds of the model's test BA, each fold's lookup
            table built on its training rows.
        top_cvc_ : ndarray of int, shape (m,)
            Folds in which the model is that fold's best.
        top_fold_hits_ : ndarray of int, shape (m,)
            Folds in which it is among that fold's ``n_top`` best.
        """
        n_top = int(n_top)
        if n_top < 1:
            raise ValueError(f"n_top must be >= 1. Got {n_top}")
        if n_top > _lib.MDR_MAX_TOP:
            raise ValueError(f"n_top must be <= {_lib.MDR_MAX_TOP} (the library's kMdrMaxTop). "
                             f"Got {n_top}")
        X, y, k, fold, splits = self._validate(X, y)
        scan = dict(n_top=n_top, device=self.device, n_jobs=self.n_jobs)
        all_ba, all_rank = _lib.mdr_scan_top(self.effective_backend_, X, y == 1, k, **scan)
        _, fold_rank = _lib.mdr_scan_top(self.effective_backend_, X, y == 1, k, fold, len(splits),
                                         **scan)
        self._set_model(X, y, *summarise_folds(X, y, splits, fold_rank[:, 0], k, self.verbose))

        m = min(n_top, _lib.mdr_combinations(X.shape[1], k))
        ranks = all_rank[0, :m]
        combos = [_lib.mdr_unrank(X.shape[1], k, int(r)) for r in ranks]
        self.top_interactions_ = np.array(combos, dtype=np.int64).reshape(m, k)
        self.top_training_ba_ = all_ba[0, :m].copy()
        self.top_mean_testing_ba_ = np.array(
            [np.mean([fold_test_ba(X[:, c], y, tr, te) for tr, te in splits]) for c in combos],
            dtype=np.float64)
        self.top_cvc_ = np.array([np.sum(fold_rank[:, 0] == r) for r in ranks], dtype=np.int64)
        self.top_fold_hits_ = np.array([np.sum(np.any(fold_rank == r, axis=1)) for r in ranks],
                                       dtype=np.int64)
        return self

    def predict(self, X):
        """1 for samples in a high-risk cell of the best interaction, else 0."""
        check_is_fitted(self)
        X = check_array(X, dtype=np.uint8)
        if X.shape[1] != self.n_features_in_:
            raise ValueError(f"X has {X.shape[1]} features, but MDR is expecting "
                             f"{self.n_features_in_} features as input.")
        if np.max(X[:, list(self.best_interaction_)], initial=0) > 2:
            raise ValueError("Genotypes must be coded 0/1/2.")
        return self.best_model_lookup_table_[cell_index(X, self.best_interaction_)]

    def transform(self, X):
        return self.predict(X).reshape(-1, 1)

    def predict_proba(self, X):
        """Not implemented: MDR is a hard classifier (as in the reference)."""
        raise NotImplementedError("predict_proba is not supported in this MDR implementation.")
