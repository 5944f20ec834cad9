"""Device-resident re-scoring of column subsets for ReliefF and SURF (the
TuRF caller, TuRF.py:93-115): X is uploaded once into a ReliefF / SURF plan
(``fs_plan_create_relieff`` / ``_surf``) and every ``refit(active)`` re-targets
it with ``fs_plan_set_features`` instead of refitting on ``X[:, active]``.
Per-column preprocessing (discreteness, ranges) does not depend on the other
columns, so the subset's inputs are the full ones restricted to ``active``.
``ResidentTargets`` does the same for RReliefF on a one-class ReliefF plan.
"""
from __future__ import annotations

import numpy as np

from . import _base, _lib


class ResidentRows:
    """``refit(active)`` leaves ``est`` exactly as ``est.fit(X[:, active], y)``
    would (fitted attributes included), scoring on the resident plan."""

    def __init__(self, est, name: str, plan: _lib.RowsPlan, n: int, is_discrete, backend: str,
                 before_score=None):
        self.est = est
        self.name = name
        self.plan = plan
        self.n = n
        self.is_discrete = is_discrete
        self.backend = backend
        self.before_score = before_score
        self.active = None
        self._buf = None

    def _sums(self, n_kept: int) -> np.ndarray:
        if self.backend == "gpu":
            import torch
            if self._buf is None or self._buf.numel() != n_kept:
                # no fill kernel: the plan clears the sums on its own stream.
                # That stream is non-blocking, so nothing torch queued on its
                # stream is ordered before the plan's kernels -- a torch.zeros
                # here could land after the plan's k_reduce and wipe the
                # sums (TuRF over ReliefF varied run to run that way)
                self._buf = torch.empty(n_kept, dtype=torch.float64, device="cuda")
            torch.cuda.current_stream().synchronize()
            self.plan.score(self._buf.data_ptr())  # synchronises the plan's stream
            return self._buf.cpu().numpy()
        out = np.zeros(n_kept, dtype=np.float64)
        self.plan.score(out.ctypes.data)
        return out

    def score_stir(self):
        """One ``fs_plan_score_stir`` call on the current feature subset (a
        ReliefF plan): (score_sums[n_kept], stir_sums (4, n_kept), |H|, |M|),
        the score sums being ``_sums``'s bits."""
        n_kept = self.plan.n_kept
        if self.backend == "gpu":
            import torch
            # torch.empty, no fill kernels, and the same ordering as _sums
            sums = torch.empty(n_kept, dtype=torch.float64, device="cuda")
            stir = torch.empty(4 * n_kept, dtype=torch.float64, device="cuda")
            counts = torch.empty(2, dtype=torch.float64, device="cuda")
            torch.cuda.current_stream().synchronize()
            # synchronises the plan's stream
            self.plan.score_stir(sums.data_ptr(), stir.data_ptr(), counts.data_ptr())
            sums, stir, counts = sums.cpu().numpy(), stir.cpu().numpy(), counts.cpu().numpy()
        else:
            sums = np.zeros(n_kept, dtype=np.float64)
            stir = np.zeros(4 * n_kept, dtype=np.float64)
            counts = np.zeros(2, dtype=np.float64)
            self.plan.score_stir(sums.ctypes.data, stir.ctypes.data, counts.ctypes.data)
        return sums, stir.reshape(4, n_kept), int(counts[0]), int(counts[1])

    def score_labels(self, labels) -> np.ndarray:
        """One labellings call on the current feature subset: the (B, n_kept)
        float64 score sums of the (B, n) labellings.  A ReliefF plan:
        ``fs_plan_relieff_score_labels``, class codes in [0, 64); a SURF plan:
        ``fs_plan_surf_score_labels``."""
        if self.plan.algo == "surf":
            return self._surf_score_labels(labels)
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if labels.ndim == 1:
            labels = labels.reshape(1, -1)
        B, n_kept = labels.shape[0], self.plan.n_kept
        if self.backend == "gpu":
            import torch
            # torch.empty, no fill kernels, and the same ordering as _sums
            out = torch.empty(max(B * n_kept, 1), dtype=torch.float64, device="cuda")
            torch.cuda.current_stream().synchronize()
            self.plan.score_labels(labels, out.data_ptr())  # synchronises the plan's stream
            return out[:B * n_kept].cpu().numpy().reshape(B, n_kept)
        out = np.zeros((B, n_kept), dtype=np.float64)
        self.plan.score_labels(labels, out.ctypes.data)
        return out

    def _surf_score_labels(self, labels) -> np.ndarray:
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if labels.ndim == 1:
            labels = labels.reshape(1, -1)
        B, n_kept = labels.shape[0], self.plan.n_kept
        if self.backend == "gpu":
            import torch
            # torch.empty, no fill kernels, and the same ordering as _sums
            out = torch.empty(max(B * n_kept, 1), dtype=torch.float64, device="cuda")
            torch.cuda.current_stream().synchronize()
            self.plan.surf_score_labels(labels, out.data_ptr())  # synchronises the plan's stream
            return out[:B * n_kept].cpu().numpy().reshape(B, n_kept)
        out = np.zeros((B, n_kept), dtype=np.float64)
        self.plan.surf_score_labels(labels, out.ctypes.data)
        return out

    def refit(self, active, stir=False):
        """stir: score through ``score_stir`` and keep its STIR sums and pair
        counts in ``stir_`` = (sums (4, n_kept), |H|, |M|)."""
        est = self.est
        active = np.asarray(active, dtype=np.int64)
        n_select = est._validate_parameters(self.n, active.size)
        est.n_features_in_ = active.size
        if self.before_score is not None:
            self.before_score()
        if est.verbose:
            print(f"Running {self.name} on the {self.backend.upper()} now...")
        if self.active is None or not np.array_equal(active, self.active):
            self.plan.set_features(active)
            self.active = active
        if stir:
            sums, *self.stir_ = self.score_stir()
        else:
            sums = self._sums(active.size)
        scores = (sums / self.n).astype(np.float32)
        est.is_discrete_ = self.is_discrete[active]
        est.feature_importances_ = scores
        est.top_features_ = _base.top_features(scores, n_select)
        return est

    def close(self):
        self.plan.close()


class ResidentTargets:
    """RReliefF on a resident one-class ReliefF plan: ``refit(active)`` leaves
    ``est`` exactly as ``est.fit(X[:, active], y)`` would, and
    ``score_targets(targets)`` scores any number of targets of the same
    samples in one ``fs_plan_score_targets`` call (the neighbours do not read
    the target, so distances and selection run once per call)."""

    def __init__(self, est, plan: _lib.RowsPlan, n: int, k: int, y, is_discrete, backend: str):
        self.est = est
        self.plan = plan
        self.n = n
        self.k = k
        self.y = np.ascontiguousarray(y, dtype=np.float64)
        self.is_discrete = is_discrete
        self.backend = backend
        self.active = None

    def sums(self, targets):
        """(S_A (n_kept), S_CA (B, n_kept), S_C (B)) of the (B, n) targets on
        the current feature subset."""
        targets = np.ascontiguousarray(targets, dtype=np.float64)
        if targets.ndim == 1:
            targets = targets.reshape(1, -1)
        B, n_kept = targets.shape[0], self.plan.n_kept
        if self.backend == "gpu":
            import torch
            # torch.empty, no fill kernels: the plan clears its sums on its own
            # (non-blocking) stream, which nothing torch queued is ordered
            # before (ResidentRows._sums)
            buf = torch.empty(n_kept + B * n_kept + B, dtype=torch.float64, device="cuda")
            torch.cuda.current_stream().synchronize()
            p0 = buf.data_ptr()
            # synchronises the plan's stream
            self.plan.score_targets(targets, p0, p0 + 8 * n_kept, p0 + 8 * (n_kept + B * n_kept))
            out = buf.cpu().numpy()
        else:
            out = np.zeros(n_kept + B * n_kept + B, dtype=np.float64)
            p0 = out.ctypes.data
            self.plan.score_targets(targets, p0, p0 + 8 * n_kept, p0 + 8 * (n_kept + B * n_kept))
        return (out[:n_kept], out[n_kept:n_kept + B * n_kept].reshape(B, n_kept),
                out[n_kept + B * n_kept:])

    def score_targets(self, targets) -> np.ndarray:
        """The (B, n_kept) float32 RReliefF scores of the (B, n) targets."""
        s_a, s_ca, s_c = self.sums(targets)
        return _lib.rrelieff_scores(s_a, s_ca, s_c, float(self.n) * float(self.k))

    def refit(self, active):
        est = self.est
        active = np.asarray(active, dtype=np.int64)
        n_select = est._validate_parameters(self.n, active.size)
        est.n_features_in_ = active.size
        if est.verbose:
            print(f"Running RReliefF on the {self.backend.upper()} now...")
        if self.active is None or not np.array_equal(active, self.active):
            self.plan.set_features(active)
            self.active = active
        scores = self.score_targets(self.y)[0]
        est.is_discrete_ = self.is_discrete[active]
        est.feature_importances_ = scores
        est.top_features_ = _base.top_features(scores, n_select)
        return est

    def close(self):
        self.plan.close()
