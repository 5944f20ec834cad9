"""Float64 numpy model of STIR -- TEST INFRASTRUCTURE ONLY.

The definitions of fastselect_amd/csrc/fs_stir.h restated on the
``multisurf`` loop of ``oracle/relief_np.py``: the same per-feature diffs
(``_diff_rows``: the reference's float32 diffs widened to float64), distances,
thresholds and near sets, with the four pooled sums per feature in place of
the weighted one, and the epilogue.  Nothing here calls the library.
"""
from __future__ import annotations

import numpy as np

from oracle import relief_np


def mixed_case(n=300, pc=20, pd=20, seed=0):
    """The standard case: pc uniform float32 columns, then pd columns of
    integers in {0, 1, 2}; y from continuous column 3 and discrete column
    pc + 5 (n = 300, p = 40: three row blocks with a ragged last one, one
    feature block half continuous and half discrete)."""
    rng = np.random.default_rng(seed)
    x = rng.random((n, pc + pd)).astype(np.float32)
    x[:, pc:] = rng.integers(0, 3, size=(n, pd))
    a = x[:, 3] if pc > 3 else 0.0
    b = 0.5 * (x[:, pc + 5] == 2) if pd > 5 else 0.0
    y = (a + b + 0.3 * rng.standard_normal(n) > 0.7).astype(np.float64)
    return x, y


def preprocess(x, discrete_limit=10):
    """(recip, is_discrete) as MultiSURF.fit derives them (MultiSURF.py:384-420)."""
    isd = np.array([np.unique(x[:, f]).size <= discrete_limit for f in range(x.shape[1])])
    ranges = (x.max(0) - x.min(0)).astype(np.float32)
    ranges[ranges == 0] = 1
    return (1.0 / ranges).astype(np.float32), isd


def stir_sums(x32, y, recip, is_disc, rows=None):
    """(sums[4, p], |H|, |M|, counts[n, 2]) of the focal samples ``rows``
    (default all): S1H, S2H, S1M, S2M over the ordered near pairs."""
    n, p = x32.shape
    lo, hi = (0, n) if rows is None else rows
    sums = np.zeros((4, p), dtype=np.float64)
    counts = np.zeros((n, 2), dtype=np.int64)
    for i in range(lo, hi):
        d = relief_np._diff_rows(x32, i, recip, is_disc)     # (n, p) float64
        dist = d.sum(axis=1)
        others = np.arange(n) != i
        mu = dist[others].sum() / (n - 1)
        var = max(0.0, (dist[others] ** 2).sum() / (n - 1) - mu * mu)
        near = (dist < mu - 0.5 * np.sqrt(var)) & others
        nh, nm = near & (y == y[i]), near & (y != y[i])
        sums[0] += d[nh].sum(axis=0)
        sums[1] += (d[nh] ** 2).sum(axis=0)
        sums[2] += d[nm].sum(axis=0)
        sums[3] += (d[nm] ** 2).sum(axis=0)
        counts[i] = nh.sum(), nm.sum()
    return sums, int(counts[:, 0].sum()), int(counts[:, 1].sum()), counts


def statistics(sums, n_hit, n_miss):
    """(hit_mean, miss_mean, t, df, p) of the epilogue; p one-sided."""
    from scipy.stats import t as student_t
    nh, nm = float(n_hit), float(n_miss)
    hbar, mbar = sums[0] / nh, sums[2] / nm
    vh = np.maximum((sums[1] - nh * hbar ** 2) / (nh - 1), 0.0)
    vm = np.maximum((sums[3] - nm * mbar ** 2) / (nm - 1), 0.0)
    sp = np.sqrt(((nm - 1) * vm + (nh - 1) * vh) / (nm + nh - 2))
    d = mbar - hbar
    with np.errstate(divide="ignore", invalid="ignore"):
        t = d / (sp * np.sqrt(1 / nm + 1 / nh))
    flat = sp == 0
    t[flat] = np.where(d[flat] > 0, np.inf, np.where(d[flat] < 0, -np.inf, 0.0))
    df = nm + nh - 2
    pv = student_t.sf(t, df)
    pv[flat] = np.where(d[flat] > 0, 0.0, 1.0)
    return hbar, mbar, t, df, pv


def t_tolerance(sums, n_hit, n_miss, rel):
    """Absolute tolerance on t per feature when every sum is within ``rel``
    relative of the model's: the means move by at most rel * Mbar and
    rel * Hbar, so t by rel * (Mbar + Hbar) / (sp * sqrt(1/|M| + 1/|H|))
    (the sums of squares move sp by a relative rel at most, second order
    here).  inf where sp == 0."""
    nh, nm = float(n_hit), float(n_miss)
    hbar, mbar = sums[0] / nh, sums[2] / nm
    vh = np.maximum((sums[1] - nh * hbar ** 2) / (nh - 1), 0.0)
    vm = np.maximum((sums[3] - nm * mbar ** 2) / (nm - 1), 0.0)
    sp = np.sqrt(((nm - 1) * vm + (nh - 1) * vh) / (nm + nh - 2))
    with np.errstate(divide="ignore"):
        return rel * (mbar + hbar) / (sp * np.sqrt(1 / nm + 1 / nh))


def benjamini_hochberg(p):
    """Benjamini-Hochberg adjusted p-values, the textbook loop."""
    p = np.asarray(p, dtype=np.float64)
    m = p.size
    order = sorted(range(m), key=lambda k: p[k])
    out = np.empty(m)
    running = 1.0
    for rank in range(m, 0, -1):
        k = order[rank - 1]
        running = min(running, p[k] * m / rank)
        out[k] = running
    return out
