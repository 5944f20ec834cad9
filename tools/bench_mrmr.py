#!/usr/bin/env python
"""Time selection-only mRMR (fs_mrmr_select) on the GPU (MI355X) and the CPU
backend, beside the matrix route where the matrix fits.

One JSON line per shape.  A "selected call" is what mRMR.fit hands to the
native library with redundancy="selected": one fs_mrmr_select (upload, pack,
relevance, k - 1 x (row, step), one download) on codes that are already uint8,
with the k rows returned as the estimator asks; it is synchronous, so the host
clock around it covers device work that has finished.  The line holds the
median call time, the fs_mrmr_last_timing breakdown of one call (upload, pack,
relevance with the first pick, rows, steps; HIP events), the time per step
((rows + steps) / (k - 1), and the host clock's share after upload, pack and
relevance), the same call without rows, and the CPU backend's call at 16
threads.  Both backends must select the same features.

A "matrix route" is what redundancy="matrix" hands over: one fs_mi_matrices
call (the p x p float64 matrix computed and downloaded) plus the numpy greedy
loop of mRMR.fit on the host, timed in the same session, alternating with the
selected call.  It is skipped where the matrix does not fit (wide3: 80 GB).
"Python encoding" is the np.unique + searchsorted of mRMR.fit over all of X,
which both modes pay before the call.

The data is bench_cfs.py's: 40 columns are independent noisy copies of a
3-class target; k = 40.

    python tools/bench_mrmr.py                          # the three shapes
    python tools/bench_mrmr.py --shape geno3 --out profiles/mrmr/bench_mrmr.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_cfs import N_PLANTED, SHAPES, make  # noqa: E402

K = N_PLANTED
NO_MATRIX = ("wide3",)   # p x p float64 would be 80 GB


def greedy_numpy(rel, red, k, method):
    """The loop of mRMR.fit (redundancy="matrix") on the host."""
    p = rel.shape[0]
    sel = np.zeros(k, dtype=np.int32)
    left = np.ones(p, dtype=bool)
    first = np.argmax(rel)
    sel[0] = first
    left[first] = False
    rsum = red[:, first].copy()
    for i in range(1, k):
        idx = np.where(left)[0]
        if method == "MID":
            scores = rel[idx] - (rsum[idx] / i)
        else:
            scores = rel[idx] / ((rsum[idx] / i) + 1e-9)
        top = idx[np.isclose(scores, np.max(scores), atol=1e-12)]
        best = top[np.argmin(rsum[top] / i)] if top.size > 1 else top[0]
        sel[i] = best
        left[best] = False
        rsum += red[:, best]
    return sel


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def run(name, warmup, reps, cpu_threads, method):
    from fastselect_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("bench_mrmr: no HIP device visible")
    n, p, states = SHAPES[name]
    X, y = make(n, p, states)
    with_matrix = name not in NO_MATRIX

    def selected(rows=True, backend="gpu", n_jobs=-1):
        return _lib.mrmr_select(backend, X, y, states, K, method=method, n_jobs=n_jobs,
                                want_rows=rows)

    def matrix():
        rel, red = _lib.mi_matrices("gpu", X, y, states)
        return greedy_numpy(rel, red, K, method)

    ts, tm, tn = [], [], []
    sel = msel = None
    for r in range(warmup + reps):   # alternating, the same session
        a, (sel, _, _) = clock(selected)
        timing = _lib.mrmr_last_timing()
        b, _ = clock(lambda: selected(rows=False))
        if with_matrix:
            c, msel = clock(matrix)
        if r >= warmup:
            ts.append(a)
            tn.append(b)
            if with_matrix:
                tm.append(c)
    up, pack, relv, rows, steps = timing
    cts = [clock(lambda: selected(backend="cpu", n_jobs=cpu_threads)) for _ in range(3)]
    cmed = statistics.median(t for t, _ in cts)
    csel = cts[-1][1][0]
    enc_ms, _ = clock(lambda: (lambda u: (np.searchsorted(u, X), np.searchsorted(u, y)))(
        np.unique(np.concatenate([np.unique(X), np.unique(y)]))))
    med = statistics.median(ts)
    line = {
        "bench": "mrmr_selected", "shape": name, "n": n, "p": p, "states": states, "k": K,
        "method": method,
        "gpu_ms_per_call": round(med, 3), "gpu_ms_min": round(min(ts), 3),
        "gpu_ms_max": round(max(ts), 3),
        "gpu_ms_per_call_no_rows": round(statistics.median(tn), 3),
        "gpu_ms_upload": round(up, 3), "gpu_ms_pack": round(pack, 3),
        "gpu_ms_relevance": round(relv, 3), "gpu_ms_rows": round(rows, 3),
        "gpu_ms_steps": round(steps, 3),
        "gpu_us_per_step": round((rows + steps) / (K - 1) * 1e3, 2),
        "gpu_us_per_step_host": round((med - up - pack - relv) / (K - 1) * 1e3, 2),
        "pairs_computed": int((K + 1) * p), "pairs_of_full_matrix": int(p * (p - 1) // 2 + p),
        "rows_bytes": int(K * p * 8), "full_matrix_bytes_f64": int(p * p * 8),
        "cpu_threads": cpu_threads, "cpu_ms_per_call": round(cmed, 3),
        "gpu_faster_than_cpu": bool(med < cmed),
        "same_selection_as_cpu": bool(np.array_equal(csel, sel)),
        "python_encoding_ms": round(enc_ms, 1),
        "warmup": warmup, "reps": reps,
        "how": "host clock around synchronous calls, medians; breakdown from HIP events",
    }
    if with_matrix:
        mmed = statistics.median(tm)
        line.update({
            "matrix_route_ms": round(mmed, 3), "matrix_route_ms_min": round(min(tm), 3),
            "matrix_route_ms_max": round(max(tm), 3),
            "selected_not_slower_than_matrix_route": bool(med <= mmed),
            "same_selection_as_matrix_route": bool(np.array_equal(msel, sel)),
        })
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", choices=sorted(SHAPES), action="append")
    ap.add_argument("--method", choices=["MID", "MIQ"], default="MID")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--out", help="append the JSON lines to this file too")
    a = ap.parse_args()
    for name in a.shape or ["geno3", "states10", "wide3"]:
        line = json.dumps(run(name, a.warmup, a.reps, a.cpu_threads, a.method))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
