#!/usr/bin/env python
"""Time CFS (fs_cfs_*) on the GPU (MI355X) and the CPU backend.

One JSON line per shape.  A "call" is what CFS.fit hands to the native
library: fs_cfs_create (upload, pack, class correlations), fs_cfs_search (one
lazy row of symmetrical uncertainty and one scan per step) and
fs_cfs_destroy, on codes that are already uint8; it is synchronous, so the
host clock around it covers device work that has finished.  The line holds
the median call time, the fs_cfs_last_timing breakdown of one call (upload,
pack, relevance, rows, steps; HIP events), the number of features selected,
the number of steps (scans, the stopping one included), the time per step
(rows + steps over the steps) and the CPU backend's call time at 16 threads.
The data is planted so that the search is some tens of steps deep: 40 columns
are independent noisy copies of a 3-class target.  Both backends must select
the same features.  --mi adds one fs_mi_matrices GPU call of the same shape,
the only route to a full matrix the library has.

    python tools/bench_cfs.py                          # the three shapes
    python tools/bench_cfs.py --shape geno3 --mi --out profiles/cfs/bench_cfs.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {
    # name: (n, p, states)
    "geno3": (2000, 5000, 3),
    "wide3": (2000, 100000, 3),
    "states10": (2000, 2000, 10),
}
N_PLANTED = 40


def make(n, p, states, seed=0):
    """y uniform over 3 classes; N_PLANTED columns spread over the width are
    copies of y with 45 % to 70 % of their entries replaced by noise, each
    independently; every other column is uniform noise."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 3, size=n)
    X = rng.integers(0, states, size=(n, p)).astype(np.uint8)
    cols = np.linspace(1, p - 2, N_PLANTED).astype(int)
    for col, frac in zip(cols, np.linspace(0.45, 0.70, N_PLANTED)):
        noisy = rng.random(n) < frac
        X[:, col] = np.where(noisy, rng.integers(0, states, size=n), y)
    return X, y.astype(np.uint8)


def call(backend, X, y, states, n_jobs):
    from fastselect_amd import _lib
    with _lib.Cfs(backend, X, y, states, n_jobs=n_jobs) as h:
        return h.search()


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def run(name, warmup, reps, cpu_threads, with_mi):
    from fastselect_amd import CFS, _lib
    if _lib.device_count() < 1:
        raise SystemExit("bench_cfs: no HIP device visible")
    n, p, states = SHAPES[name]
    X, y = make(n, p, states)
    out = {}
    med, lo, hi = timed(lambda: out.update(g=call("gpu", X, y, states, -1)), warmup, reps)
    up, pack, rel, rows, steps = _lib.cfs_last_timing()
    sel, merits = out["g"]
    n_steps = len(sel)  # len - 1 accepting scans and the stopping one
    cmed, _, _ = timed(lambda: out.update(c=call("cpu", X, y, states, cpu_threads)), 1, 3)
    t0 = time.perf_counter()
    est = CFS(backend="gpu").fit(X, y)
    fit_ms = (time.perf_counter() - t0) * 1e3
    line = {
        "bench": "cfs", "shape": name, "n": n, "p": p, "states": states,
        "gpu_ms_per_call": round(med, 3), "gpu_ms_min": round(lo, 3), "gpu_ms_max": round(hi, 3),
        "gpu_ms_upload": round(up, 3), "gpu_ms_pack": round(pack, 3),
        "gpu_ms_relevance": round(rel, 3), "gpu_ms_rows": round(rows, 3),
        "gpu_ms_steps": round(steps, 3),
        "n_selected": int(len(sel)), "steps": n_steps,
        "gpu_ms_per_step": round((rows + steps) / max(n_steps, 1), 4),
        "gpu_ms_per_step_host": round((med - up - pack - rel) / max(n_steps, 1), 4),
        "merit": float(merits[-1]) if len(merits) else 0.0,
        "pairs_computed": int((len(sel) + 1) * p), "pairs_of_full_matrix": int(p * (p - 1) // 2 + p),
        "row_cache_bytes": int(max(len(sel), 16) * p * 4), "full_matrix_bytes_f32": int(p * p * 4),
        "cpu_threads": cpu_threads, "cpu_ms_per_call": round(cmed, 3),
        "gpu_faster_than_cpu": bool(med < cmed),
        "same_selection_as_cpu": bool(np.array_equal(out["c"][0], sel)),
        "estimator_fit_ms": round(fit_ms, 1), "estimator_n_selected": int(est.selected_indices_.size),
        "warmup": warmup, "reps": reps,
    }
    if with_mi:
        mmed, _, _ = timed(lambda: _lib.mi_matrices("gpu", X, y, states), 1, 3)
        line["mi_matrices_gpu_ms_per_call"] = round(mmed, 3)
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", choices=sorted(SHAPES), action="append")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--mi", action="store_true", help="also time fs_mi_matrices on the GPU "
                    "(needs the p x p float64 matrix on the host: not for wide3)")
    ap.add_argument("--out", help="append the JSON lines to this file too")
    a = ap.parse_args()
    for name in a.shape or ["geno3", "wide3", "states10"]:
        line = json.dumps(run(name, a.warmup, a.reps, a.cpu_threads, a.mi and name != "wide3"))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
