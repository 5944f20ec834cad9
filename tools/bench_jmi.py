#!/usr/bin/env python
"""Time JMI / CMIM selection (fs_jmi_select) on the GPU (MI355X) and the CPU
backend, beside fs_mrmr_select of the same session.

One JSON line per shape.  A "call" is what JMI.fit hands to the native library:
one fs_jmi_select (upload, pack, relevance, k - 1 x (row, step), the last row,
one download) on codes that are already uint8, with the k rows returned as the
estimator asks; it is synchronous, so the host clock around it covers device
work that has finished.  The line holds the median call time, the
fs_jmi_last_timing breakdown of one call (upload, pack, relevance with the
first pick, rows, steps; HIP events), the device time of one row kernel
(rows / k) and of one step's kernels (steps / (k - 1)), the same call without
rows, and the CPU backend's call at 16 threads.

The comparison point is fs_mrmr_select on the same data, alternating with the
JMI call in the same session: its call time, its breakdown, and the ratio of a
k_jmi_row to a k_mi_row (rows / k of each).  Both kernels stream the same
column planes once per row; k_jmi_row counts them against one masked copy of
the anchor per class of y and runs the epilogue on a table C times as large.

The data is bench_cfs.py's: 40 columns are independent noisy copies of a
3-class target; k = 40.

    python tools/bench_jmi.py                          # the three shapes
    python tools/bench_jmi.py --shape geno3 --out profiles/jmi/bench_jmi.jsonl
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


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def run(name, warmup, reps, cpu_threads, method):
    from fastselect_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("bench_jmi: no HIP device visible")
    n, p, states = SHAPES[name]
    X, y = make(n, p, states)
    classes = int(y.max()) + 1

    def jmi(rows=True, backend="gpu", n_jobs=-1):
        return _lib.jmi_select(backend, X, y, states, K, method=method, n_jobs=n_jobs,
                               want_rows=rows)

    def mrmr():
        return _lib.mrmr_select("gpu", X, y, states, K, method="MID")

    tj, tn, tm = [], [], []
    sel = None
    for r in range(warmup + reps):   # alternating, the same session
        a, (sel, _, _) = clock(jmi)
        timing = _lib.jmi_last_timing()
        b, _ = clock(lambda: jmi(rows=False))
        c, _ = clock(mrmr)
        mtiming = _lib.mrmr_last_timing()
        if r >= warmup:
            tj.append(a)
            tn.append(b)
            tm.append(c)
    up, pack, relv, rows, steps = timing
    mup, mpack, mrelv, mrows, msteps = mtiming
    cts = [clock(lambda: jmi(backend="cpu", n_jobs=cpu_threads)) for _ in range(3)]
    cmed = statistics.median(t for t, _ in cts)
    csel = cts[-1][1][0]
    med, mmed = statistics.median(tj), statistics.median(tm)
    return {
        "bench": "jmi_select", "shape": name, "n": n, "p": p, "states": states,
        "classes": classes, "k": K, "method": method,
        "gpu_ms_per_call": round(med, 3), "gpu_ms_min": round(min(tj), 3),
        "gpu_ms_max": round(max(tj), 3),
        "gpu_ms_per_call_no_rows": round(statistics.median(tn), 3),
        "gpu_ms_upload": round(up, 3), "gpu_ms_pack": round(pack, 3),
        "gpu_ms_relevance": round(relv, 3), "gpu_ms_rows": round(rows, 3),
        "gpu_ms_steps": round(steps, 3),
        "gpu_us_per_row_kernel": round(rows / K * 1e3, 2),
        "gpu_us_per_step_kernels": round(steps / (K - 1) * 1e3, 2),
        "mrmr_ms_per_call": round(mmed, 3), "mrmr_ms_min": round(min(tm), 3),
        "mrmr_ms_max": round(max(tm), 3),
        "mrmr_ms_upload": round(mup, 3), "mrmr_ms_pack": round(mpack, 3),
        "mrmr_ms_relevance": round(mrelv, 3), "mrmr_ms_rows": round(mrows, 3),
        "mrmr_ms_steps": round(msteps, 3),
        "mrmr_us_per_row_kernel": round(mrows / K * 1e3, 2),
        "mrmr_us_per_step_kernels": round(msteps / (K - 1) * 1e3, 2),
        "jmi_row_over_mi_row": round(rows / mrows, 3),
        "jmi_call_over_mrmr_call": round(med / mmed, 3),
        "joint_tables_computed": int(K * p), "rows_bytes": int(K * p * 8),
        "cpu_threads": cpu_threads, "cpu_ms_per_call": round(cmed, 3),
        "gpu_faster_than_cpu": bool(med < cmed),
        "same_selection_as_cpu": bool(np.array_equal(csel, sel)),
        "warmup": warmup, "reps": reps,
        "how": "host clock around synchronous calls, medians; breakdown from HIP events",
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", choices=sorted(SHAPES), action="append")
    ap.add_argument("--method", choices=["JMI", "CMIM"], default="JMI")
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
