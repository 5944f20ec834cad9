#!/usr/bin/env python
"""Time fs_mdr_scan_top on the GPU (MI355X) against the plain fs_mdr_scan.

One JSON line per (shape, n_top): the shapes of tools/bench_mdr.py, n_top in
{1, 100, 4096}.  Each timed repetition calls the plain scan and then the top-N
scan on the same data, so both see the same device state; the figures are the
medians of the timed repetitions after warm-up (a call is synchronous: the host
clock around it covers device work that has finished).  ``ratio`` is top-N
over plain, ``plain_spread`` the plain scan's (max - min) / median in this
session, and ``phases_ms`` the top-N call's upload / pack / scan / download
from HIP events (fs_mdr_top_last_timing; "scan" holds both scans, the
threshold search between them and the selection).

    python tools/bench_mdr_top.py
    python tools/bench_mdr_top.py --shape pairs_cv10 --n-top 100 --reps 7
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_mdr import SHAPES, folds, make  # noqa: E402

N_TOPS = (1, 100, 4096)


def run(name, n_top, warmup, reps):
    from fastselect_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("bench_mdr_top: no HIP device visible")
    n, p, k, cv, _ = SHAPES[name]
    X, y = make(n, p, k)
    fold = folds(X, y, cv)
    case = y == 1
    plain, top, phases, out = [], [], [], {}
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        out["plain"] = _lib.mdr_scan("gpu", X, case, k, fold, cv)
        t1 = time.perf_counter()
        out["top"] = _lib.mdr_scan_top("gpu", X, case, k, fold, cv, n_top=n_top)
        t2 = time.perf_counter()
        if i >= warmup:
            plain.append((t1 - t0) * 1e3)
            top.append((t2 - t1) * 1e3)
            phases.append(_lib.mdr_top_last_timing())
    pm, tm = statistics.median(plain), statistics.median(top)
    same = bool(np.array_equal(out["top"][0][:, 0], out["plain"][0])
                and np.array_equal(out["top"][1][:, 0], out["plain"][1]))
    return {
        "bench": "mdr_scan_top", "shape": name, "n": n, "p": p, "k": k, "cv": cv, "n_top": n_top,
        "combinations": _lib.mdr_combinations(p, k),
        "plain_ms": round(pm, 3), "plain_ms_min": round(min(plain), 3),
        "plain_ms_max": round(max(plain), 3),
        "plain_spread": round((max(plain) - min(plain)) / pm, 4),
        "top_ms": round(tm, 3), "top_ms_min": round(min(top), 3), "top_ms_max": round(max(top), 3),
        "ratio": round(tm / pm, 3),
        "phases_ms": {name_: round(statistics.median(v), 3) for name_, v in
                      zip(("upload", "pack", "scan", "download"), zip(*phases))},
        "entry0_equals_plain": same,
        "gap_best_to_last": float(out["top"][0][0, 0] - out["top"][0][0, -1]),
        "warmup": warmup, "reps": reps,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", choices=sorted(SHAPES), action="append")
    ap.add_argument("--n-top", type=int, action="append")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", help="append the JSON lines to this file too")
    a = ap.parse_args()
    for name in a.shape or ["pairs_cv10", "pairs_nofold", "triples_cv10"]:
        for n_top in a.n_top or N_TOPS:
            line = json.dumps(run(name, n_top, a.warmup, a.reps))
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
