#!/usr/bin/env python
"""Time fs_mdr_scan on the GPU (MI355X) and the CPU backend.

One JSON line per shape: shape, k, cv, combinations, milliseconds per scan
(median of the timed calls after warm-up; a call is synchronous -- it uploads
X, packs the bit-planes, scans and returns the folds' best models, so the host
clock around it covers device work that has finished), combinations per
second, the VALU lane operations the scan kernel's inner loop implies and
their share of the VALU peak (256 CUs x 128 lanes x 2.4 GHz), and the CPU
backend's time.  The CPU time is measured with 16 threads on the first
columns only (the last entry of a SHAPES row) and scaled by the ratio of combination counts:
an extrapolation, labelled as such.

    python tools/bench_mdr.py                 # the three shapes + the no-fold pair
    python tools/bench_mdr.py --shape pairs_cv10 --reps 7
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
    # name: (n, p, k, cv, cpu columns)
    "pairs_cv10": (2000, 5000, 2, 10, 1500),
    "triples_cv10": (2000, 500, 3, 10, 120),
    "pairs_nofold": (2000, 5000, 2, 0, 1500),
}
PEAK_LANE_OPS = 256 * 128 * 2.4e9


def make(n, p, k, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 3, size=(n, p)).astype(np.uint8)
    y = (rng.random(n) < np.where((X[:, 1] == X[:, p - 2]), 0.8, 0.2)).astype(np.uint8)
    return X, y


def folds(X, y, cv):
    if not cv:
        return None
    from sklearn.model_selection import StratifiedKFold
    fold = np.empty(X.shape[0], dtype=np.int32)
    for i, (_, te) in enumerate(StratifiedKFold(cv, shuffle=True, random_state=42).split(X, y)):
        fold[te] = i
    return fold


def words(y, fold, cv, bits=32):
    """Words per plane of the segment layout: every (class, fold) segment
    padded to whole words."""
    f = np.zeros(len(y), dtype=np.int64) if fold is None else fold
    return sum(-(-int(np.sum((y == c) & (f == i))) // bits)
               for c in (0, 1) for i in range(max(cv, 1)))


def lane_ops(count, k, w, cv):
    """Per combination, cell of the first k-1 columns and word: k-1 ANDs for
    the prefix, 3 ANDs and 3 popcount-accumulates for the last column's
    genotypes (loads, the per-cell decisions and the epilogue not counted).
    More than 16 folds run in groups that each walk every word."""
    groups = max(1, -(-cv // 16))
    return count * 3 ** (k - 1) * w * (k + 5) * groups


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def run(name, warmup, reps, cpu_threads):
    from fastselect_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("bench_mdr: no HIP device visible")
    n, p, k, cv, pc = SHAPES[name]
    X, y = make(n, p, k)
    fold = folds(X, y, cv)
    count = _lib.mdr_combinations(p, k)
    out = {}
    med, lo, hi = timed(lambda: out.update(r=_lib.mdr_scan("gpu", X, y == 1, k, fold, cv)),
                        warmup, reps)
    Xc = np.ascontiguousarray(X[:, :pc])
    cc = _lib.mdr_combinations(pc, k)
    cmed, _, _ = timed(lambda: out.update(c=_lib.mdr_scan("cpu", Xc, y == 1, k, fold, cv,
                                                          n_jobs=cpu_threads)), 1, 3)
    gc = _lib.mdr_scan("gpu", Xc, y == 1, k, fold, cv)
    same = bool(np.array_equal(gc[0], out["c"][0]) and np.array_equal(gc[1], out["c"][1]))
    w = words(y, fold, cv)
    ops = lane_ops(count, k, w, cv)
    return {
        "bench": "mdr_scan", "shape": name, "n": n, "p": p, "k": k, "cv": cv,
        "combinations": count, "words_per_plane": w,
        "gpu_ms_per_scan": round(med, 3), "gpu_ms_min": round(lo, 3), "gpu_ms_max": round(hi, 3),
        "gpu_combinations_per_s": round(count / (med * 1e-3), 1),
        "valu_lane_ops": ops, "valu_roofline_ms": round(ops / PEAK_LANE_OPS * 1e3, 4),
        "valu_roofline_fraction_of_call": round(ops / PEAK_LANE_OPS * 1e3 / med, 4),
        "cpu_threads": cpu_threads, "cpu_columns": pc, "cpu_combinations": cc,
        "cpu_ms_measured_on_slice": round(cmed, 3),
        "cpu_ms_extrapolated": round(cmed * count / cc, 1),
        "gpu_equals_cpu_on_slice": same,
        "best_rank_fold0": int(out["r"][1][0]),
        "best_combination_fold0": list(_lib.mdr_unrank(p, k, int(out["r"][1][0]))),
        "warmup": warmup, "reps": reps,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", choices=sorted(SHAPES), action="append")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--out", help="append the JSON lines to this file too")
    a = ap.parse_args()
    for name in a.shape or ["pairs_cv10", "triples_cv10", "pairs_nofold"]:
        line = json.dumps(run(name, a.warmup, a.reps, a.cpu_threads))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
