#!/usr/bin/env python
"""Time fs_mdr_scan_labels (the MDR permutation test) on the GPU (MI355X)
against the route it replaces, B calls of fs_mdr_scan.

One JSON line per shape:

* the batched call: host-clock median of the timed calls after warm-up (a call
  is synchronous: it uploads X and the labels, packs, scans, reduces on the
  device and downloads B x F results), and the medians of its phases from HIP
  events on the call's stream (upload, pack, scan with the reduction,
  download);
* the baseline: the median of ``--base-calls`` fs_mdr_scan calls, each on one
  of the permuted labellings, multiplied by B -- an extrapolation, labelled as
  such, timed in the same process;
* the VALU lane operations the scan's word loop implies by DESIGN.md's MDR
  definition -- per combination, prefix cell, 32-bit word and labelling: 3
  ANDs and 3 popcounts in the lane (loads, the wave-uniform plane work, the
  per-cell decisions and the BA epilogue not counted) -- and their share of
  the VALU peak (256 CUs x 128 lanes x 2.4 GHz) over the scan phase;
* the Python side of MDR.permutation_test: the per-labelling fold summaries,
  timed on their own, and the whole method.

    python tools/bench_mdr_perm.py
    python tools/bench_mdr_perm.py --shape pairs_p50 --reps 7 --out profiles/mdr_perm/bench.jsonl
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
    # name: (n, p, k, cv, B)
    "pairs_p50": (2000, 50, 2, 10, 1000),
    "triples_p50": (2000, 50, 3, 10, 1000),
    "pairs_p500": (2000, 500, 2, 10, 1000),
}
PEAK_LANE_OPS = 256 * 128 * 2.4e9


def make(n, p, seed=0):
    """uint8 genotypes; the phenotype follows one planted pair with noise."""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 3, size=(n, p)).astype(np.uint8)
    y = (rng.random(n) < np.where((X[:, 1] == X[:, p - 2]), 0.8, 0.2)).astype(np.uint8)
    return X, y


def folds(X, y, cv):
    from sklearn.model_selection import StratifiedKFold
    splits = list(StratifiedKFold(cv, shuffle=True, random_state=42).split(X, y))
    fold = np.empty(X.shape[0], dtype=np.int32)
    for i, (_, te) in enumerate(splits):
        fold[te] = i
    return fold, splits


def labellings(y, splits, B, seed=0):
    """Row 0 is the phenotype; the others permute it within each fold, as
    MDR.permutation_test does."""
    rng = np.random.default_rng(seed)
    lab = np.empty((B, len(y)), dtype=np.uint8)
    lab[0] = y == 1
    for b in range(1, B):
        for _, te in splits:
            lab[b, te] = rng.permutation(lab[0, te])
    return lab


def quad_words(fold, cv):
    """32-bit words per plane of the labels layout: every fold's segment
    padded to whole quads of four words (128 samples)."""
    return 4 * sum(-(-int(np.sum(fold == i)) // 128) for i in range(cv))


def timed(fn, warmup, reps, after=None):
    for _ in range(warmup):
        fn()
    ts, extra = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
        if after:
            extra.append(after())
    return ts, extra


def run(name, warmup, reps, base_calls):
    from fastselect_amd import MDR, _lib
    from fastselect_amd.MDR import summarise_folds
    if _lib.device_count() < 1:
        raise SystemExit("bench_mdr_perm: no HIP device visible")
    n, p, k, cv, B = SHAPES[name]
    X, y = make(n, p)
    fold, splits = folds(X, y, cv)
    lab = labellings(y, splits, B)
    count = _lib.mdr_combinations(p, k)
    out = {}

    ts, phases = timed(lambda: out.update(r=_lib.mdr_scan_labels("gpu", X, lab, k, fold, cv)),
                       warmup, reps, _lib.mdr_labels_last_timing)
    med = statistics.median(ts)
    ph = [statistics.median(v[i] for v in phases) for i in range(4)]
    best_ba, best_rank = out["r"]

    # the route this replaces: one fs_mdr_scan per labelling
    singles = {}
    rows = list(range(base_calls))

    def one_pass():
        b = rows[one_pass.i % len(rows)]
        one_pass.i += 1
        singles[b] = _lib.mdr_scan("gpu", X, lab[b], k, fold, cv)
    one_pass.i = 0
    bts, _ = timed(one_pass, 2, base_calls)
    bmed = statistics.median(bts)
    same = all(np.array_equal(best_ba[b].view(np.uint32), singles[b][0].view(np.uint32)) and
               np.array_equal(best_rank[b], singles[b][1]) for b in singles)

    w = quad_words(fold, cv)
    ops = count * 3 ** (k - 1) * w * 6 * B

    t0 = time.perf_counter()
    for b in range(B):
        summarise_folds(X, lab[b], splits, best_rank[b], k)
    summary_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    est = MDR(k=k, cv=cv, backend="gpu").permutation_test(X, y, B - 1, random_state=0)
    method_ms = (time.perf_counter() - t0) * 1e3

    return {
        "bench": "mdr_scan_labels", "shape": name, "n": n, "p": p, "k": k, "cv": cv,
        "labelings": B, "combinations": count, "words_per_plane": w,
        "gpu_ms_per_call": round(med, 3), "gpu_ms_min": round(min(ts), 3),
        "gpu_ms_max": round(max(ts), 3),
        "event_ms_upload": round(ph[0], 3), "event_ms_pack": round(ph[1], 3),
        "event_ms_scan": round(ph[2], 3), "event_ms_download": round(ph[3], 3),
        "single_scan_ms_median": round(bmed, 3), "single_scan_calls": base_calls,
        "b_single_scans_ms_extrapolated": round(bmed * B, 1),
        "speedup_over_extrapolated": round(bmed * B / med, 2),
        "rows_equal_single_scans": bool(same),
        "valu_lane_ops": ops, "valu_roofline_ms": round(ops / PEAK_LANE_OPS * 1e3, 4),
        "valu_roofline_fraction_of_scan": round(ops / PEAK_LANE_OPS * 1e3 / ph[2], 4),
        "valu_roofline_fraction_of_call": round(ops / PEAK_LANE_OPS * 1e3 / med, 4),
        "host_summary_ms": round(summary_ms, 1), "permutation_test_ms": round(method_ms, 1),
        "p_value": est.p_value_, "best_interaction": list(est.best_interaction_),
        "warmup": warmup, "reps": reps,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", choices=sorted(SHAPES), action="append")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--base-calls", type=int, default=20)
    ap.add_argument("--out", help="append the JSON lines to this file too")
    a = ap.parse_args()
    if a.base_calls < 20:
        ap.error("--base-calls must be at least 20")
    for name in a.shape or ["pairs_p50", "triples_p50", "pairs_p500"]:
        line = json.dumps(run(name, a.warmup, a.reps, a.base_calls))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
