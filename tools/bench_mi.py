#!/usr/bin/env python
"""Time fs_mi_matrices on the GPU (MI355X) and the CPU backend.

One JSON line per shape: shape, states, pairs, milliseconds per call (median
of the timed calls after warm-up; a call is synchronous -- it uploads the
codes, packs the bit-planes, scans every pair and downloads the p x p matrix,
so the host clock around it covers device work that has finished), the call's
phases from HIP events (upload, pack, scan, download), the VALU lane
operations the scan kernel's inner loop implies and their share of the VALU
peak (256 CUs x 128 lanes x 2.4 GHz, the convention of tools/bench_mdr.py)
over the scan phase and over the whole call, and the CPU backend's time.  The
CPU time is measured with 16 threads on the first columns only (the last entry
of a SHAPES row) and scaled by the ratio of pair counts: an extrapolation,
labelled as such.  On that slice the two backends' tables must be equal and
their mutual information within 1e-10.

    python tools/bench_mi.py                  # the three shapes
    python tools/bench_mi.py --shape geno3 --out profiles/mi/bench_mi.jsonl
    python tools/bench_mi.py --n 8000         # four times the words: the scan's cost per word
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
    # name: (n, p, states, cpu columns)
    "geno3": (2000, 5000, 3, 1000),
    "states10": (2000, 2000, 10, 400),
    "states32": (2000, 500, 32, 120),
}
PEAK_LANE_OPS = 256 * 128 * 2.4e9
TOL = 1e-10


def make(n, p, states, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.integers(0, states, size=(n, p)).astype(np.uint8)
    y = np.where(rng.random(n) < 0.7, X[:, 1] % 3, rng.integers(0, 3, size=n)).astype(np.uint8)
    return X, y


def pairs(p):
    """Column pairs i < j plus every column with y."""
    return p * (p - 1) // 2 + p


def lane_ops(p, n, states):
    """Per pair and 32-sample word: ceil(states / 4)^2 lanes, each with 16
    ANDs and 16 popcount-accumulates for its 4 x 4 block of the table (LDS
    reads, staging, idle lanes of ragged tiles and the epilogue not
    counted)."""
    nb = -(-states // 4)
    return pairs(p) * nb * nb * (-(-n // 32)) * 32


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
    return statistics.median(ts), min(ts), max(ts), extra


def run(name, warmup, reps, cpu_threads, n_override=None):
    from fastselect_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("bench_mi: no HIP device visible")
    n, p, states, pc = SHAPES[name]
    n = n_override or n
    X, y = make(n, p, states)
    out = {}
    med, lo, hi, phases = timed(lambda: out.update(g=_lib.mi_matrices("gpu", X, y, states)),
                                warmup, reps, _lib.mi_last_timing)
    up, pack, scan, down = (statistics.median(v) for v in zip(*phases))
    Xc = np.ascontiguousarray(X[:, :pc])
    cmed, _, _, _ = timed(lambda: out.update(c=_lib.mi_matrices("cpu", Xc, y, states,
                                                                n_jobs=cpu_threads)), 1, 3)
    gs = _lib.mi_matrices("gpu", Xc, y, states, want_counts=True)
    cs = _lib.mi_matrices("cpu", Xc, y, states, n_jobs=cpu_threads, want_counts=True)
    counts_equal = bool(np.array_equal(gs[2], cs[2]))
    mi_err = float(max(np.abs(gs[0] - cs[0]).max(), np.abs(gs[1] - cs[1]).max()))
    ops = lane_ops(p, n, states)
    roof_ms = ops / PEAK_LANE_OPS * 1e3
    cpu_ms = cmed * pairs(p) / pairs(pc)
    return {
        "bench": "mi_matrices", "shape": name, "n": n, "p": p, "states": states,
        "pairs": pairs(p), "words_per_plane": -(-n // 32),
        "gpu_ms_per_call": round(med, 3), "gpu_ms_min": round(lo, 3), "gpu_ms_max": round(hi, 3),
        "gpu_ms_upload": round(up, 3), "gpu_ms_pack": round(pack, 3),
        "gpu_ms_scan": round(scan, 3), "gpu_ms_download": round(down, 3),
        "gpu_pairs_per_s": round(pairs(p) / (med * 1e-3), 1),
        "valu_lane_ops": ops, "valu_roofline_ms": round(roof_ms, 4),
        "valu_roofline_fraction_of_scan": round(roof_ms / scan, 4) if scan > 0 else None,
        "valu_roofline_fraction_of_call": round(roof_ms / med, 5),
        "cpu_threads": cpu_threads, "cpu_columns": pc, "cpu_pairs": pairs(pc),
        "cpu_ms_measured_on_slice": round(cmed, 3),
        "cpu_ms_extrapolated": round(cpu_ms, 1),
        "gpu_faster_than_cpu_extrapolated": bool(med < cpu_ms),
        "counts_equal_on_slice": counts_equal, "mi_max_abs_diff_on_slice": mi_err,
        "gpu_agrees_with_cpu_on_slice": bool(counts_equal and mi_err <= TOL),
        "warmup": warmup, "reps": reps,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", choices=sorted(SHAPES), action="append")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--n", type=int, help="samples instead of the shape's own (the scan's "
                    "time per word is the slope between two sample counts)")
    ap.add_argument("--out", help="append the JSON lines to this file too")
    a = ap.parse_args()
    for name in a.shape or ["geno3", "states10", "states32"]:
        line = json.dumps(run(name, a.warmup, a.reps, a.cpu_threads, a.n))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
