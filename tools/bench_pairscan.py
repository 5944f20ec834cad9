#!/usr/bin/env python
"""Time the all-pairs interaction screen (fs_pair_screen) on the GPU (MI355X)
beside the only other route to the same answer, and beside fs_mi_matrices.

One JSON line per shape.  A "call" is what PairScreen.fit hands to the native
library: one fs_pair_screen (upload, pack, relevance, the tiled scan with its
selection, a download of kilobytes) on codes that are already uint8; it is
synchronous, so the host clock around it covers device work that has finished.
The line holds the median call time, the fs_pair_screen_last_timing breakdown
(HIP events; the scan phase includes the host merges between its launches) and
the CPU backend's call on a slice of the columns, extrapolated by the pair
count (the work is one table per pair).

Two comparison points, alternating with the screen in the same session:

* the all-anchors route: fs_jmi_rows over all p anchors (p launches of
  k_jmi_row, every table twice, a p x p float64 matrix back) and the numpy
  selection on it (a stable argsort); it must give the same list;
* fs_mi_matrices on the same data: its scan phase is k_mi_scan, the kernel
  whose geometry k_pair_scan takes; the ratio of the two scan phases stands
  beside the class count C (k_pair_scan counts C masked words per word and runs
  k_jmi_row's serial three-way epilogue).

Kernel times proper come from one run of this tool under
``rocprofv3 --kernel-trace --stats`` on its own (no counters in that run).

The data: uniform columns, y = (x_a + x_b) mod classes for two columns a third
and two thirds along the width, 10 % of the labels moved to the next class.

    python tools/bench_pairscan.py                      # the three shapes
    python tools/bench_pairscan.py --shape geno3 --out profiles/pairscan/bench_pairscan.jsonl
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
    # name: (n, p, states, classes, cpu columns)
    "geno3": (2000, 5000, 3, 2, 400),
    "states10": (2000, 2000, 10, 2, 120),
    "states32": (2000, 500, 32, 4, 40),
}
N_TOP = 100
TOL = 1e-10


def make(n, p, states, classes, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.integers(0, states, size=(n, p)).astype(np.uint8)
    a, b = p // 3, 2 * p // 3
    y = (X[:, a].astype(np.int64) + X[:, b]) % classes
    y = np.where(rng.random(n) < 0.1, (y + 1) % classes, y)
    return X, y.astype(np.uint8), (a, b)


def select(J, rel, score, n_top):
    """The numpy selection of the all-anchors route: the score by the written
    expression over np.triu_indices (rank order), a stable argsort of its
    negation, and the per-feature maxima."""
    i, j = np.triu_indices(J.shape[0], 1)
    s = J[i, j] if score == "joint" else (J[i, j] - rel[i]) - rel[j]
    order = np.argsort(-s, kind="stable")[:n_top]
    best = np.full(J.shape[0], -np.inf)
    np.maximum.at(best, i, s)
    np.maximum.at(best, j, s)
    return s[order], np.stack([i[order], j[order]], axis=1), best


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def run(name, warmup, reps, cpu_threads, score, skip_baseline):
    from fastselect_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("bench_pairscan: no HIP device visible")
    n, p, states, classes, pc = SHAPES[name]
    X, y, planted = make(n, p, states, classes)
    total = p * (p - 1) // 2
    anchors = np.arange(p)

    def screen(backend="gpu", cols=X, n_jobs=-1):
        return _lib.pair_screen(backend, cols, y, states, n_top=N_TOP, score=score, n_jobs=n_jobs)

    def all_anchors():
        J = _lib.jmi_rows("gpu", X, y, states, anchors)
        _, rel, _ = _lib.jmi_select("gpu", X, y, states, 1, want_rows=False)
        return select(J, rel, score, N_TOP)

    def mi():
        return _lib.mi_matrices("gpu", X, y, states)

    ts, tb, tm, phases, mphases = [], [], [], [], []
    got = want = None
    for r in range(warmup + reps):   # alternating, the same session
        a, got = clock(screen)
        ph = _lib.pair_screen_last_timing()
        b = None
        if not skip_baseline:
            b, want = clock(all_anchors)
        c, _ = clock(mi)
        mph = _lib.mi_last_timing()
        if r >= warmup:
            ts.append(a)
            phases.append(ph)
            mphases.append(mph)
            tm.append(c)
            if b is not None:
                tb.append(b)
    up, pack, relv, scan, down = (statistics.median(v) for v in zip(*phases))
    mscan = statistics.median(v[2] for v in mphases)
    med = statistics.median(ts)
    same = None
    if want is not None:
        same = bool(np.array_equal(got[1], want[0]) and np.array_equal(got[2], want[1])
                    and np.array_equal(got[3], want[2]))
    lo, hi = min(planted), max(planted)
    line = {
        "bench": "pair_screen", "shape": name, "n": n, "p": p, "states": states,
        "classes": classes, "pairs": total, "n_top": N_TOP, "score": score,
        "gpu_ms_per_call": round(med, 3), "gpu_ms_min": round(min(ts), 3),
        "gpu_ms_max": round(max(ts), 3),
        "gpu_ms_upload": round(up, 3), "gpu_ms_pack": round(pack, 3),
        "gpu_ms_relevance": round(relv, 3), "gpu_ms_scan_and_selection": round(scan, 3),
        "gpu_ms_download": round(down, 3),
        "gpu_pairs_per_s": round(total / (med * 1e-3), 1),
        "top_pair": [int(v) for v in got[2][0]], "planted_pair": [lo, hi],
        "top_pair_is_planted": bool(got[2][0].tolist() == [lo, hi]),
        "mi_matrices_ms_per_call": round(statistics.median(tm), 3),
        "mi_scan_phase_ms": round(mscan, 3),
        "pair_scan_phase_over_mi_scan_phase": round(scan / mscan, 3) if mscan > 0 else None,
        "warmup": warmup, "reps": reps, "gpu_calls_of_each_kind": warmup + reps,
        "how": "host clock around synchronous calls, medians; breakdown from HIP events",
    }
    if not skip_baseline:
        # the CPU backend on a slice of the columns, extrapolated by the pair count
        Xc = np.ascontiguousarray(X[:, :pc])
        cts = [clock(lambda: screen("cpu", Xc, cpu_threads)) for _ in range(3)]
        cmed = statistics.median(t for t, _ in cts)
        err = float(np.abs(screen("gpu", Xc)[1] - cts[-1][1][1]).max())
        line.update({
            "cpu_threads": cpu_threads, "cpu_columns": pc, "cpu_pairs": pc * (pc - 1) // 2,
            "cpu_ms_measured_on_slice": round(cmed, 3),
            "cpu_ms_extrapolated": round(cmed * total / (pc * (pc - 1) // 2), 1),
            "cpu_column_is": "measured on the slice, extrapolated by the pair count",
            "gpu_cpu_max_abs_score_diff_on_slice": err,
            "gpu_agrees_with_cpu_on_slice": bool(err <= TOL),
        })
    if tb:
        bmed = statistics.median(tb)
        line.update({
            "all_anchors_ms_per_call": round(bmed, 3), "all_anchors_ms_min": round(min(tb), 3),
            "all_anchors_ms_max": round(max(tb), 3),
            "all_anchors_matrix_bytes": int(p) * int(p) * 8,
            "screen_over_all_anchors": round(med / bmed, 4),
            "screen_at_most_half_of_all_anchors": bool(med <= 0.5 * bmed),
            "same_list_as_all_anchors": same,
        })
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", choices=sorted(SHAPES), action="append")
    ap.add_argument("--score", choices=["gain", "joint"], default="gain")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--skip-baseline", action="store_true",
                    help="only the screen and fs_mi_matrices, each warmup + reps times: no "
                         "all-anchors route, no CPU slice (for a kernel-trace run)")
    ap.add_argument("--out", help="append the JSON lines to this file too")
    a = ap.parse_args()
    for name in a.shape or ["geno3", "states10", "states32"]:
        line = json.dumps(run(name, a.warmup, a.reps, a.cpu_threads, a.score, a.skip_baseline))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
