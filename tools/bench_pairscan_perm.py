#!/usr/bin/env python
"""Time fs_pair_screen_labels (the pair screen's permutation test) on the GPU
(MI355X) against the route it replaces, B calls of fs_pair_screen(n_top=1).

One JSON line per shape:

* the batched call: host-clock median of the timed calls after warm-up (a call
  is synchronous: it uploads the codes and the labels, packs, computes the
  relevance of every labelling, scans, reduces on the device and downloads B
  results), and the medians of its five phases from HIP events on the call's
  stream (upload, pack, relevance, scan with the reduction, download);
* the baseline: the median of ``--base-calls`` fs_pair_screen(n_top=1) calls,
  each on one of the permuted labellings, multiplied by B -- an extrapolation,
  labelled as such, timed in the same process;
* whether those rows of the batch equal their single calls bit for bit;
* on the fast route (up to 4 states) the VALU lane operations the scan's word
  loop implies by DESIGN.md's MDR definition -- per pair, joint cell
  (kcol[i] x kcol[j]), 32-bit word and labelling: one AND and one popcount for
  each class but the last (loads, the wave-uniform plane work and the float64
  epilogue not counted) -- and their share of the VALU peak (256 CUs x 128
  lanes x 2.4 GHz) over the scan phase.

    python tools/bench_pairscan_perm.py
    python tools/bench_pairscan_perm.py --shape p500 --out profiles/pairscan_perm/bench.jsonl
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
    # name: (n, p, states, classes, B)
    "p50": (2000, 50, 3, 2, 1000),
    "p500": (2000, 500, 3, 2, 1000),
    "p2000": (2000, 2000, 3, 2, 1000),
    "general_p100_s10": (2000, 100, 10, 2, 100),
}
PEAK_LANE_OPS = 256 * 128 * 2.4e9
SCORE = "gain"


def make(n, p, states, classes, seed=0):
    """uint8 codes; y follows one planted pair with noise."""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, states, size=(n, p)).astype(np.uint8)
    y = (X[:, 1] + X[:, p - 2]) % classes
    y = np.where(rng.random(n) < 0.2, rng.integers(0, classes, n), y).astype(np.uint8)
    return X, y


def labellings(y, B, seed=0):
    """Row 0 is y; the others permute it, as PairScreen.permutation_test does."""
    rng = np.random.default_rng(seed)
    return np.stack([y] + [rng.permutation(y) for _ in range(B - 1)]).astype(np.uint8)


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
    from fastselect_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("bench_pairscan_perm: no HIP device visible")
    n, p, states, classes, B = SHAPES[name]
    S = max(states, classes)
    X, y = make(n, p, states, classes)
    lab = labellings(y, B)
    pairs = p * (p - 1) // 2
    out = {}

    ts, phases = timed(
        lambda: out.update(r=_lib.pair_screen_labels("gpu", X, lab, S, score=SCORE,
                                                     want_relevance=True)),
        warmup, reps, _lib.pair_labels_last_timing)
    med = statistics.median(ts)
    ph = [statistics.median(v[i] for v in phases) for i in range(5)]
    best, best_pairs, rel = out["r"]

    # the route this replaces: one fs_pair_screen(n_top=1) per labelling
    singles = {}
    rows = list(range(min(base_calls, B)))

    def one_pass():
        b = rows[one_pass.i % len(rows)]
        one_pass.i += 1
        singles[b] = _lib.pair_screen("gpu", X, lab[b], S, n_top=1, score=SCORE,
                                      want_feature_best=False)
    one_pass.i = 0
    bts, _ = timed(one_pass, 2, base_calls)
    bmed = statistics.median(bts)
    same = all(np.array_equal(best[b:b + 1], singles[b][1]) and
               np.array_equal(best_pairs[b:b + 1], singles[b][2]) and
               np.array_equal(rel[b], singles[b][0]) for b in singles)

    line = {
        "bench": "pair_screen_labels", "shape": name, "n": n, "p": p, "states": states,
        "classes": classes, "score": SCORE, "labelings": B, "pairs": pairs,
        "route": "fast" if S <= 4 else "general",
        "gpu_ms_per_call": round(med, 3), "gpu_ms_min": round(min(ts), 3),
        "gpu_ms_max": round(max(ts), 3),
        "event_ms_upload": round(ph[0], 3), "event_ms_pack": round(ph[1], 3),
        "event_ms_relevance": round(ph[2], 3), "event_ms_scan": round(ph[3], 3),
        "event_ms_download": round(ph[4], 3),
        "single_call_ms_median": round(bmed, 3), "single_calls": base_calls,
        "b_single_calls_ms_extrapolated": round(bmed * B, 1),
        "speedup_over_extrapolated": round(bmed * B / med, 2),
        "rows_checked": len(singles), "rows_equal_single_calls": bool(same),
        "best_pair": [int(v) for v in best_pairs[0]], "best_score": float(best[0]),
        "null_max": float(best[1:].max()),
        "warmup": warmup, "reps": reps,
    }
    if S <= 4:
        kcol = X.max(axis=0).astype(np.int64) + 1
        cells = (int(kcol.sum()) ** 2 - int((kcol ** 2).sum())) // 2   # sum over i < j of k_i k_j
        words = 4 * ((n + 127) // 128)      # whole quads of four 32-bit words
        ops = cells * words * 2 * (classes - 1) * B
        line.update({
            "words_per_plane": words, "valu_lane_ops": ops,
            "valu_roofline_ms": round(ops / PEAK_LANE_OPS * 1e3, 4),
            "valu_roofline_fraction_of_scan": round(ops / PEAK_LANE_OPS * 1e3 / ph[3], 4),
            "valu_roofline_fraction_of_call": round(ops / PEAK_LANE_OPS * 1e3 / med, 4),
        })
    return line


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
    for name in a.shape or ["p50", "p500", "p2000", "general_p100_s10"]:
        line = json.dumps(run(name, a.warmup, a.reps, a.base_calls))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
