#!/usr/bin/env python
"""Time the SURF / SURF* permutation test's batched call
(fs_plan_surf_score_labels, fs_surf_labels.hip) on the GPU (MI355X) beside what
a user did before it existed: one full score() per labelling.

One JSON line per (shape, variant): 2000 x 2000 with B = 1000 labellings and
bench.py's cfg2 (5000 x 5000) with B = 128, the same make_classification data,
each for SURF and SURF*.  Labelling 0 is y, the rest are permutations of it.

* ``labels_host_ms``: the host clock around one synchronous
  ``ResidentRows.score_labels`` with the (B, p) block downloaded; median of 7
  calls after 2 warm-ups.
* ``distance_records_ms`` / ``weights_ms`` / ``score_ms`` / ``star_ms``: HIP
  events of those calls (``fs_plan_surf_labels_kernel_ms`` 0..3: distances +
  resolve + records once per call; the weights kernels and the score kernel
  summed over the chunks of 32 labellings; the column sort once plus the star
  walk and its epilogue over the chunks, -1 for plain SURF), medians.
* ``score_host_ms``: the plan's plain ``score()`` in the same session, median
  of 20; ``b_scores_ms_extrapolated`` is that times B -- an extrapolation, not
  a measurement of B calls.
* ``row0_max_err_over_scale``: row 0 against ``score()``, over max |s|.

    python tools/bench_surf_perm.py
    python tools/bench_surf_perm.py --shape cfg2 --star 1 --out profiles/surf_perm/bench.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    # name: (n, p, redundant columns, labellings)
    "n2000": (2000, 2000, 100, 1000),
    "cfg2": (5000, 5000, 100, 128),
}


def make_data(n, p, red, seed=42):
    from sklearn.datasets import make_classification
    X, y = make_classification(n_samples=n, n_features=p, n_informative=20, n_redundant=red,
                               random_state=seed)
    return np.ascontiguousarray(X, dtype=np.float64), y


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run(name, star, calls, warmup, steps):
    import torch
    from fastselect_amd import SURF, _lib
    if _lib.device_count() < 1:
        raise SystemExit("bench_surf_perm.py needs a HIP device (no CPU fallback)")
    n, p, red, B = SHAPES[name]
    X, y = make_data(n, p, red)
    enc = np.unique(y, return_inverse=True)[1].astype(np.int32).reshape(-1)
    rng = np.random.default_rng(0)
    labels = np.stack([enc] + [rng.permutation(enc) for _ in range(B - 1)])
    scorer = SURF(backend="gpu", use_star=bool(star))._resident_scorer(X, y)
    try:
        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out

        scorer._sums(p)
        scorer._sums(p)
        t_score = []
        for _ in range(steps):
            ms, s = timed(lambda: scorer._sums(p))
            t_score.append(ms)
        t_lab, k = [], [[], [], [], []]
        first = None
        for c in range(warmup + calls):
            ms, out = timed(lambda: scorer.score_labels(labels))
            if first is None:
                first = out
            elif not np.array_equal(out, first):
                raise SystemExit("score_labels() is not repeatable")
            if c >= warmup:
                t_lab.append(ms)
                for w in range(4):
                    k[w].append(scorer.plan.surf_labels_kernel_ms(w))
        if not np.array_equal(scorer._sums(p), s):
            raise SystemExit("score() changed after score_labels()")
        info = scorer.plan.surf_labels_info()
        score_ms, lab_ms = statistics.median(t_score), statistics.median(t_lab)
        return {
            "tool": "bench_surf_perm", "shape": name, "n": n, "p": p, "use_star": int(bool(star)),
            "labellings": B, "calls": calls, "warmup": warmup, "steps": steps,
            "weighted_pairs": info[0], "near_sides": info[1], "chunks": info[2],
            "star_walk": info[3],
            "labels_host_ms": spread(t_lab), "distance_records_ms": spread(k[0]),
            "weights_ms": spread(k[1]), "score_ms": spread(k[2]), "star_ms": spread(k[3]),
            "score_host_ms": spread(t_score),
            "b_scores_ms_extrapolated": score_ms * B,
            "speedup_over_b_scores_extrapolated": score_ms * B / lab_ms,
            "labels_host_ms_per_labelling": lab_ms / B,
            "row0_max_err_over_scale": float(np.max(np.abs(first[0] - s)) / np.max(np.abs(s))),
        }
    finally:
        scorer.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shape", action="append", choices=sorted(SHAPES),
                    help="shape(s) to run (default: both)")
    ap.add_argument("--star", action="append", type=int, choices=[0, 1],
                    help="variant(s) to run: 0 SURF, 1 SURF* (default: both)")
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surf_perm",
                                                  "bench_surf_perm.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for name in args.shape or ["n2000", "cfg2"]:
            for star in args.star if args.star is not None else [0, 1]:
                line = json.dumps(run(name, star, args.calls, args.warmup, args.steps))
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()


if __name__ == "__main__":
    main()
