#!/usr/bin/env python
"""Time the ReliefF permutation test's batched call
(fs_plan_relieff_score_labels, fs_relieff_labels.hip) on the GPU (MI355X)
beside what a user did before it existed: one full scoring call per labelling.

One JSON line per shape: 2000 x 2000 with B = 1000 labellings, 5000 x 5000
with B = 128 and bench.py's cfg3 (20000 x 2000) with B = 128, all with k = 10,
the same make_classification data; and ``ties`` (5000 x 200 columns of
integers in {0, 1, 2}, B = 128), where every row's keys tie and the candidate
prefix pays the quicksort replay on every row.  Labelling 0 is y, the rest are
permutations of it.

* ``auto`` / ``general`` / ``fast``: the same ``RowsPlan.score_labels`` call
  (device output, not downloaded) on the automatic route, with the
  ``rf_labels_route = 1`` test hook, and with ``rf_labels_depth`` set to the
  depth the rule computes (which takes the fast route whatever the rule's
  floor and cost estimate say), in the same session, alternating; per route ``host_ms`` (the host clock around the synchronous call, median of
  ``--calls`` after ``--warmup``), ``kernel_ms`` (the medians of
  ``fs_plan_relieff_labels_kernel_ms`` 0..3: candidate prefix once per call,
  walk and weights, score kernel, general-route kernels) and ``info``
  (``fs_plan_relieff_labels_info``: fast, general, overflow reruns, depth).
* ``rule_picks``: the route of the automatic call, read from its ``info``;
  ``faster_route``: the smaller of the ``general`` and ``fast`` medians;
  ``auto_picks_faster``: they agree, or the two medians are within 2% of each
  other (a tie at the repeatability of these calls).
* ``score_host_ms``: ``RowsPlan.score()`` of the same plan in the same
  session, median of ``--steps`` (20) calls; ``b_scores_ms_extrapolated`` is
  that times B -- an extrapolation, not a measurement of B calls.
* ``fast_vs_general_max_over_scale``: the largest difference between the two
  routes' rows over max |row 0|; ``row0_general_equals_score``: the general
  route's row 0 has the bits of the plan's own score.

    python tools/bench_relieff_perm.py
    python tools/bench_relieff_perm.py --shape cfg3 --out profiles/relieff_perm/bench.jsonl
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
    # name: (n, p, redundant columns, k, labellings)   (cfg3: bench.py CONFIGS)
    "n2000": (2000, 2000, 100, 10, 1000),
    "n5000-p5000": (5000, 5000, 100, 10, 128),
    "cfg3": (20000, 2000, 50, 10, 128),
    "ties": (5000, 200, 0, 10, 128),
}


def make_data(n, p, red, seed=42):
    if red == 0:  # the tie-heavy shape: small integers, y from two columns
        rng = np.random.default_rng(seed)
        X = rng.integers(0, 3, size=(n, p)).astype(np.float64)
        return X, (X[:, 3] + X[:, 5] + rng.standard_normal(n) > 2.0).astype(np.int64)
    from sklearn.datasets import make_classification
    return make_classification(n_samples=n, n_features=p, n_informative=20, n_redundant=red,
                               random_state=seed)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run(name, calls, warmup, steps):
    import torch
    from fastselect_amd import _lib
    from fastselect_amd.ReliefF import relieff_inputs
    if _lib.device_count() < 1:
        raise SystemExit("bench_relieff_perm.py needs a HIP device (no CPU fallback)")
    n, p, red, k, B = SHAPES[name]
    X, y = make_data(n, p, red)
    x32, y_enc, recip, isd, probs = relieff_inputs(X, y, 10, "gpu", 0)
    rng = np.random.default_rng(0)
    labels = np.stack([y_enc] + [rng.permutation(y_enc) for _ in range(B - 1)]).astype(np.int32)
    plan = _lib.RowsPlan("gpu", "relieff", x32, y_enc, recip, isd, k=k, class_probs=probs)
    try:
        sums = torch.empty(p, dtype=torch.float64, device="cuda")
        out = torch.empty(B * p, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

        def timed(fn):
            t0 = time.perf_counter()
            fn()  # synchronises the plan's stream before it returns
            return (time.perf_counter() - t0) * 1e3

        for _ in range(2):
            plan.score(sums.data_ptr())
        t_score, k_p1, k_su = [], [], []
        for _ in range(steps):
            t_score.append(timed(lambda: plan.score(sums.data_ptr())))
            k_p1.append(plan.kernel_ms(0))
            k_su.append(plan.kernel_ms(1))
        own = sums.cpu()
        # the rule's depth: the smallest of 64 / 128 / 256 covering
        # min(ceil(3 k / smallest class share), n - 1)
        need = min(-(-3 * k * n // int(np.bincount(y_enc).min())), n - 1)
        depth = 64 if need <= 64 else 128 if need <= 128 else 256
        routes = {"auto": {}, "general": {"rf_labels_route": 1},
                  "fast": {"rf_labels_depth": depth}}
        t_lab = {r: [] for r in routes}
        kms = {r: [[] for _ in range(4)] for r in routes}
        first, info = {}, {}
        for c in range(warmup + calls):
            for r, hooks in routes.items():
                with _lib.test_hooks(**hooks):
                    ms = timed(lambda: plan.score_labels(labels, out.data_ptr()))
                rows = out.cpu()
                if r not in first:
                    first[r] = rows
                elif not torch.equal(rows, first[r]):
                    raise SystemExit(f"score_labels() ({r}) is not repeatable")
                info[r] = plan.labels_info()
                if c >= warmup:
                    t_lab[r].append(ms)
                    for w in range(4):
                        kms[r][w].append(plan.labels_kernel_ms(w))
        plan.score(sums.data_ptr())
        if not torch.equal(sums.cpu(), own):
            raise SystemExit("score() changed after score_labels()")
        score_ms = statistics.median(t_score)
        med = {r: statistics.median(t_lab[r]) for r in routes}
        fa = first["fast"].numpy().reshape(B, p)
        ge = first["general"].numpy().reshape(B, p)
        res = {
            "tool": "bench_relieff_perm", "shape": name, "n": n, "p": p, "k": k,
            "labellings": B, "calls": calls, "warmup": warmup, "steps": steps,
            "score_host_ms": spread(t_score), "pass1_kernel_ms": spread(k_p1),
            "select_update_kernel_ms": spread(k_su),
            "b_scores_ms_extrapolated": score_ms * B,
            "rule_picks": "fast" if info["auto"][0] > 0 else "general",
            "faster_route": "fast" if med["fast"] < med["general"] else "general",
            "fast_over_general": med["fast"] / med["general"],
            "auto_over_general": med["auto"] / med["general"],
            "speedup_over_b_scores_extrapolated": score_ms * B / med["auto"],
            "fast_vs_general_max_over_scale": float(np.max(np.abs(fa - ge))
                                                    / np.max(np.abs(ge[0]))),
            "row0_general_equals_score": bool(np.array_equal(ge[0], own.numpy())),
            "null_max_over_observed_max": float(ge[1:].max() / ge[0].max()),
        }
        res["auto_picks_faster"] = bool(res["rule_picks"] == res["faster_route"]
                                        or abs(res["fast_over_general"] - 1.0) <= 0.02)
        for r in routes:
            res[r] = {"host_ms": spread(t_lab[r]), "info": list(info[r]),
                      "kernel_ms": [statistics.median(v) for v in kms[r]],
                      "host_ms_per_labelling": med[r] / B}
        return res
    finally:
        plan.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shape", action="append", choices=sorted(SHAPES),
                    help="shape(s) to run (default: all four)")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relieff_perm",
                                                  "bench_relieff_perm.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for name in args.shape or ["n2000", "n5000-p5000", "cfg3", "ties"]:
            line = json.dumps(run(name, args.calls, args.warmup, args.steps))
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    main()
