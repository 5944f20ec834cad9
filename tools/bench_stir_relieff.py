#!/usr/bin/env python
"""Time STIR for ReliefF (fs_plan_score_stir) on the GPU (MI355X) beside the
plain score (fs_plan_score) of the same resident plan, score() and
score_stir() alternating in one session.

One JSON line per configuration: cfg3 (bench.py's ReliefF configuration,
20000 x 2000, k = 10) and 5000 x 5000, k = 10, the same make_classification
data as bench.py.  Per round the host time of a score() and of a score_stir()
(host clock around calls that end in a synchronise of the plan's stream), the
HIP-event time of the selection + update (fs_plan_kernel_ms(1)) and of
k_rf_stir (fs_plan_stir_kernel_ms(2)); the line holds the medians and the
extremes.

Derived figures, from the median kernel time:

* the gather bandwidth of k_rf_stir: every neighbour of every focal row is one
  row of the float32 operands, PW * 4 bytes (PW the padded feature width), so
  (|H| + |M|) * PW * 4 bytes over the kernel time;
* pair-features per second: (|H| + |M|) * p over the kernel time.

--parent-root DIR names a checkout of the parent commit with its library
built: a child process times that checkout's score() on the same data in the
same session (interleaving is not possible across two libraries; the child
runs right after this process's rounds), and the line carries the ratios of
score() and score_stir() to it.

    python tools/bench_stir_relieff.py
    python tools/bench_stir_relieff.py --config cfg3 --parent-root ../parent
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIGS = {
    # name: (n, p, redundant columns, k)   (cfg3: bench.py CONFIGS)
    "cfg3": (20000, 2000, 50, 10),
    "n5000-p5000": (5000, 5000, 100, 10),
}


def make_data(n, p, red, seed=42):
    from sklearn.datasets import make_classification
    X, y = make_classification(n_samples=n, n_features=p, n_informative=20, n_redundant=red,
                               random_state=seed)
    return X, y


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run(name, rounds, warmup, score_only):
    import torch
    from fastselect_amd import _lib
    from fastselect_amd.ReliefF import relieff_inputs
    if _lib.device_count() < 1:
        raise SystemExit("bench_stir_relieff.py needs a HIP device (no CPU fallback)")
    n, p, red, k = CONFIGS[name]
    X, y = make_data(n, p, red)
    x32, y_enc, recip, isd, probs = relieff_inputs(X, y, 10, "gpu", 0)
    plan = _lib.RowsPlan("gpu", "relieff", x32, y_enc, recip, isd, k=k, class_probs=probs)
    try:
        sums = torch.empty(p, dtype=torch.float64, device="cuda")
        sums2 = torch.empty(p, dtype=torch.float64, device="cuda")
        stir = torch.empty(4 * p, dtype=torch.float64, device="cuda")
        counts = torch.empty(2, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

        def timed(fn):
            t0 = time.perf_counter()
            fn()  # synchronises the plan's stream before it returns
            return (time.perf_counter() - t0) * 1e3

        def score():
            plan.score(sums.data_ptr())

        def score_stir():
            plan.score_stir(sums2.data_ptr(), stir.data_ptr(), counts.data_ptr())

        for _ in range(warmup):
            score()
            if not score_only:
                score_stir()
        t_score, t_stir, k_sel, k_sel_stir, k_stir = [], [], [], [], []
        first = last_stir = None
        for _ in range(rounds):
            t_score.append(timed(score))
            k_sel.append(plan.kernel_ms(1))
            s = sums.cpu()
            if first is not None and not torch.equal(s, first):
                raise SystemExit("score() is not repeatable")
            first = s
            if score_only:
                continue
            t_stir.append(timed(score_stir))
            k_sel_stir.append(plan.kernel_ms(1))
            k_stir.append(plan.stir_kernel_ms(2))
            if not torch.equal(sums2.cpu(), first):
                raise SystemExit("score_stir()'s score sums are not score()'s")
            st = stir.cpu()
            if last_stir is not None and not torch.equal(st, last_stir):
                raise SystemExit("score_stir() is not repeatable")
            last_stir = st
        out = {"tool": "bench_stir_relieff", "config": name, "n": n, "p": p, "k": k,
               "rounds": rounds, "warmup": warmup, "score_host_ms": spread(t_score),
               "select_update_kernel_ms": spread(k_sel)}
        if score_only:
            return out
        nh, nm = (int(v) for v in counts.cpu().tolist())
        pw = (-(-int((~isd).sum()) // 64) + -(-int(isd.sum()) // 64)) * 64
        stir_s = statistics.median(k_stir) * 1e-3
        _, _, t, _ = _lib.stir_statistics(last_stir.numpy().reshape(4, p), nh, nm)
        out.update({
            "score_stir_host_ms": spread(t_stir),
            "select_update_kernel_ms_in_score_stir": spread(k_sel_stir),
            "rf_stir_kernel_ms": spread(k_stir),
            "score_stir_over_score_host": statistics.median(t_stir) / statistics.median(t_score),
            "rf_stir_over_score_host": statistics.median(k_stir) / statistics.median(t_score),
            "n_hit_pairs": nh, "n_miss_pairs": nm, "padded_width": pw,
            "gather_bytes": (nh + nm) * pw * 4,
            "gather_GBps": (nh + nm) * pw * 4 / stir_s / 1e9,
            "pair_features_per_s": (nh + nm) * p / stir_s,
            "features_with_t_above_5": int((t > 5).sum()),
        })
        return out
    finally:
        plan.close()


def parent_score(root, name, rounds, warmup):
    """score() of the checkout at ``root`` (its own library), in a child process."""
    cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--score-only", "--config",
           name, "--rounds", str(rounds), "--warmup", str(warmup), "--out", os.devnull]
    res = subprocess.run(cmd, check=True, capture_output=True, text=True)
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", action="append", choices=sorted(CONFIGS),
                    help="configuration(s) to run (default: both)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--root", default=HERE, help="checkout whose fastselect_amd is timed")
    ap.add_argument("--score-only", action="store_true", help="time score() alone")
    ap.add_argument("--parent-root", default=None,
                    help="a built checkout of the parent commit to time score() of")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "stir_relieff",
                                                  "bench_stir_relieff.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for name in args.config or ["cfg3", "n5000-p5000"]:
            res = run(name, args.rounds, args.warmup, args.score_only)
            if args.parent_root:
                par = parent_score(args.parent_root, name, args.rounds, args.warmup)
                base = par["score_host_ms"]["median"]
                res["parent_score_host_ms"] = par["score_host_ms"]
                res["parent_select_update_kernel_ms"] = par["select_update_kernel_ms"]
                res["score_over_parent_score"] = res["score_host_ms"]["median"] / base
                res["score_stir_over_parent_score"] = res["score_stir_host_ms"]["median"] / base
            line = json.dumps(res)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    main()
