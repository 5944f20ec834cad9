#!/usr/bin/env python
"""Time RReliefF (fs_plan_score_targets on a one-class ReliefF plan) on the GPU
(MI355X) beside the score of a two-class ReliefF plan (fs_plan_score) of the
same shape, the two alternating in one session.

One JSON line per configuration: cfg3 (bench.py's ReliefF configuration,
20000 x 2000, k = 10) and 5000 x 5000, k = 10, the same make_classification
data as bench.py; the continuous target is a noisy linear form of the first
five columns.  Per round the host time of a score_targets() with B = 1 and of
a two-class score() (host clock around calls that end in a synchronise of the
plan's stream) and the HIP-event times of the selection
(fs_plan_targets_kernel_ms(0)) and of k_rrf_update (..(1)); then, in the same
session, rounds of B = 8 (one full chunk) and of B = 128.  The line holds the
medians and the extremes.

Derived figures, from the median times:

* the gather bandwidth of k_rrf_update per chunk: every neighbour of every
  focal row is one row of the float32 operands, so n * k * PW * 4 bytes (PW the
  padded feature width) over the kernel time of one chunk, at width 1 (B = 1)
  and at width 8 (B = 8);
* ``b128_over_128_b1_extrapolated``: the B = 128 call's host time over 128
  times the B = 1 call's.  The denominator is an extrapolation (128 separate
  calls were not run), the numerator is measured.

    python tools/bench_rrelieff.py
    python tools/bench_rrelieff.py --config cfg3 --rounds 20
"""
import argparse
import json
import os
import statistics
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
    rng = np.random.default_rng(seed)
    t = X[:, :5] @ rng.standard_normal(5) + 0.5 * rng.standard_normal(n)
    return X, y, t


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run(name, rounds, rounds_batch, warmup):
    import torch
    from fastselect_amd import _lib
    from fastselect_amd.ReliefF import relieff_inputs
    if _lib.device_count() < 1:
        raise SystemExit("bench_rrelieff.py needs a HIP device (no CPU fallback)")
    n, p, red, k = CONFIGS[name]
    X, y, t = make_data(n, p, red)
    x32, y_enc, recip, isd, probs = relieff_inputs(X, y, 10, "gpu", 0)
    rng = np.random.default_rng(1)
    targets = np.stack([t] + [rng.permutation(t) for _ in range(127)])
    two = _lib.RowsPlan("gpu", "relieff", x32, y_enc, recip, isd, k=k, class_probs=probs)
    one = _lib.RowsPlan("gpu", "relieff", x32, np.zeros(n, np.int32), recip, isd, k=k,
                        class_probs=np.ones(1, np.float32))
    try:
        sums = torch.empty(p, dtype=torch.float64, device="cuda")
        out = torch.empty(p + 128 * p + 128, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        p0 = out.data_ptr()

        def timed(fn):
            t0 = time.perf_counter()
            fn()  # synchronises the plan's stream before it returns
            return (time.perf_counter() - t0) * 1e3

        def score():
            two.score(sums.data_ptr())

        def score_targets(B):
            def call():
                one.score_targets(targets[:B], p0, p0 + 8 * p, p0 + 8 * (p + B * p))
            return call

        for _ in range(warmup):
            score()
            score_targets(1)()
        t_score, k_two, t_b1, k_sel, k_upd1 = [], [], [], [], []
        first = None
        for _ in range(rounds):
            t_score.append(timed(score))
            k_two.append(two.kernel_ms(1))
            t_b1.append(timed(score_targets(1)))
            k_sel.append(one.targets_kernel_ms(0))
            k_upd1.append(one.targets_kernel_ms(1))
            h = out[:2 * p].cpu()
            if first is not None and not torch.equal(h, first):
                raise SystemExit("score_targets() is not repeatable")
            first = h
        t_b8, k_upd8, t_b128, k_upd128 = [], [], [], []
        for _ in range(rounds_batch):
            t_b8.append(timed(score_targets(8)))
            k_upd8.append(one.targets_kernel_ms(1))
            t_b128.append(timed(score_targets(128)))
            k_upd128.append(one.targets_kernel_ms(1))
        if not torch.equal(out[:2 * p].cpu(), first):
            raise SystemExit("row 0 of the B = 128 call is not the B = 1 call")
        pw = (-(-int((~isd).sum()) // 64) + -(-int(isd.sum()) // 64)) * 64
        gather = n * k * pw * 4
        b1, b128 = statistics.median(t_b1), statistics.median(t_b128)
        return {
            "tool": "bench_rrelieff", "config": name, "n": n, "p": p, "k": k, "rounds": rounds,
            "rounds_batch": rounds_batch, "warmup": warmup,
            "relieff_two_class_score_host_ms": spread(t_score),
            "relieff_two_class_select_update_kernel_ms": spread(k_two),
            "b1_host_ms": spread(t_b1), "b1_selection_ms": spread(k_sel),
            "b1_update_kernel_ms": spread(k_upd1),
            "b1_over_relieff_score_host": b1 / statistics.median(t_score),
            "b8_host_ms": spread(t_b8), "b8_update_kernel_ms": spread(k_upd8),
            "b128_host_ms": spread(t_b128), "b128_update_kernel_ms": spread(k_upd128),
            "b128_update_kernel_ms_per_chunk_of_8": statistics.median(k_upd128) / 16,
            "extrapolated_128_b1_calls_host_ms": 128 * b1,
            "b128_over_128_b1_extrapolated": b128 / (128 * b1),
            "padded_width": pw, "gather_bytes_per_chunk": gather,
            "gather_GBps_width1": gather / (statistics.median(k_upd1) * 1e-3) / 1e9,
            "gather_GBps_width8": gather / (statistics.median(k_upd8) * 1e-3) / 1e9,
            "chunk_of_8_over_chunk_of_1": statistics.median(k_upd8) / statistics.median(k_upd1),
        }
    finally:
        one.close()
        two.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", action="append", choices=sorted(CONFIGS),
                    help="configuration(s) to run (default: both)")
    ap.add_argument("--rounds", type=int, default=20, help="alternating rounds of B = 1 / score")
    ap.add_argument("--rounds-batch", type=int, default=5, help="rounds of B = 8 and B = 128")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "rrelieff",
                                                  "bench_rrelieff.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for name in args.config or ["cfg3", "n5000-p5000"]:
            line = json.dumps(run(name, args.rounds, args.rounds_batch, args.warmup))
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    main()
