#!/usr/bin/env python
"""Time the STIR stage (fs_plan_stir) on the GPU (MI355X) beside pass 2 of the
same plan, step() and stir() alternating in one session.

One JSON line per configuration (bench.py's cfg2: MultiSURF 5000 x 5000, cfg4:
20000 x 20000, the same make_classification data).  Per round the host time of
a step() and of a stir() (host clock around work that ends in a device
synchronise), the HIP-event time of pass 2's score kernels
(fs_plan_kernel_ms(1)) and of the two STIR kernels (fs_plan_stir_kernel_ms:
k_stir_weights and k_stir_score, summed over the stage's chunks of tiles); the
line holds the medians and the extremes.

Derived figures, from the median kernel times:

* near pair sides x features per second: (|H| + |M|) p / k_stir_score time --
  the useful work;
* the dense walk's rate: every pair of every owned tile (128 x 128 a tile, the
  lower halves of diagonal tiles and the padding rows included) x the padded
  feature width, times the VALU instructions k_stir_score issues per
  pair-feature (7 for a continuous feature: subtract, two fixed-point
  conversions, four multiply-adds; 4 for a discrete one), over the chip's VALU
  issue peak (256 CUs x 4 SIMDs x 32
  lanes per clock at 2.4 GHz = 78.6e12 lane-instructions/s, the rate behind
  the 157.3 TFLOPS FP32 vector peak);
* the share of unordered sample pairs that carry no near side (the zeros the
  dense walk multiplies through), from fs_plan_weighted_pairs.

    python tools/bench_stir.py                      # cfg2 and cfg4
    python tools/bench_stir.py --config cfg2 --out profiles/stir/bench_stir.jsonl
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

CONFIGS = {
    # name: (n, p, redundant columns)   (bench.py CONFIGS)
    "cfg2": (5000, 5000, 100),
    "cfg4": (20000, 20000, 100),
}
VALU_PEAK = 256 * 4 * 32 * 2.4e9   # lane-instructions per second
TILE = 128


def make_data(n, p, red, seed=42):
    from sklearn.datasets import make_classification
    X, y = make_classification(n_samples=n, n_features=p, n_informative=20, n_redundant=red,
                               random_state=seed)
    return np.ascontiguousarray(X, dtype=np.float32), y


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run(name, rounds, warmup):
    import torch
    from fastselect_amd import _lib
    from fastselect_amd.parallel import ShardedMultiSURF, prepare_inputs
    if _lib.device_count() < 1:
        raise SystemExit("bench_stir.py needs a HIP device (no CPU fallback)")
    n, p, red = CONFIGS[name]
    X, y = make_data(n, p, red)
    x, yv, recip, isd = prepare_inputs(X, y, backend="gpu")
    job = ShardedMultiSURF(x, yv, recip, isd, backend="gpu", shard=False)
    try:
        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out

        for _ in range(warmup):
            job.step()
            job.stir()
        t_step, t_stir, k_pass2, k_w, k_s = [], [], [], [], []
        scores = sums = None
        for _ in range(rounds):
            ms, s = timed(job.step)
            t_step.append(ms)
            k_pass2.append(job.kernel_ms(1))
            if scores is not None and not torch.equal(s, scores):
                raise SystemExit("step() changed after a stir()")
            scores = s
            ms, (sm, nh, nm) = timed(job.stir)
            t_stir.append(ms)
            k_w.append(job.plan.stir_kernel_ms(0))
            k_s.append(job.plan.stir_kernel_ms(1))
            if sums is not None and not torch.equal(sm, sums):
                raise SystemExit("stir() is not repeatable")
            sums = sm
        tiles = job.info()[0]
        weighted = job.weighted_pairs()
        pcnt, pdis = int((~isd).sum()), int(isd.sum())
        pad = lambda v: -(-v // 64) * 64  # noqa: E731
        dense_pairs = tiles * TILE * TILE
        valu = dense_pairs * (7.0 * pad(pcnt) + 4.0 * pad(pdis))
        score_s = statistics.median(k_s) * 1e-3
        _, _, t, _ = _lib.stir_statistics(sums.cpu().numpy(), nh, nm)
        return {
            "tool": "bench_stir", "config": name, "n": n, "p": p, "shards": job.shards,
            "rounds": rounds, "warmup": warmup,
            "step_host_ms": spread(t_step), "stir_host_ms": spread(t_stir),
            "pass2_kernel_ms": spread(k_pass2),
            "stir_weights_kernel_ms": spread(k_w), "stir_score_kernel_ms": spread(k_s),
            "stir_score_over_pass2": statistics.median(k_s) / statistics.median(k_pass2),
            "stir_host_over_step_host": statistics.median(t_stir) / statistics.median(t_step),
            "n_hit_pairs": nh, "n_miss_pairs": nm,
            "near_sides_x_features_per_s": (nh + nm) * p / score_s,
            "owned_tiles": tiles, "dense_pairs": dense_pairs,
            "zero_pair_share": 1.0 - weighted / (n * (n - 1) / 2.0) if weighted >= 0 else None,
            "valu_per_pair_feature": {"continuous": 7, "discrete": 4},
            "dense_pair_features_per_s": dense_pairs * (pad(pcnt) + pad(pdis)) / score_s,
            "valu_peak_fraction": valu / score_s / VALU_PEAK,
            "features_with_t_above_5": int((t > 5).sum()),
        }
    finally:
        job.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", action="append", choices=sorted(CONFIGS),
                    help="configuration(s) to run (default: cfg2 and cfg4)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stir", "bench_stir.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for name in args.config or ["cfg2", "cfg4"]:
            line = json.dumps(run(name, args.rounds, args.warmup))
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    main()
