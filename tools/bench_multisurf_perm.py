#!/usr/bin/env python
"""Time the MultiSURF permutation test's batched call (fs_plan_score_labels,
fs_labels.hip) on the GPU (MI355X) beside what a user did before it existed:
one full scoring step per labelling.

One JSON line per shape: 2000 x 2000 with B = 1000 labellings, bench.py's cfg2
(5000 x 5000) with B = 128 and cfg4 (20000 x 20000) with B = 32, the same
make_classification data.  Labelling 0 is y, the rest are permutations of it.

* ``labels_host_ms``: the host clock around one synchronous
  ``ShardedMultiSURF.score_labels`` with the (B, p) block downloaded; median of
  7 calls after 2 warm-ups.
* ``records_kernel_ms`` / ``counts_kernel_ms`` / ``score_kernel_ms``: HIP
  events of those calls (``fs_plan_labels_kernel_ms``: the record kernels once
  per call; the counts, reciprocal and weights kernels and the score kernel
  summed over the chunks of 32 labellings), medians.
* ``step_host_ms``: the full step (pass 1 + select + pass 2,
  ``ShardedMultiSURF.step()``) in the same session, median of 20;
  ``b_steps_ms_extrapolated`` is that times B -- an extrapolation, not a
  measurement of B steps.  ``pass2_kernel_ms``: the step's pass-2 score kernels
  (``fs_plan_kernel_ms(1)``), median.
* ``score_kernel_ms_per_labelling`` beside ``pass2_kernel_ms``: what a
  labelling costs beside the pass 2 it replaces (DESIGN.md reads it);
  ``mfma_peak_fraction_lower_bound``: weighted pairs (the padding to groups of
  256 not counted) x padded features x 32 labellings x 2 FLOP over the score
  kernel time and the chip's FP32-input MFMA peak (256 CUs x 4 SIMDs x 64
  FLOP/clk at 2.4 GHz = 157.3 TFLOPS).
* ``row0_max_err_over_scale``: row 0 against the step's scores, over max |s|.

    python tools/bench_multisurf_perm.py
    python tools/bench_multisurf_perm.py --shape cfg2 --out profiles/multisurf_perm/bench.jsonl
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
    "cfg4": (20000, 20000, 100, 32),
}
MFMA_PEAK = 256 * 4 * 64 * 2.4e9   # FP32-input MFMA FLOP per second


def make_data(n, p, red, seed=42):
    from sklearn.datasets import make_classification
    X, y = make_classification(n_samples=n, n_features=p, n_informative=20, n_redundant=red,
                               random_state=seed)
    return np.ascontiguousarray(X, dtype=np.float32), y


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run(name, calls, warmup, steps):
    import torch
    from fastselect_amd import _lib
    from fastselect_amd.parallel import ShardedMultiSURF, prepare_inputs
    if _lib.device_count() < 1:
        raise SystemExit("bench_multisurf_perm.py needs a HIP device (no CPU fallback)")
    n, p, red, B = SHAPES[name]
    X, y = make_data(n, p, red)
    x, yv, recip, isd = prepare_inputs(X, y, backend="gpu")
    enc = np.unique(yv, return_inverse=True)[1].astype(np.int32).reshape(-1)
    rng = np.random.default_rng(0)
    labels = np.stack([enc] + [rng.permutation(enc) for _ in range(B - 1)])
    job = ShardedMultiSURF(x, yv, recip, isd, backend="gpu", shard=False)
    try:
        if job.shards != 1:
            raise SystemExit("the distance tiles do not fit the device")

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out

        job.step()
        job.step()
        t_step, k_pass1, k_pass2 = [], [], []
        for _ in range(steps):
            ms, s = timed(lambda: job.step().cpu())
            t_step.append(ms)
            k_pass1.append(job.kernel_ms(0))
            k_pass2.append(job.kernel_ms(1))
        step_scores = s.numpy()
        t_lab, k_rec, k_cnt, k_sc = [], [], [], []
        first = None
        for c in range(warmup + calls):
            ms, out = timed(lambda: job.score_labels(labels).cpu())
            if first is None:
                first = out
            elif not torch.equal(out, first):
                raise SystemExit("score_labels() is not repeatable")
            if c >= warmup:
                t_lab.append(ms)
                k_rec.append(job.plan.labels_kernel_ms(0))
                k_cnt.append(job.plan.labels_kernel_ms(1))
                k_sc.append(job.plan.labels_kernel_ms(2))
        if not torch.equal(job.step().cpu(), s):
            raise SystemExit("step() changed after score_labels()")
        weighted = job.weighted_pairs()
        tiles = job.info()[0]
        pad = lambda v, m: -(-v // m) * m  # noqa: E731
        PW = pad(int((~isd).sum()), 64) + pad(int(isd.sum()), 64)
        chunks = -(-B // 32)
        score_s = statistics.median(k_sc) * 1e-3
        step_ms, lab_ms = statistics.median(t_step), statistics.median(t_lab)
        rows = first.numpy()
        return {
            "tool": "bench_multisurf_perm", "shape": name, "n": n, "p": p, "labellings": B,
            "calls": calls, "warmup": warmup, "steps": steps, "owned_tiles": tiles,
            "weighted_pairs": weighted,
            "labels_host_ms": spread(t_lab), "records_kernel_ms": spread(k_rec),
            "counts_kernel_ms": spread(k_cnt), "score_kernel_ms": spread(k_sc),
            "step_host_ms": spread(t_step), "pass1_kernel_ms": spread(k_pass1),
            "pass2_kernel_ms": spread(k_pass2),
            "b_steps_ms_extrapolated": step_ms * B,
            "speedup_over_b_steps_extrapolated": step_ms * B / lab_ms,
            "labels_host_ms_per_labelling": lab_ms / B,
            "score_kernel_ms_per_labelling": statistics.median(k_sc) / B,
            "score_per_labelling_over_pass2": statistics.median(k_sc) / B
            / statistics.median(k_pass2),
            # the padding records (at most one group of 256 per tile) are not counted
            "mfma_peak_fraction_lower_bound": (weighted * PW * 32.0 * chunks * 2.0) / score_s
            / MFMA_PEAK,
            "row0_max_err_over_scale": float(np.max(np.abs(rows[0] - step_scores))
                                             / np.max(np.abs(step_scores))),
            "null_max_over_observed_max": float(rows[1:].max() / rows[0].max()),
        }
    finally:
        job.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shape", action="append", choices=sorted(SHAPES),
                    help="shape(s) to run (default: all three)")
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multisurf_perm",
                                                  "bench_multisurf_perm.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for name in args.shape or ["n2000", "cfg2", "cfg4"]:
            line = json.dumps(run(name, args.calls, args.warmup, args.steps))
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    main()
