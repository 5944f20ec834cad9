#!/usr/bin/env python
"""Hash what the pair-table kernels (k_mi_scan, k_cfs_row, k_mi_row) compute,
to compare two builds of the library bit for bit.

One JSON line per case with a SHA-256 of the raw bytes of
  * mi_matrices("gpu"): relevance, redundancy and counts;
  * the GPU Cfs handle: relevance(), every row(f), and search(0.0)'s selection
    and merits;
  * mrmr_select("gpu"): selection, relevance and rows, for MID and MIQ.
The cases are the GPU suites' own tables (mi_np.SHAPES, test_gpu_cfs.SU_CASES,
test_gpu_mrmr_selected.SHAPES; a case that two tables share runs once) with the
suites' k (p up to 130, else 24), and bench_cfs.py's geno3 and states10, the
shapes that are timed, with bench_mrmr.py's k.  The suites' tolerances against
the CPU backend would not show a reordered sum; two files of this tool from two
builds on the same device must be byte-identical.

    python tools/pair_bits.py --out profiles/pairtab/bits_change.jsonl
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def cases():
    """name -> (make() -> (X, y, S), k)"""
    import mi_np
    import test_gpu_cfs
    import test_gpu_mrmr_selected
    import bench_cfs
    import bench_mrmr
    out, seen = {}, set()
    for table, shapes in (("mi", mi_np.SHAPES), ("su", test_gpu_cfs.SU_CASES),
                          ("mrmr", test_gpu_mrmr_selected.SHAPES)):
        for name in sorted(shapes):
            if shapes[name] not in seen:
                seen.add(shapes[name])
                out[f"{table}/{name}"] = (shapes[name], None)
    for name in ("geno3", "states10"):
        n, p, states = bench_cfs.SHAPES[name]
        out[f"bench/{name}"] = ((lambda n, p, s: lambda: bench_cfs.make(n, p, s) + (s,))(
            n, p, states), bench_mrmr.K)
    return out


def run(name, make, k):
    from fastselect_amd import _lib
    X, y, S = make()
    p = X.shape[1]
    k = k or (p if p <= 130 else 24)
    line = {"case": name, "n": int(X.shape[0]), "p": int(p), "states": int(S), "k": int(k)}
    rel, red, cnt = _lib.mi_matrices("gpu", X, y, S, want_counts=True)
    line["mi_relevance"], line["mi_redundancy"], line["mi_counts"] = sha(rel), sha(red), sha(cnt)
    with _lib.Cfs("gpu", X, y, S) as g:
        line["cfs_relevance"] = sha(g.relevance())
        line["cfs_rows"] = sha(*(g.row(f) for f in range(p)))
        sel, merits = g.search(0.0)
        line["cfs_selected"], line["cfs_merits"] = sha(sel), sha(merits)
    for method in ("MID", "MIQ"):
        sel, r, rows = _lib.mrmr_select("gpu", X, y, S, k, method=method)
        m = method.lower()
        line[f"mrmr_{m}_selected"], line[f"mrmr_{m}_relevance"] = sha(sel), sha(r)
        line[f"mrmr_{m}_rows"] = sha(rows)
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="write the JSON lines to this file too (replaced)")
    a = ap.parse_args()
    from fastselect_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("pair_bits: no HIP device visible")
    lines = []
    for name, (make, k) in cases().items():
        lines.append(json.dumps(run(name, make, k)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
