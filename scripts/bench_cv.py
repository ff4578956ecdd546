"""Rank selection on held-out entries: the batched factorisation on a hold-out handle against the SEQUENCE of solo missing-value runs of
the same members on the same handle: one JSON line, written to profiles/cv_bench.json.

Shape 20000 x 10000 (A = rank-10 product + noise), 10 % of the entries held out, both arithmetic modes, R defaults for square loss
(inner 50, trace 2); cases: the rank sweep k = 1 .. 10 and 8 restarts at k = 8.  Timing, set-up and phases as scripts/bench_batch.py
reports them (a step = one outer iteration of every member); + the time of one nnlm_holdout_errors call on the final factors.
Usage: python scripts/bench_cv.py [--steps 20] [--warmup 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib  # noqa: E402
from bench_batch import INNER, TRACE, measure, run_batch, run_sequence  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--holdout", type=float, default=0.1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cv_bench.json"))
    args = ap.parse_args()
    n, m = args.n, args.m
    rng = np.random.default_rng(0)
    A = np.asfortranarray(rng.random((n, 10)) @ rng.random((10, m)) + 0.1 * rng.random((n, m)))
    cols, rows = np.nonzero(rng.random((m, n)) < args.holdout)  # (column-major order: the CSC pattern as it stands)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=m))])
    cases = {"ranks_1_to_10": list(range(1, 11)), "restarts_8x8": [8] * 8}
    res = {"n": n, "m": m, "held_out": int(rows.size), "inner_max_iter": INNER, "trace": TRACE, "steps": args.steps, "cases": {}}
    for pname, prec in (("f32", _lib.PREC_F32), ("f64", _lib.PREC_F64)):
        with nnlm_amd.Handle(0, prec) as h:
            t0 = time.perf_counter()
            h.set_matrix_holdout(A, ptr, rows)
            res[f"{pname}/set_matrix_holdout_s"] = round(time.perf_counter() - t0, 3)
            for cname, ks in cases.items():
                irng = np.random.default_rng(sum(ks))
                inits = [(0.01 * irng.random((n, k)), 0.01 * irng.random((k, m))) for k in ks]
                s = measure(h, run_sequence, ks, inits, args.steps, args.warmup)
                b = measure(h, run_batch, ks, inits, args.steps, args.warmup)  # (last: the batch's factors are the ones left on the handle)
                t0 = time.perf_counter()
                hm, _ = h.holdout_errors()
                t_ho = time.perf_counter() - t0
                res["cases"][f"{pname}/{cname}"] = {"ranks": ks, "batch": b, "sequence": s,
                                                    "batch_over_sequence": round(b["ms_per_step"] / s["ms_per_step"], 3),
                                                    "holdout_errors_ms": round(1e3 * t_ho, 3), "holdout_mse": [float(v) for v in hm]}
                print(pname, cname, b["ms_per_step"], s["ms_per_step"], file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
