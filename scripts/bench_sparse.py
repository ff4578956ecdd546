"""Sparse A against the same matrix run dense: one JSON line with ms per step and per phase.

  * 20000 x 10000, k = 50, R defaults for square loss (inner 50, trace 2), densities 0.1 %, 1 % and 5 %, both arithmetic modes, each
    next to the same matrix uploaded dense;
  * 2 000 000 x 50 000 with 5e6 non-zeros at k = 8 (no dense counterpart: 400 GB as fp32).

A step is one outer iteration of nnlm_run() (W half-step, H half-step, the error block every second iteration), timed on a resident
handle like bench.py times the dense path; phases come from the library's own event scopes (nnlm_profile_get) in a second, profiled
run of the same length.  Usage: python scripts/bench_sparse.py [--steps 100] [--warmup 10] [--only-huge]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib  # noqa: E402

INNER, TRACE, INNER_TOL = 50, 2, 1e-9
PHASES_SPARSE = ["gram", "spmm_h", "spmm_w", "sweep_h", "sweep_w", "sp_errors"]
PHASES_DENSE = ["gram", "xprod_h", "xprod_w", "xprod_w_err", "sweep_h", "sweep_w", "errors", "err_reduce"]


def rand_csc(n, m, nnz, rng):
    flat = np.unique(rng.integers(0, n * m, size=int(nnz * 1.02) + 16, dtype=np.int64))
    flat = np.sort(rng.choice(flat, size=min(nnz, flat.size), replace=False))
    cols, rows = flat // n, flat % n
    indptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=m), out=indptr[1:])
    return indptr, rows.astype(np.int32), rng.random(flat.size), (n, m)


def to_dense(csc):
    indptr, idx, val, (n, m) = csc
    A = np.zeros((n, m), order="F")
    A[idx, np.repeat(np.arange(m), np.diff(indptr))] = val
    return A


def measure(prec, k, steps, warmup, csc=None, A=None):
    n, m = csc[3] if csc is not None else A.shape
    rng = np.random.default_rng(1)
    W0, H0 = rng.random((n, k)) * 0.1, rng.random((k, m)) * 0.1
    out = {}
    with nnlm_amd.Handle(0, prec) as h:
        t0 = time.perf_counter()
        h.set_matrix_csc(*csc) if csc is not None else h.set_matrix(A)
        out["upload_s"] = round(time.perf_counter() - t0, 3)
        out["matrix_bytes"] = h.get_info("matrix_bytes")
        z = [0.0, 0.0, 0.0]
        h.set_factors(k, W0, H0)
        h.run(z, z, warmup, -1.0, 0, False, INNER, INNER_TOL, 1, TRACE)
        h.sync()
        t0 = time.perf_counter()
        h.run(z, z, steps, -1.0, 0, False, INNER, INNER_TOL, 1, TRACE)
        h.sync()
        out["ms_per_step"] = round(1e3 * (time.perf_counter() - t0) / steps, 4)
        h.set_factors(k, W0, H0)
        h.run(z, z, warmup, -1.0, 0, False, INNER, INNER_TOL, 1, TRACE)
        h.profile_enable(True)
        h.profile_reset()
        h.run(z, z, steps, -1.0, 0, False, INNER, INNER_TOL, 1, TRACE)
        h.sync()
        out["phase_ms_per_step"] = {p: round(h.profile_get(p)[0] / steps, 4)
                                    for p in (PHASES_SPARSE if csc is not None else PHASES_DENSE) if h.profile_get(p)[1] > 0}
        h.profile_enable(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only-huge", action="store_true")
    args = ap.parse_args()
    res = {"config": {"inner_max_iter": INNER, "trace": TRACE, "steps": args.steps, "warmup": args.warmup}, "cases": []}
    rng = np.random.default_rng(0)
    if not args.only_huge:
        n, m, k = 20000, 10000, 50
        for density in (0.001, 0.01, 0.05):
            csc = rand_csc(n, m, int(density * n * m), rng)
            A = to_dense(csc)
            for pname, prec in (("f32", _lib.PREC_F32), ("f64", _lib.PREC_F64)):
                case = {"n": n, "m": m, "k": k, "density": density, "nnz": int(csc[2].size), "precision": pname,
                        "sparse": measure(prec, k, args.steps, args.warmup, csc=csc),
                        "dense": measure(prec, k, args.steps, args.warmup, A=A)}
                case["sparse_over_dense"] = round(case["sparse"]["ms_per_step"] / case["dense"]["ms_per_step"], 3)
                res["cases"].append(case)
            del A
    n, m, k, nnz = 2_000_000, 50_000, 8, 5_000_000
    csc = rand_csc(n, m, nnz, rng)
    for pname, prec in (("f32", _lib.PREC_F32), ("f64", _lib.PREC_F64)):
        res["cases"].append({"n": n, "m": m, "k": k, "nnz": int(csc[2].size), "precision": pname,
                             "sparse": measure(prec, k, max(args.steps // 5, 4), max(args.warmup // 5, 2), csc=csc)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
