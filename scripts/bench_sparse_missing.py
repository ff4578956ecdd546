"""Sparse A whose absent entries are missing (nnlm_set_matrix_csc_missing): ms per outer iteration and per phase, one JSON line, also
written to profiles/sparse_missing_bench.json.

  * a MovieLens-20M-shaped synthetic: 138 000 x 27 000, 2e7 stored entries, power-law column counts (movies), uniform rows
    (customers), k = 16 and 50;
  * 20000 x 10000 at 1 % and 5 % observed, k = 50, next to the dense NA path (nnlm_set_matrix with NaN at the absent entries).
Both arithmetic modes.  A step is one outer iteration of nnlm_run() (W half-step, H half-step, the error block every second iteration),
R defaults for square loss (inner 50, trace 2); phases from the library's event scopes (nnlm_profile_get) in a second, profiled run.
Usage: python scripts/bench_sparse_missing.py [--steps 20] [--warmup 4] [--only small|movielens] [--no-write]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib  # noqa: E402

INNER, TRACE, INNER_TOL = 50, 2, 1e-9
PHASES_SPARSE = ["spmm_h", "spmm_w", "sp_gram", "sweep_h", "sweep_w", "sp_errors"]
PHASES_DENSE = ["gram", "xprod_h", "xprod_w", "xprod_w_err", "sweep_h", "sweep_w", "errors", "err_reduce"]


def csc_of(flat, n, m, rng):
    flat = np.unique(flat)
    cols, rows = flat // n, flat % n
    indptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=m), out=indptr[1:])
    return indptr, rows.astype(np.int32), 0.5 + 4.5 * rng.random(flat.size), (n, m)  # (scores in [0.5, 5])


def uniform_csc(n, m, nnz, rng):
    return csc_of(rng.integers(0, n * m, size=nnz, dtype=np.int64), n, m, rng)


def power_law_csc(n, m, nnz, rng, alpha=1.0):
    """Column j drawn with probability ~ 1 / (rank_j + 10)^alpha (a few very popular movies, a long tail), rows uniform; duplicates are
    dropped, so a little under nnz entries remain."""
    p = 1.0 / (np.arange(m) + 10.0) ** alpha
    p /= p.sum()
    cols = rng.permutation(m)[rng.choice(m, size=int(nnz * 1.08), p=p)]
    rows = rng.integers(0, n, size=cols.size)
    flat = np.unique(cols.astype(np.int64) * n + rows)
    if flat.size > nnz:
        flat = np.sort(rng.choice(flat, size=nnz, replace=False))
    return csc_of(flat, n, m, rng)


def nan_dense(csc):
    indptr, idx, val, (n, m) = csc
    A = np.full((n, m), np.nan, order="F")
    A[idx, np.repeat(np.arange(m), np.diff(indptr))] = val
    return A


def measure(prec, k, steps, warmup, csc=None, A=None):
    n, m = csc[3] if csc is not None else A.shape
    rng = np.random.default_rng(1)
    W0, H0 = rng.random((n, k)) * 0.1, rng.random((k, m)) * 0.1
    out = {}
    z = [0.0, 0.0, 0.0]
    with nnlm_amd.Handle(0, prec) as h:
        t0 = time.perf_counter()
        h.set_matrix_csc_missing(*csc) if csc is not None else h.set_matrix(A)
        out["upload_s"] = round(time.perf_counter() - t0, 3)
        out["matrix_bytes"] = h.get_info("matrix_bytes")
        h.set_factors(k, W0, H0)
        h.run(z, z, warmup, -1.0, 0, False, INNER, INNER_TOL, 1, TRACE)
        h.sync()
        t0 = time.perf_counter()
        h.run(z, z, steps, -1.0, 0, False, INNER, INNER_TOL, 1, TRACE)
        h.sync()
        out["ms_per_step"] = round(1e3 * (time.perf_counter() - t0) / steps, 4)
        if csc is not None:
            out["gram_chunks_last_h"] = h.get_info("sp_gram_chunks")
            out["gram_buffer_bytes"] = h.get_info("sp_gram_bytes")
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--only", choices=("small", "movielens"), default=None)
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    res = {"config": {"inner_max_iter": INNER, "trace": TRACE, "steps": args.steps, "warmup": args.warmup}, "cases": []}
    rng = np.random.default_rng(0)
    precs = (("f32", _lib.PREC_F32), ("f64", _lib.PREC_F64))
    if args.only in (None, "small"):
        n, m, k = 20000, 10000, 50
        for density in (0.01, 0.05):
            csc = uniform_csc(n, m, int(density * n * m), rng)
            A = nan_dense(csc)
            for pname, prec in precs:
                case = {"n": n, "m": m, "k": k, "density": density, "nnz": int(csc[2].size), "precision": pname,
                        "sparse_missing": measure(prec, k, args.steps, args.warmup, csc=csc),
                        "dense_na": measure(prec, k, args.steps, args.warmup, A=A)}
                case["sparse_over_dense_na"] = round(case["sparse_missing"]["ms_per_step"] / case["dense_na"]["ms_per_step"], 3)
                res["cases"].append(case)
                print(json.dumps(case), file=sys.stderr, flush=True)
            del A
    if args.only in (None, "movielens"):
        n, m, nnz = 138_000, 27_000, 20_000_000
        csc = power_law_csc(n, m, nnz, rng)
        counts = np.diff(csc[0])
        shape = {"nnz": int(csc[2].size), "col_count_max": int(counts.max()), "col_count_median": float(np.median(counts)),
                 "cols_with_at_most_5": int(np.sum(counts <= 5))}
        for k in (16, 50):
            for pname, prec in precs:
                case = {"n": n, "m": m, "k": k, "precision": pname, "structure": shape,
                        "sparse_missing": measure(prec, k, max(args.steps // 2, 4), max(args.warmup // 2, 2), csc=csc)}
                res["cases"].append(case)
                print(json.dumps(case), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if not args.no_write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "sparse_missing_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
