"""What nnlm_svd and the NNDSVD start cost, and what the start buys.  One JSON document, written to profiles/svd_init_bench.json.

Matrices: bench.py's dense A (20000 x 10000, U(0, 1)) and a 1 % sparse matrix of the same shape (2e6 stored U(0, 1) values, absent
entries zeros).  k = 50, sketch width l = 60, 2 power iterations, both arithmetic modes, one handle per matrix and mode.

Reported per matrix and mode:
  svd_ms            wall time of Handle.svd with the device idle before and after: one warm-up call, then --reps timed ones
                    (median [min, max]); `phases_ms` is one more call with nnlm_profile_enable, in which every phase waits for its
                    kernels: cross products (2 q + 2 = 6 passes over A), Grams, rotations, the 13 host eigendecompositions, waits and
                    transfers, setting and freeing the rank-l factor buffers.  `xprod_ms` / `spmm_ms`: the library's device-event scopes around the passes of that call.
  nndsvd_ms         wall time of Handle.set_factors_nndsvd (variant nndsvd; nndsvda: + the one-off sum of A, `nndsvda_first_ms`).
  convergence       for each of three seeds, alternating in one process: a run from the random start 0.01 U(0, 1) to rel.tol 1e-4
                    (SCD, square loss, R defaults) gives that seed's final target error; a run from nndsvd and one from nndsvda (the
                    sketch matrix drawn from the same seed) are read at the first trace point at or below it, then repeated with exactly
                    that many iterations to time them.  Medians over the seeds of iterations and seconds; the decomposition and the
                    start are not in the seconds of the nndsvd rows (they are svd_ms + nndsvd_ms).
Usage: python scripts/bench_svd_init.py [--reps 3] [--out profiles/svd_init_bench.json] [--size n,m,k,l]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nnlm_amd import _lib, api  # noqa: E402
import bench  # noqa: E402

Z3 = [0.0, 0.0, 0.0]
PHASES = ("cross", "gram", "rotate", "eig", "wait", "setup", "total")


def spread(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def timed(h, f):
    h.sync()
    t0 = time.perf_counter()
    f()
    h.sync()
    return (time.perf_counter() - t0) * 1e3


def sparse_matrix(n, m, density, rng):
    flat = np.unique(rng.integers(0, n, size=int(density * n * m)) + n * rng.integers(0, m, size=int(density * n * m)))
    cols = flat // n
    ptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=m), out=ptr[1:])
    return ptr, (flat % n).astype(np.int32), rng.random(flat.size) + 0.01, (n, m)


def run(h, max_iter, rel_tol):
    h.sync()
    t0 = time.perf_counter()
    t = h.run(Z3, Z3, max_iter, rel_tol, 0, False, 50, 1e-9, 1, 2)
    return t, time.perf_counter() - t0


def measure(load, n, m, k, l, q, prec, reps, sparse):
    out = {}
    with _lib.Handle(0, prec) as h:
        load(h)
        om = api._svd_omega(l, m, np.random.default_rng(0))
        h.svd(l, q, om)
        out["svd_ms"] = spread([timed(h, lambda: h.svd(l, q, om)) for _ in range(reps)])
        h.profile_enable(True)
        h.profile_reset()
        h.svd(l, q, om)
        out["phases_ms"] = {p: round(h.get_info("svd_ms_" + p), 3) for p in PHASES}
        names = ("spmm_h", "spmm_w") if sparse else ("xprod_h", "xprod_w")
        out["spmm_ms" if sparse else "xprod_ms"] = {nm: dict(zip(("ms", "launches"), h.profile_get(nm))) for nm in names + ("gram",)}
        h.profile_enable(False)
        out["kept"] = int(h.get_info("svd_kept"))
        out["sigma"] = [float(x) for x in h.get_svd(k)[1][[0, 1, k - 1]]]
        out["nndsvda_first_ms"] = round(timed(h, lambda: h.set_factors_nndsvd(k, "nndsvda")), 3)
        out["nndsvd_ms"] = spread([timed(h, lambda: h.set_factors_nndsvd(k, "nndsvd")) for _ in range(reps)])
        rows = {"random": [], "nndsvd": [], "nndsvda": []}
        for seed in (1, 2, 3):
            g = np.random.default_rng(seed)
            h.set_factors(k, 0.01 * g.random((n, k)), 0.01 * g.random((k, m)))
            t, sec = run(h, 500, 1e-4)
            target = t["target_error"][-1]
            rows["random"].append(dict(iters=t["n_iteration"], seconds=sec, final=float(target)))
            h.svd(l, q, api._svd_omega(l, m, np.random.default_rng(seed)))
            for variant in ("nndsvd", "nndsvda"):
                h.set_factors_nndsvd(k, variant)
                t, _ = run(h, 500, 1e-4)
                hit = np.flatnonzero(t["target_error"] <= target)
                if hit.size == 0:  # (stopped by its own rule above the random start's error)
                    rows[variant].append(dict(iters=None, seconds=None, final=float(t["target_error"][-1]), own_iters=t["n_iteration"]))
                    continue
                iters = int(min(2 * (hit[0] + 1), t["n_iteration"]))
                h.set_factors_nndsvd(k, variant)
                _, sec = run(h, iters, -1.0)
                rows[variant].append(dict(iters=iters, seconds=sec, final=float(t["target_error"][-1]), own_iters=t["n_iteration"]))
        conv = {}
        for name, rs in rows.items():
            ok = [r for r in rs if r["iters"] is not None]
            conv[name] = dict(runs=rs, reached=len(ok), median_iters=statistics.median(r["iters"] for r in ok) if ok else None,
                              median_seconds=round(statistics.median(r["seconds"] for r in ok), 4) if ok else None)
        out["convergence"] = conv
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svd_init_bench.json"))
    ap.add_argument("--size", default="20000,10000,50,60")
    a = ap.parse_args()
    n, m, k, l = (int(v) for v in a.size.split(","))
    q = 2
    A = bench.make_inputs(n, m, k, False)[0]
    S = sparse_matrix(n, m, 0.01, np.random.default_rng(bench.SEED))
    res = dict(shape=[n, m], k=k, l=l, power_iters=q, reps=a.reps, sparse_nnz=int(S[2].size), results={})
    for pname, prec in (("f32", _lib.PREC_F32), ("f64", _lib.PREC_F64)):
        res["results"]["dense_" + pname] = measure(lambda h: h.set_matrix(A), n, m, k, l, q, prec, a.reps, False)
        print(json.dumps({"dense_" + pname: res["results"]["dense_" + pname]}), flush=True)
        res["results"]["sparse_" + pname] = measure(lambda h: h.set_matrix_csc(*S), n, m, k, l, q, prec, a.reps, True)
        print(json.dumps({"sparse_" + pname: res["results"]["sparse_" + pname]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
