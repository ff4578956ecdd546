"""Per-entry weights on a sparse A (nnlm_set_matrix_csc_weighted): ms per outer iteration and per phase next to the unweighted doors on
the SAME structure, one JSON line, also written to profiles/sparse_weighted_bench.json.

  20000 x 10000 at 1 % and 5 % stored, k = 50, both arithmetic modes, four doors per case:
    missing            nnlm_set_matrix_csc_missing                 (per-column Grams over the stored rows)
    weighted_missing   nnlm_set_matrix_csc_weighted, absent = 1    (the same Grams with one weight read per stored entry)
    zero               nnlm_set_matrix_csc                         (one shared Gram: the plain zero door)
    weighted_zero      nnlm_set_matrix_csc_weighted, absent = 0    (implicit feedback: the Gram work of `missing` + the shared Gram)
The four handles live side by side; after a warm-up of each, timed windows of `steps` outer iterations ALTERNATE between the doors for
`rounds` rounds (the machines are shared: a difference is read against the spread of the rounds).  A step is one outer iteration of
nnlm_run() (W half-step, H half-step, the error block every second iteration), R defaults for square loss (inner 50, trace 2); phases
from the library's event scopes (nnlm_profile_get) in a separate, profiled run per door.
Usage: python scripts/bench_sparse_weighted.py [--steps 20] [--warmup 4] [--rounds 5] [--no-write]"""
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
PHASES = ["gram", "spmm_h", "spmm_w", "sp_gram", "sweep_h", "sweep_w", "sp_errors"]
DOORS = ["missing", "weighted_missing", "zero", "weighted_zero"]
Z = [0.0, 0.0, 0.0]


def uniform_csc(n, m, nnz, rng):
    flat = np.unique(rng.integers(0, n * m, size=nnz, dtype=np.int64))
    cols, rows = flat // n, flat % n
    indptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=m), out=indptr[1:])
    return indptr, rows.astype(np.int32), 0.5 + 4.5 * rng.random(flat.size), (n, m)  # (scores in [0.5, 5])


def open_door(h, door, csc, w):
    ptr, idx, val, shape = csc
    if door == "missing":
        h.set_matrix_csc_missing(ptr, idx, val, shape)
    elif door == "zero":
        h.set_matrix_csc(ptr, idx, val, shape)
    else:
        h.set_matrix_csc_weighted(ptr, idx, val, w, shape, absent_missing=door == "weighted_missing")


def run(h, steps):
    h.run(Z, Z, steps, -1.0, 0, False, INNER, INNER_TOL, 1, TRACE)
    h.sync()


def measure(prec, k, csc, w, steps, warmup, rounds):
    n, m = csc[3]
    rng = np.random.default_rng(1)
    W0, H0 = rng.random((n, k)) * 0.1, rng.random((k, m)) * 0.1
    hs = {d: nnlm_amd.Handle(0, prec) for d in DOORS}
    out = {d: {} for d in DOORS}
    try:
        for d in DOORS:
            open_door(hs[d], d, csc, w)
            out[d]["matrix_bytes"] = hs[d].get_info("matrix_bytes")
            hs[d].set_factors(k, W0, H0)
            run(hs[d], warmup)
        times = {d: [] for d in DOORS}
        for _ in range(rounds):
            for d in DOORS:  # (alternating: every door sees the same neighbours on the machine)
                t0 = time.perf_counter()
                run(hs[d], steps)
                times[d].append(1e3 * (time.perf_counter() - t0) / steps)
        for d in DOORS:
            t = np.array(times[d])
            out[d]["ms_per_step"] = round(float(np.median(t)), 4)
            out[d]["ms_per_step_min_max"] = [round(float(t.min()), 4), round(float(t.max()), 4)]
        for d in DOORS:  # phases: a run of their own (event scopes serialise the streams)
            h = hs[d]
            h.set_factors(k, W0, H0)
            run(h, warmup)
            h.profile_enable(True)
            h.profile_reset()
            run(h, steps)
            out[d]["phase_ms_per_step"] = {p: round(h.profile_get(p)[0] / steps, 4) for p in PHASES if h.profile_get(p)[1] > 0}
            h.profile_enable(False)
    finally:
        for h in hs.values():
            h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    res = {"config": {"inner_max_iter": INNER, "trace": TRACE, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds},
           "cases": []}
    rng = np.random.default_rng(0)
    n, m, k = 20000, 10000, 50
    for density in (0.01, 0.05):
        csc = uniform_csc(n, m, int(density * n * m), rng)
        w = 1.0 + 40.0 * rng.random(csc[2].size)  # (confidences 1 + alpha r)
        for pname, prec in (("f32", _lib.PREC_F32), ("f64", _lib.PREC_F64)):
            case = {"n": n, "m": m, "k": k, "density": density, "nnz": int(csc[2].size), "precision": pname}
            case.update(measure(prec, k, csc, w, args.steps, args.warmup, args.rounds))
            ms = {d: case[d]["ms_per_step"] for d in DOORS}
            gram = {d: case[d]["phase_ms_per_step"].get("sp_gram", 0.0) for d in DOORS}
            case["ratios"] = {"weighted_missing_over_missing": round(ms["weighted_missing"] / ms["missing"], 3),
                              "weighted_zero_over_missing": round(ms["weighted_zero"] / ms["missing"], 3),
                              "weighted_zero_over_zero": round(ms["weighted_zero"] / ms["zero"], 3),
                              "sp_gram_weighted_missing_over_missing": round(gram["weighted_missing"] / gram["missing"], 3),
                              "sp_gram_weighted_zero_over_missing": round(gram["weighted_zero"] / gram["missing"], 3)}
            res["cases"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if not args.no_write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "sparse_weighted_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
