"""Batched factorisation against the same members run one after another: one JSON line, written to profiles/batch_bench.json.

Cases at 20000 x 10000 (A = rank-10 product + noise), both arithmetic modes, R defaults for square loss (inner 50, trace 2):
  * restarts: 8 members of rank 8 (sum 64);
  * ranks:    the rank sweep k = 1 .. 10 (sum 55).
"batch" is one nnlm_run_batch of all members; "sequence" is nnlm_set_factors + nnlm_run of each member in turn on the same warm handle
(the matrix uploaded once).  A step is one outer iteration of every member, timed without the factor setup (set_factors_batch /
set_factors: host repack, upload, allocations), which is reported apart as setup_ms; phases come from the library's event scopes
(nnlm_profile_get) in a second, profiled run of the same length; outside_phases_ms_per_step = step time not covered by any scope.  Usage: python scripts/bench_batch.py [--steps 40] [--warmup 5]"""
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
PHASES = ["gram", "xprod_h", "xprod_w", "xprod_w_err", "sweep_h", "sweep_w", "errors", "err_reduce", "batch_errors", "batch_pen"]
Z = [0.0, 0.0, 0.0]


def phases(h):
    out = {}
    for nm in PHASES:
        ms, cnt = h.profile_get(nm)
        if cnt:
            out[nm] = {"ms": round(ms, 4), "launches": cnt}
    return out


def run_batch(h, ks, inits, steps):
    """(setup s, run s): set_factors_batch (host repack, upload, batch buffers) timed apart from run_batch."""
    t0 = time.perf_counter()
    h.set_factors_batch(ks, [w for w, _ in inits], [x for _, x in inits])
    h.sync()
    t1 = time.perf_counter()
    h.run_batch(Z, Z, steps, -1.0, 0, False, INNER, INNER_TOL, 1, TRACE)
    h.sync()
    return t1 - t0, time.perf_counter() - t1


def run_sequence(h, ks, inits, steps):
    """(setup s, run s): each member's set_factors timed apart from its run."""
    setup = run = 0.0
    for k, (w, x) in zip(ks, inits):
        t0 = time.perf_counter()
        h.set_factors(k, w, x)
        h.sync()
        t1 = time.perf_counter()
        h.run(Z, Z, steps, -1.0, 0, False, INNER, INNER_TOL, 1, TRACE)
        h.sync()
        setup, run = setup + t1 - t0, run + time.perf_counter() - t1
    return setup, run


def measure(h, fn, ks, inits, steps, warmup):
    fn(h, ks, inits, warmup)
    setup, run = fn(h, ks, inits, steps)
    h.profile_reset()
    h.profile_enable(True)
    fn(h, ks, inits, steps)
    ph = phases(h)
    h.profile_enable(False)
    per = {nm: {"ms": round(v["ms"] / steps, 4), "launches": round(v["launches"] / steps, 2)} for nm, v in ph.items()}
    ms = 1e3 * run / steps
    return {"ms_per_step": round(ms, 4), "setup_ms": round(1e3 * setup, 3), "phases_per_step": per,
            "outside_phases_ms_per_step": round(ms - sum(v["ms"] for v in per.values()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "batch_bench.json"))
    args = ap.parse_args()
    n, m = args.n, args.m
    rng = np.random.default_rng(0)
    A = np.asfortranarray(rng.random((n, 10)) @ rng.random((10, m)) + 0.1 * rng.random((n, m)))
    cases = {"restarts_8x8": [8] * 8, "ranks_1_to_10": list(range(1, 11))}
    res = {"n": n, "m": m, "inner_max_iter": INNER, "trace": TRACE, "steps": args.steps, "cases": {}}
    for pname, prec in (("f32", _lib.PREC_F32), ("f64", _lib.PREC_F64)):
        with nnlm_amd.Handle(0, prec) as h:
            h.set_matrix(A)
            for cname, ks in cases.items():
                irng = np.random.default_rng(sum(ks))
                inits = [(0.01 * irng.random((n, k)), 0.01 * irng.random((k, m))) for k in ks]
                b = measure(h, run_batch, ks, inits, args.steps, args.warmup)
                s = measure(h, run_sequence, ks, inits, args.steps, args.warmup)
                res["cases"][f"{pname}/{cname}"] = {"ranks": ks, "batch": b, "sequence": s,
                                                    "batch_over_sequence": round(b["ms_per_step"] / s["ms_per_step"], 3)}
                print(pname, cname, b["ms_per_step"], s["ms_per_step"], file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
