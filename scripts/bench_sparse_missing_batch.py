"""Batched factorisation on a sparse A whose absent entries are missing against the same members run one after another on the solo
sparse-missing path (what rank selection on a ratings matrix cost before): one JSON line, written to
profiles/sparse_missing_batch_bench.json.

Matrices: 20000 x 10000 at 1 % and 5 % observed (uniform pattern) and the MovieLens-20M-shaped synthetic of bench_sparse_missing.py
(138 000 x 27 000, 1.95e7 stored entries, power-law column counts).  Members: the rank sweep k = 1 .. 10 and eight restarts at k = 8.
Both arithmetic modes, R defaults for square loss (inner 50, trace 2).
"batch" is one nnlm_run_batch of all members on a handle loaded by nnlm_set_matrix_csc_missing_batch; "sequence" is nnlm_set_factors +
nnlm_run of each member in turn on the same resident handle (the solo sparse-missing path, which such a handle runs bit for bit).  A step
is one outer iteration of every member, timed by a host clock around work that ends in a device synchronise, without the factor set-up.
Every case is warmed up first; batch and sequence alternate `--repeats` times in one process and the median, the smallest and the largest
step time are reported.  Phases come from the library's event scopes (nnlm_profile_get) in a further, profiled run of the same length.
Usage: python scripts/bench_sparse_missing_batch.py [--steps 20] [--warmup 3] [--repeats 3] [--only small|movielens] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib  # noqa: E402
import bench_sparse_missing as bsm  # noqa: E402  (the matrix generators)

INNER, TRACE, INNER_TOL = 50, 2, 1e-9
PHASES = ["spmm_h", "spmm_w", "sp_gram", "sweep_h", "sweep_w", "sp_errors", "sp_batch_errors", "batch_pen", "gram"]
Z = [0.0, 0.0, 0.0]
CASES = {"ranks_1_to_10": list(range(1, 11)), "restarts_8x8": [8] * 8}


def run_batch(h, ks, inits, steps):
    h.set_factors_batch(ks, [w for w, _ in inits], [x for _, x in inits])
    h.sync()
    t0 = time.perf_counter()
    h.run_batch(Z, Z, steps, -1.0, 0, False, INNER, INNER_TOL, 1, TRACE)
    h.sync()
    return time.perf_counter() - t0


def run_sequence(h, ks, inits, steps):
    run = 0.0
    for k, (w, x) in zip(ks, inits):
        h.set_factors(k, w, x)
        h.sync()
        t0 = time.perf_counter()
        h.run(Z, Z, steps, -1.0, 0, False, INNER, INNER_TOL, 1, TRACE)
        h.sync()
        run += time.perf_counter() - t0
    return run


def profiled(h, fn, ks, inits, steps):
    h.profile_reset()
    h.profile_enable(True)
    fn(h, ks, inits, steps)
    out = {}
    for nm in PHASES:
        ms, cnt = h.profile_get(nm)
        if cnt:
            out[nm] = {"ms": round(ms / steps, 4), "launches": round(cnt / steps, 2)}
    h.profile_enable(False)
    return out


def summary(times, steps, per):
    ms = sorted(1e3 * t / steps for t in times)
    med = ms[len(ms) // 2]
    return {"ms_per_step": round(med, 4), "ms_per_step_min": round(ms[0], 4), "ms_per_step_max": round(ms[-1], 4), "phases_per_step": per,
            "outside_phases_ms_per_step": round(med - sum(v["ms"] for v in per.values()), 4)}


def measure(res, name, S, steps, warmup, repeats):
    n, m = S[3]
    for pname, prec in (("f32", _lib.PREC_F32), ("f64", _lib.PREC_F64)):
        with nnlm_amd.Handle(0, prec) as h:
            h.set_matrix_csc_missing_batch(*S)
            for cname, ks in CASES.items():
                irng = np.random.default_rng(sum(ks))
                inits = [(0.1 * irng.random((n, k)), 0.1 * irng.random((k, m))) for k in ks]
                run_batch(h, ks, inits, warmup)
                pairs, chunks = int(h.get_info("sp_gram_batch_pairs")), int(h.get_info("sp_gram_chunks"))
                run_sequence(h, ks, inits, warmup)
                tb, ts = [], []
                for _ in range(repeats):  # (alternating: both see the same neighbours on a shared host)
                    tb.append(run_batch(h, ks, inits, steps))
                    ts.append(run_sequence(h, ks, inits, steps))
                bt = summary(tb, steps, profiled(h, run_batch, ks, inits, steps))
                sq = summary(ts, steps, profiled(h, run_sequence, ks, inits, steps))
                key = f"{pname}/{name}/{cname}"
                res["cases"][key] = {"ranks": ks, "shape": [n, m], "nnz": int(S[1].size), "tile_pairs": pairs, "h_gram_chunks": chunks, "batch": bt,
                                     "sequence": sq, "batch_over_sequence": round(bt["ms_per_step"] / sq["ms_per_step"], 3)}
                print(key, bt["ms_per_step"], sq["ms_per_step"], bt["phases_per_step"].get("sp_gram"), sq["phases_per_step"].get("sp_gram"),
                      file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=["small", "movielens"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_missing_batch_bench.json"))
    args = ap.parse_args()
    res = {"inner_max_iter": INNER, "trace": TRACE, "steps": args.steps, "repeats": args.repeats, "cases": {}}
    if os.path.exists(args.out) and args.only:  # (the two halves may be measured by separate runs: keep the other half's cases)
        try:
            res["cases"] = json.load(open(args.out)).get("cases", {})
        except ValueError:
            pass
    if args.only != "movielens":
        for density in (0.01, 0.05):
            S = bsm.uniform_csc(20000, 10000, int(density * 2e8), np.random.default_rng(int(1e6 * density)))
            measure(res, "20000x10000_d%g" % density, S, args.steps, args.warmup, args.repeats)
    if args.only != "small":
        S = bsm.power_law_csc(138000, 27000, 20_000_000, np.random.default_rng(20))
        measure(res, "movielens_shape", S, args.steps, args.warmup, args.repeats)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
