"""Batched factorisation on a sparse A against the same members run one after another on the solo sparse path: one JSON line, written
to profiles/sparse_batch_bench.json.

Cases at 20000 x 10000 (rank-10 product + noise on a uniform pattern), densities 0.1 %, 1 % and 5 %, both arithmetic modes, R defaults for
square loss (inner 50, trace 2):
  * restarts: 8 members of rank 8 (sum 64);
  * ranks:    the rank sweep k = 1 .. 10 (sum 55).
"batch" is one nnlm_run_batch of all members on a handle loaded by nnlm_set_matrix_csc_batch; "sequence" is nnlm_set_factors + nnlm_run
of each member in turn on the same resident handle (the solo sparse path, which a batch-loaded handle runs bit for bit).  A step is one
outer iteration of every member, timed by a host clock around work that ends in a device synchronise, without the factor set-up
(reported apart as setup_ms).  Every shape is warmed up first; batch and sequence alternate `--repeats` times and the median, the
smallest and the largest step time are reported.  Phases come from the library's event scopes (nnlm_profile_get) in a further, profiled
run of the same length: per step and, for the three phases that walk the non-zeros, per launch.
Usage: python scripts/bench_sparse_batch.py [--steps 50] [--warmup 5] [--repeats 3]"""
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
PHASES = ["gram", "spmm_h", "spmm_w", "sweep_h", "sweep_w", "sp_errors", "sp_batch_errors", "batch_pen"]
PER_LAUNCH = ("spmm_h", "spmm_w", "sp_batch_errors", "sp_errors")
Z = [0.0, 0.0, 0.0]


def make_csc(n, m, density, rng):
    """Uniform pattern of about density n m entries; values = a rank-10 product + noise at the stored positions."""
    want = int(round(density * n * m))
    flat = np.unique(rng.integers(0, n * m, size=int(want * 1.06) + 16, dtype=np.int64))
    if flat.size > want:
        flat = np.sort(rng.choice(flat, size=want, replace=False))
    cols, rows = flat // n, flat % n
    Wp, Hp = rng.random((n, 10)), rng.random((10, m))
    val = np.empty(flat.size)
    for s in range(0, flat.size, 1 << 20):
        e = slice(s, s + (1 << 20))
        val[e] = np.einsum("ij,ji->i", Wp[rows[e]], Hp[:, cols[e]]) + 0.1 * rng.random(rows[e].size)
    indptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=m), out=indptr[1:])
    return indptr, rows.astype(np.int32), val, (n, m)


def phases(h):
    out = {}
    for nm in PHASES:
        ms, cnt = h.profile_get(nm)
        if cnt:
            out[nm] = {"ms": ms, "launches": cnt}
    return out


def run_batch(h, ks, inits, steps):
    t0 = time.perf_counter()
    h.set_factors_batch(ks, [w for w, _ in inits], [x for _, x in inits])
    h.sync()
    t1 = time.perf_counter()
    h.run_batch(Z, Z, steps, -1.0, 0, False, INNER, INNER_TOL, 1, TRACE)
    h.sync()
    return t1 - t0, time.perf_counter() - t1


def run_sequence(h, ks, inits, steps):
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


def profiled(h, fn, ks, inits, steps):
    h.profile_reset()
    h.profile_enable(True)
    fn(h, ks, inits, steps)
    ph = phases(h)
    h.profile_enable(False)
    per = {nm: {"ms": round(v["ms"] / steps, 4), "launches": round(v["launches"] / steps, 2)} for nm, v in ph.items()}
    launch = {nm: round(ph[nm]["ms"] / ph[nm]["launches"], 4) for nm in PER_LAUNCH if nm in ph}
    return per, launch


def summary(times, setups, steps, per, launch):
    ms = sorted(1e3 * t / steps for t in times)
    med = ms[len(ms) // 2]
    return {"ms_per_step": round(med, 4), "ms_per_step_min": round(ms[0], 4), "ms_per_step_max": round(ms[-1], 4),
            "setup_ms": round(1e3 * sorted(setups)[len(setups) // 2], 3), "phases_per_step": per, "ms_per_launch": launch,
            "outside_phases_ms_per_step": round(med - sum(v["ms"] for v in per.values()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--densities", type=float, nargs="+", default=[0.001, 0.01, 0.05])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sparse_batch_bench.json"))
    args = ap.parse_args()
    n, m, steps = args.n, args.m, args.steps
    cases = {"restarts_8x8": [8] * 8, "ranks_1_to_10": list(range(1, 11))}
    res = {"n": n, "m": m, "inner_max_iter": INNER, "trace": TRACE, "steps": steps, "repeats": args.repeats, "cases": {}}
    for density in args.densities:
        S = make_csc(n, m, density, np.random.default_rng(int(1e6 * density)))
        for pname, prec in (("f32", _lib.PREC_F32), ("f64", _lib.PREC_F64)):
            with nnlm_amd.Handle(0, prec) as h:
                h.set_matrix_csc_batch(*S)
                for cname, ks in cases.items():
                    irng = np.random.default_rng(sum(ks))
                    inits = [(0.01 * irng.random((n, k)), 0.01 * irng.random((k, m))) for k in ks]
                    tb, ts, sb, ss = [], [], [], []
                    run_batch(h, ks, inits, args.warmup)
                    run_sequence(h, ks, inits, args.warmup)
                    for _ in range(args.repeats):  # (alternating: both see the same neighbours on a shared host)
                        a, b = run_batch(h, ks, inits, steps)
                        sb.append(a), tb.append(b)
                        a, b = run_sequence(h, ks, inits, steps)
                        ss.append(a), ts.append(b)
                    bt = summary(tb, sb, steps, *profiled(h, run_batch, ks, inits, steps))
                    sq = summary(ts, ss, steps, *profiled(h, run_sequence, ks, inits, steps))
                    key = f"{pname}/d{density:g}/{cname}"
                    res["cases"][key] = {"ranks": ks, "density": density, "nnz": int(S[1].size), "batch": bt, "sequence": sq,
                                         "batch_over_sequence": round(bt["ms_per_step"] / sq["ms_per_step"], 3)}
                    print(key, bt["ms_per_step"], sq["ms_per_step"], bt["ms_per_launch"], file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
