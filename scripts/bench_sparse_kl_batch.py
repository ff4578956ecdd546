"""Batched KL factorisation of a sparse count matrix against the same members run one after another on the solo sparse-KL path: one
JSON line, written to profiles/sparse_kl_batch_bench.json.

Cases at 20000 x 10000 (Poisson counts of a rank-10 model on a uniform pattern; zeros leave the structure), densities 0.1 %, 1 % and 5 %,
both arithmetic modes, SCD (method 3) and Lee (method 4), R's defaults for KL loss (one inner sweep, trace 100):
  * restarts: 8 members of rank 8 (sum 64);
  * ranks:    the rank sweep k = 1 .. 10 (sum 55).
"batch" is one nnlm_run_batch of all members on a handle loaded by nnlm_set_matrix_csc_kl_batch; "sequence" is nnlm_set_factors +
nnlm_run of each member in turn on the same resident handle (the solo sparse-KL path, which that handle runs bit for bit).  A step is one
outer iteration of every member, timed by a host clock around work that ends in a device synchronise, without the factor set-up (reported
apart as setup_ms).  Every shape is warmed up first; the step count is doubled until a window of either kind lasts at least
`--min-window` seconds; batch and sequence then alternate `--repeats` times, and the median and the spread (max - min) / median of each
are reported.  "batch_wins" says whether the batch's median is below the sequence's by more than the two spreads together.  Phases come
from the library's event scopes (nnlm_profile_get) in a further, profiled run of the same length.
`--group G` (1, 2 or 4) sets NNLM_SPKL_BATCH_GROUP, the number of member chains a wavefront of sp_kl_batch_kernel interleaves, for the
handles of the run; the file then goes to profiles/sparse_kl_batch_bench_g<G>.json.
Usage: python scripts/bench_sparse_kl_batch.py [--steps 8] [--warmup 2] [--repeats 3] [--group G]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib  # noqa: E402

INNER, TRACE, INNER_TOL = 1, 100, 1e-9
PHASES = ["spkl_copy", "spkl_batch_h", "spkl_batch_w", "spkl_solve_h", "spkl_solve_w", "sp_errors", "sp_batch_errors", "batch_pen"]
Z = [0.0, 0.0, 0.0]


def make_counts(n, m, density, rng):
    """Uniform pattern of about density n m positions; Poisson counts of a rank-10 model with mean 4 there, the zeros dropped."""
    want = int(round(density * n * m))
    flat = np.unique(rng.integers(0, n * m, size=int(want * 1.06) + 16, dtype=np.int64))
    if flat.size > want:
        flat = np.sort(rng.choice(flat, size=want, replace=False))
    cols, rows = flat // n, flat % n
    Wp, Hp = rng.random((n, 10)), rng.random((10, m))
    val = np.empty(flat.size)
    for s in range(0, flat.size, 1 << 20):
        e = slice(s, s + (1 << 20))
        val[e] = rng.poisson(1.6 * np.einsum("ij,ji->i", Wp[rows[e]], Hp[:, cols[e]]))
    keep = val > 0
    cols, rows, val = cols[keep], rows[keep], val[keep]
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


def run_batch(h, ks, inits, steps, method):
    t0 = time.perf_counter()
    h.set_factors_batch(ks, [w for w, _ in inits], [x for _, x in inits])
    h.sync()
    t1 = time.perf_counter()
    h.run_batch(Z, Z, steps, -1.0, 0, False, INNER, INNER_TOL, method, TRACE)
    h.sync()
    return t1 - t0, time.perf_counter() - t1


def run_sequence(h, ks, inits, steps, method):
    setup = run = 0.0
    for k, (w, x) in zip(ks, inits):
        t0 = time.perf_counter()
        h.set_factors(k, w, x)
        h.sync()
        t1 = time.perf_counter()
        h.run(Z, Z, steps, -1.0, 0, False, INNER, INNER_TOL, method, TRACE)
        h.sync()
        setup, run = setup + t1 - t0, run + time.perf_counter() - t1
    return setup, run


def profiled(h, fn, ks, inits, steps, method):
    h.profile_reset()
    h.profile_enable(True)
    fn(h, ks, inits, steps, method)
    ph = phases(h)
    h.profile_enable(False)
    return {nm: {"ms": round(v["ms"] / steps, 4), "launches": round(v["launches"] / steps, 2)} for nm, v in ph.items()}


def summary(times, setups, steps, per):
    ms = sorted(1e3 * t / steps for t in times)
    med = ms[len(ms) // 2]
    return {"ms_per_step": round(med, 4), "ms_per_step_min": round(ms[0], 4), "ms_per_step_max": round(ms[-1], 4),
            "spread": round((ms[-1] - ms[0]) / med, 4), "window_s_min": round(min(times), 3),
            "setup_ms": round(1e3 * sorted(setups)[len(setups) // 2], 3), "phases_per_step": per,
            "outside_phases_ms_per_step": round(med - sum(v["ms"] for v in per.values()), 4)}


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--min-window", type=float, default=0.3)
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--densities", type=float, nargs="+", default=[0.001, 0.01, 0.05])
    ap.add_argument("--modes", nargs="+", default=["f32", "f64"])
    ap.add_argument("--methods", type=int, nargs="+", default=[4, 3])
    ap.add_argument("--group", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.group:
        os.environ["NNLM_SPKL_BATCH_GROUP"] = str(args.group)  # (read when a handle is created)
    out = args.out or os.path.join(root, "profiles", "sparse_kl_batch_bench%s.json" % ("_g%d" % args.group if args.group else ""))
    n, m = args.n, args.m
    cases = {"restarts_8x8": [8] * 8, "ranks_1_to_10": list(range(1, 11))}
    names = {3: "scd", 4: "lee"}
    res = {"n": n, "m": m, "inner_max_iter": INNER, "trace": TRACE, "repeats": args.repeats, "min_window_s": args.min_window, "cases": {}}
    for density in args.densities:
        S = make_counts(n, m, density, np.random.default_rng(int(1e6 * density)))
        lens = np.concatenate([np.diff(S[0]), np.bincount(S[1], minlength=n)])
        for pname in args.modes:
            prec = _lib.PREC_F32 if pname == "f32" else _lib.PREC_F64
            with nnlm_amd.Handle(0, prec) as h:
                h.set_matrix_csc_kl_batch(*S)
                res["group"] = int(h.get_info("sparse_kl_batch_group"))
                short_max = int(h.get_info("sparse_kl_short_max"))
                for method in args.methods:
                    for cname, ks in cases.items():
                        irng = np.random.default_rng(sum(ks))
                        lvl = np.sqrt(4.0 * density)  # (the fit's level: density x the model's mean)
                        inits = [(np.sqrt(lvl / k) * (0.5 + irng.random((n, k))), np.sqrt(lvl / k) * (0.5 + irng.random((k, m)))) for k in ks]
                        run_batch(h, ks, inits, args.warmup, method)
                        run_sequence(h, ks, inits, args.warmup, method)
                        steps = args.steps
                        while True:  # every timed window at least min-window seconds
                            w = min(run_batch(h, ks, inits, steps, method)[1], run_sequence(h, ks, inits, steps, method)[1])
                            if w >= args.min_window or steps >= 4096:
                                break
                            steps *= 2 if w > args.min_window / 2 else 4
                        tb, ts, sb, ss = [], [], [], []
                        for _ in range(args.repeats):  # (alternating: both see the same neighbours on a shared host)
                            a, b = run_batch(h, ks, inits, steps, method)
                            sb.append(a), tb.append(b)
                            a, b = run_sequence(h, ks, inits, steps, method)
                            ss.append(a), ts.append(b)
                        bt = summary(tb, sb, steps, profiled(h, run_batch, ks, inits, steps, method))
                        sq = summary(ts, ss, steps, profiled(h, run_sequence, ks, inits, steps, method))
                        margin = (bt["ms_per_step_max"] - bt["ms_per_step_min"]) + (sq["ms_per_step_max"] - sq["ms_per_step_min"])
                        key = f"{pname}/d{density:g}/{names[method]}/{cname}"
                        res["cases"][key] = {"ranks": ks, "density": density, "nnz": int(S[1].size), "steps": steps,
                                             "long_lines": int((lens > short_max).sum()), "lines": int(lens.size),
                                             "forms": [int(h.get_info("sparse_kl_batch_form_w")), int(h.get_info("sparse_kl_batch_form_h"))],
                                             "batch": bt, "sequence": sq,
                                             "batch_over_sequence": round(bt["ms_per_step"] / sq["ms_per_step"], 3),
                                             "batch_wins": bool(sq["ms_per_step"] - bt["ms_per_step"] > margin)}
                        print(key, steps, bt["ms_per_step"], bt["spread"], sq["ms_per_step"], sq["spread"], file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
