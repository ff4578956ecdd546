"""KL loss on a sparse A (nnlm_set_matrix_csc_kl, k_sparse_kl.h): ms per outer iteration and per phase next to the dense KL path on the
same densified matrix in the same build; one JSON line, also written to profiles/sparse_kl_bench.json.

  20000 x 10000, k = 50, Poisson counts of a planted model on a uniform pattern of 0.1 %, 1 % and 5 % density (zeros dropped from the
  structure), both arithmetic modes, both KL methods, R's defaults for KL (inner_max_iter = 1, trace = 100: no error block inside the
  timed loop; the error block is timed by itself).

Protocol: one sparse and one dense handle per (density, mode), warmed with the shapes and the method they are timed on; a timed window is
`steps` outer iterations of nnlm_run() (dense: steps / 5, at least 4 -- its step is 10 to 100 times longer) between two device
synchronisations, timed by the host clock (the library exposes HIP events per kernel scope, not per run; a window is tens of
milliseconds of device work ended by a synchronise); sparse and dense windows alternate (`reps` of each) and the median is reported with
every window; the phases come from the library's HIP-event scopes (nnlm_profile_get) in a separate, profiled run.  The starting states are formed in the solver's
prologue, so they are part of "solver".

The per-non-zero VALU floor: vector instructions per stored entry and coordinate step of the solver's inner loop (counted from
k_sparse_kl.h: quotient, products, fp64 sums, the rank-1 refresh of the state), priced at the issue cycles of one wave64 instruction on a
SIMD-32 (fp32 2, v_rcp_f32 4, fp64 and conversions 4 -- half rate), on 1024 SIMDs at 2.4 GHz, for the two half-steps of an iteration.
Gathers, index loads and reductions are not in it: it is a floor of the arithmetic alone.
Usage: python scripts/bench_sparse_kl.py [--steps 50] [--warmup 5] [--reps 5] [--densities 0.001,0.01,0.05] [--no-write]"""
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

N, M, K = 20000, 10000, 50
INNER, INNER_TOL = 1, 1e-9
PHASES_SPARSE = ["spkl_copy", "spkl_solve_h", "spkl_solve_w"]
PHASES_DENSE = ["sweep_h", "sweep_w"]
# issue cycles of a wave64 instruction stream per stored entry and coordinate step: (fp32 mode, strict mode), method 3 / 4
#   fp32 SCD: add, abs-in-rcp, rcp(4), 2 mul, 2 cvt(4), mul_f64(4), 2 add/fma_f64(4) = 2+4+2+2+8+4+8 = 30; refresh: 2 cvt + fma_f64 + cvt = 16
#   fp32 Lee: add, rcp(4), 2 mul, cvt(4), add_f64(4) = 18; refresh 16
#   strict: add_f64, the IEEE quotient (~14 fp64 instructions), 2-4 mul/fma_f64; refresh: fma_f64
FLOOR_CYCLES = {("f32", 3): 46, ("f32", 4): 34, ("f64", 3): 4 * 20, ("f64", 4): 4 * 18}
SIMDS, CLOCK = 1024, 2.4e9


def counts_csc(density, rng):
    Wp, Hp = rng.random((N, 8)) ** 2 + 0.05, rng.random((8, M)) ** 2 + 0.05
    nnz = int(density * N * M)
    flat = np.unique(rng.integers(0, N * M, size=nnz, dtype=np.int64))
    cols, rows = flat // N, flat % N
    lam = np.einsum("ek,ke->e", Wp[rows], Hp[:, cols])
    v = rng.poisson(lam * (4.0 / lam.mean())).astype(np.float64)
    keep = v > 0
    cols, rows, v = cols[keep], rows[keep], v[keep]
    indptr = np.zeros(M + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=M), out=indptr[1:])
    return indptr, rows.astype(np.int32), v, (N, M)


def dense_of(csc):
    indptr, idx, val, (n, m) = csc
    A = np.zeros((n, m), order="F")
    A[idx, np.repeat(np.arange(m), np.diff(indptr))] = val
    return A


class Side:
    """One resident handle (sparse or dense) with its factors, timed in windows."""

    def __init__(self, prec, W0, H0, csc=None, A=None):
        self.h = nnlm_amd.Handle(0, prec)
        self.method, self.W0, self.H0 = 4, W0, H0
        self.sparse = csc is not None
        self.h.set_matrix_csc_kl(*csc) if self.sparse else self.h.set_matrix(A)
        self.bytes = self.h.get_info("matrix_bytes")

    def window(self, steps):
        z = [0.0, 0.0, 0.0]
        self.h.sync()
        t0 = time.perf_counter()
        self.h.run(z, z, steps, -1.0, 0, False, INNER, INNER_TOL, self.method, 100)
        self.h.sync()
        return 1e3 * (time.perf_counter() - t0) / steps

    def reset(self):
        self.h.set_factors(K, self.W0, self.H0)

    def phases(self, steps, warmup):
        self.reset()
        self.window(warmup)
        self.h.profile_enable(True)
        self.h.profile_reset()
        self.window(steps)
        out = {p: round(self.h.profile_get(p)[0] / steps, 4) for p in (PHASES_SPARSE if self.sparse else PHASES_DENSE) if self.h.profile_get(p)[1] > 0}
        self.h.profile_reset()
        for _ in range(5):
            self.h.errors()
        name = "sp_errors" if self.sparse else "errors"
        out["error_block"] = round(self.h.profile_get(name)[0] / max(1, self.h.profile_get(name)[1]), 4)
        self.h.profile_enable(False)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--densities", default="0.001,0.01,0.05")
    ap.add_argument("--methods", default="4,3")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    res = {"config": {"n": N, "m": M, "k": K, "inner_max_iter": INNER, "steps": args.steps, "warmup": args.warmup, "reps": args.reps}, "cases": []}
    rng = np.random.default_rng(0)
    W0, H0 = rng.random((N, K)) * 0.1 + 0.01, rng.random((K, M)) * 0.1 + 0.01
    for density in (float(v) for v in args.densities.split(",")):
        csc = counts_csc(density, rng)
        A = dense_of(csc)
        nnz = int(csc[2].size)
        rows = np.bincount(csc[1], minlength=N)
        for pname, prec in (("f32", _lib.PREC_F32), ("f64", _lib.PREC_F64)):
            sp, de = Side(prec, W0, H0, csc=csc), Side(prec, W0, H0, A=A)
            dsteps = max(4, args.steps // 5)
            for method in (int(v) for v in args.methods.split(",")):
                sp.method = de.method = method
                t = {"sparse": [], "dense": []}
                for side in (sp, de):
                    side.reset()
                    side.window(args.warmup)
                for _ in range(args.reps):  # alternating windows
                    t["sparse"].append(sp.window(args.steps))
                    t["dense"].append(de.window(dsteps))
                ms_s, ms_d = float(np.median(t["sparse"])), float(np.median(t["dense"]))
                floor_ms = 2 * nnz * K * FLOOR_CYCLES[(pname, method)] / 64.0 / SIMDS / CLOCK * 1e3
                case = {"density": density, "nnz": nnz, "precision": pname, "method": method,
                        "longest_column": int(np.diff(csc[0]).max()), "longest_row": int(rows.max()),
                        "forms_w_h": [sp.h.get_info("sparse_kl_form_w"), sp.h.get_info("sparse_kl_form_h")],
                        "sparse_ms_per_step": round(ms_s, 4), "dense_ms_per_step": round(ms_d, 4),
                        "sparse_windows": [round(v, 4) for v in t["sparse"]], "dense_windows": [round(v, 4) for v in t["dense"]],
                        "sparse_over_dense": round(ms_s / ms_d, 4), "matrix_bytes_sparse": sp.bytes, "matrix_bytes_dense": de.bytes,
                        "valu_floor_ms_per_step": round(floor_ms, 5), "fraction_of_valu_floor": round(floor_ms / ms_s, 4),
                        "sparse_phase_ms": sp.phases(args.steps, args.warmup), "dense_phase_ms": de.phases(dsteps, args.warmup)}
                res["cases"].append(case)
                print(json.dumps(case), file=sys.stderr, flush=True)
            sp.h.close()
            de.h.close()
        del A
    line = json.dumps(res)
    print(line)
    if not args.no_write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "sparse_kl_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
