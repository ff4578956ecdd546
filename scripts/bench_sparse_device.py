"""Sparse matrices in device memory: what nnlm_set_matrix_sparse_device costs against the host entry on the same matrix.  One JSON line,
written to profiles/sparse_device_bench.json.

Matrices (values already canonical on both sides: indices ascending in every column, no duplicates): 20000 x 10000 at 0.1 %, 1 % and
5 % density; 2 000 000 x 50 000 with 5e6 stored entries; one power-law pattern of tests/sparse_cases.py (4000 x 3000, about 10 % stored,
column counts ~ 1 / (rank + 3)).  Both arithmetic modes.

Per matrix and mode, wall time of the whole entry with the device idle before and after (torch.cuda.synchronize around it), one warm-up
call and --reps timed ones, reported as median [min, max]:
  device_s          Handle.set_matrix_sparse_device on int64 / int64 / fp64 device tensors (torch's defaults), CSC;
  device_csr_s      the same matrix given as CSR;
  host_s            Handle.set_matrix_csc on canonical host arrays: the host entry alone, the yardstick;
  host_with_tocsc_s the route a user with device tensors had: the three arrays to the host, api.as_csc() of the object they form (the
                    canonicalisation tocsc() callers go through), then set_matrix_csc.
`stages_ms`: the library's profile scopes around the ingest's kernels, median over the same calls -- "sp_ingest" from the first kernel
to the last copy (the host's waits for the verdicts included), and its stages "sp_ingest_ptr", "sp_ingest_check", "sp_ingest_build".
Usage: python scripts/bench_sparse_device.py [--reps 5] [--skip-large]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from nnlm_amd import _lib, api  # noqa: E402
from sparse_cases import _powerlaw, csc_from_flat, csc_from_pattern  # noqa: E402

STAGES = ("sp_ingest", "sp_ingest_ptr", "sp_ingest_check", "sp_ingest_build")


class Csc:
    def __init__(self, S):
        self.indptr, self.indices, self.data, self.shape = S

    def tocsc(self):
        return self


def random_matrix(n, m, nnz, rng):
    flat = np.unique(rng.integers(0, n, size=nnz) + n * rng.integers(0, m, size=nnz))
    return csc_from_flat(flat, rng.random(flat.size) + 0.01, n, m)


def other_side(S):
    ptr, idx, val, (n, m) = S
    cols = np.repeat(np.arange(m, dtype=np.int64), np.diff(ptr))
    order = np.argsort(idx, kind="stable")
    rptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(idx, minlength=n), out=rptr[1:])
    return rptr, cols[order], val[order]


def spread(ts):
    return {"median": round(statistics.median(ts), 6), "min": round(min(ts), 6), "max": round(max(ts), 6)}


def timed(fn, reps):
    ts = []
    for _ in range(reps + 1):  # the first call is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_device_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    specs = [("20000x10000_0.1pct", lambda: random_matrix(20000, 10000, 200000, rng)),
             ("20000x10000_1pct", lambda: random_matrix(20000, 10000, 2000000, rng)),
             ("20000x10000_5pct", lambda: random_matrix(20000, 10000, 10000000, rng)),
             ("powerlaw_4000x3000", lambda: csc_from_pattern(_powerlaw(4000, 3000, rng, False), rng.random((4000, 3000)) + 0.01))]
    if not args.skip_large:
        specs.append(("2000000x50000_5e6", lambda: random_matrix(2000000, 50000, 5000000, rng)))
    res = {"warmup": 1, "reps": args.reps, "matrices": {}}
    for name, make in specs:
        S = make()
        ptr, idx, val, (n, m) = S
        rptr, cidx, rval = other_side(S)
        tp, ti, tv = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (ptr, idx.astype(np.int64), val))
        rp, ri, rv = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (rptr, cidx, rval))
        entry = {"n": n, "m": m, "nnz": int(idx.size)}
        for pname, prec in (("f64", _lib.PREC_F64), ("f32", _lib.PREC_F32)):
            with _lib.Handle(0, prec) as h:
                def with_tocsc():
                    c = api.as_csc(Csc((tp.cpu().numpy(), ti.cpu().numpy(), tv.cpu().numpy(), (n, m))))
                    h.set_matrix_csc(*c)

                r = {"host_s": spread(timed(lambda: h.set_matrix_csc(ptr, idx, val, (n, m)), args.reps)),
                     "host_with_tocsc_s": spread(timed(with_tocsc, args.reps)),
                     "device_csr_s": spread(timed(lambda: h.set_matrix_sparse_device(rp, ri, rv, (n, m), "csr"), args.reps))}
                h.profile_enable(True)
                stage = {s: [] for s in STAGES}
                ts = []

                def device():
                    h.profile_reset()
                    h.set_matrix_sparse_device(tp, ti, tv, (n, m), "csc")
                    for s in STAGES:
                        stage[s].append(h.profile_get(s)[0])

                ts = timed(device, args.reps)
                h.profile_enable(False)
                r["device_s"] = spread(ts)
                r["stages_ms"] = {s: spread(v[1:]) for s, v in stage.items()}
                r["host_over_device"] = round(r["host_s"]["median"] / r["device_s"]["median"], 2)
                r["host_with_tocsc_over_device"] = round(r["host_with_tocsc_s"]["median"] / r["device_s"]["median"], 2)
                entry[pname] = r
                print(name, pname, json.dumps(r), file=sys.stderr, flush=True)
        res["matrices"][name] = entry
        del tp, ti, tv, rp, ri, rv
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
