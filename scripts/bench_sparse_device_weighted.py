"""A sparse matrix and its per-entry weights in device memory: what nnlm_set_matrix_sparse_device_weighted costs against the host
weighted entry on the same matrix and weights.  One JSON line, written to profiles/sparse_device_weighted_bench.json.

Matrices (canonical on both sides): 20000 x 10000 at 0.1 %, 1 % and 5 % density; 2 000 000 x 50 000 with 5e6 stored entries -- the sizes
of scripts/bench_sparse_device.py.  Weights 1 + 40 u (implicit-feedback confidences).  Both arithmetic modes.

Per matrix and mode, wall time of the whole entry with the device idle before and after (torch.cuda.synchronize around it), one warm-up
call and --reps timed ones, reported as median [min, max]:
  device_s          Handle.set_matrix_sparse_device_weighted on int64 / int64 / fp64 device tensors and fp64 weights aligned with the
                    values, CSC;
  device_csr_s      the same matrix and weights given as CSR;
  device_pattern_s  CSC, the weights as a sparse matrix of their own (int64 pattern): the pattern stage on top;
  host_s            Handle.set_matrix_csc_weighted on canonical host arrays: the host entry alone, the yardstick;
  host_with_fetch_s the route a user with device tensors had: the four arrays to the host, api.as_csc() of the object they form, then
                    set_matrix_csc_weighted.
`stages_ms`: the library's profile scopes around the ingest's kernels, median over the same calls ("sp_ingest_check" now holds the entry
check, the pattern stage and the weight check).
Usage: python scripts/bench_sparse_device_weighted.py [--reps 5] [--skip-large] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_sparse_device import STAGES, Csc, other_side, random_matrix, spread, timed  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_device_weighted_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    specs = [("20000x10000_0.1pct", lambda: random_matrix(20000, 10000, 200000, rng)),
             ("20000x10000_1pct", lambda: random_matrix(20000, 10000, 2000000, rng)),
             ("20000x10000_5pct", lambda: random_matrix(20000, 10000, 10000000, rng))]
    if not args.skip_large:
        specs.append(("2000000x50000_5e6", lambda: random_matrix(2000000, 50000, 5000000, rng)))
    res = {"warmup": 1, "reps": args.reps, "matrices": {}}
    for name, make in specs:
        S = make()
        ptr, idx, val, (n, m) = S
        w = 1.0 + 40.0 * rng.random(idx.size)
        rptr, cidx, rval = other_side(S)
        rw = w[np.argsort(idx, kind="stable")]
        tp, ti, tv, tw = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (ptr, idx.astype(np.int64), val, w))
        rp, ri, rv, rwt = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (rptr, cidx, rval, rw))
        entry = {"n": n, "m": m, "nnz": int(idx.size)}
        for pname, prec in (("f64", _lib.PREC_F64), ("f32", _lib.PREC_F32)):
            with _lib.Handle(0, prec) as h:
                def with_fetch():
                    c = api.as_csc(Csc((tp.cpu().numpy(), ti.cpu().numpy(), tv.cpu().numpy(), (n, m))))
                    h.set_matrix_csc_weighted(*c[:3], tw.cpu().numpy(), c[3])

                r = {"host_s": spread(timed(lambda: h.set_matrix_csc_weighted(ptr, idx, val, w, (n, m)), args.reps)),
                     "host_with_fetch_s": spread(timed(with_fetch, args.reps)),
                     "device_csr_s": spread(timed(lambda: h.set_matrix_sparse_device_weighted(rp, ri, rv, rwt, (n, m), "csr"), args.reps)),
                     "device_pattern_s": spread(timed(lambda: h.set_matrix_sparse_device_weighted(tp, ti, tv, (tp, ti, tw), (n, m), "csc"),
                                                      args.reps))}
                h.profile_enable(True)
                stage = {s: [] for s in STAGES}

                def device():
                    h.profile_reset()
                    h.set_matrix_sparse_device_weighted(tp, ti, tv, tw, (n, m), "csc")
                    for s in STAGES:
                        stage[s].append(h.profile_get(s)[0])

                ts = timed(device, args.reps)
                h.profile_enable(False)
                r["device_s"] = spread(ts)
                r["stages_ms"] = {s: spread(v[1:]) for s, v in stage.items()}
                r["host_over_device"] = round(r["host_s"]["median"] / r["device_s"]["median"], 2)
                r["host_with_fetch_over_device"] = round(r["host_with_fetch_s"]["median"] / r["device_s"]["median"], 2)
                entry[pname] = r
                print(name, pname, json.dumps(r), file=sys.stderr, flush=True)
        res["matrices"][name] = entry
        del tp, ti, tv, tw, rp, ri, rv, rwt
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
