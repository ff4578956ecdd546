"""Matrices in device memory: what nnlm_set_matrix_device costs per route, and what a whole api.nnmf call gains from it.  One JSON line,
written to profiles/device_io_bench.json.

Ingest: 20000 x 10000, routes column (row_stride 1), row (col_stride 1, the transposition through LDS) and gather (general strides),
source types fp64 / fp32 / fp16 / bf16, both arithmetic modes.  `kernel_ms`: HIP events on the handle's stream around the ingest kernels
(the library's "ingest" profile scope), best of the repetitions; `bytes` = n m (sizeof(S) + sizeof(T)) + n m / 8 is what the pass moves
(the gather route touches more: whole sectors for single elements), `fraction_of_peak` = bytes / kernel time / 6.29 TB/s.  `call_s`:
wall time of the whole entry (allocation, ingest, readback of the sums, and in the F32 mode the split copies of the common tail).
Whole call: api.nnmf(A_dev, 50, max_iter = 20 and 200, rel_tol = -1) against the same call on A_dev.cpu().double().numpy() with that
conversion inside the timed region, alternating, after one warm-up of each; both get the same explicit host init (the default init is
drawn element by element through a Python callback on the host route: seconds that have nothing to do with where A lives).
Usage: python scripts/bench_device_io.py [--reps 3]"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnlm_amd import _lib, api  # noqa: E402

PEAK = 6.29e12  # achievable copy rate, DESIGN section 5


def layouts(a):
    n, m = a.shape
    f = torch.empty_strided((n, m), (1, n), dtype=a.dtype, device=a.device)
    f.copy_(a)
    big = torch.zeros((n, 2 * m), dtype=a.dtype, device=a.device)
    g = big[:, ::2]
    g.copy_(a)
    return {"column": f, "row": a.contiguous(), "gather": g}


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "device_io_bench.json"))
    args = ap.parse_args()
    n, m = args.n, args.m
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    base = torch.rand((n, 10), device=dev, dtype=torch.float64, generator=gen) @ torch.rand((10, m), device=dev, dtype=torch.float64, generator=gen)
    base += 0.1 * torch.rand((n, m), device=dev, dtype=torch.float64, generator=gen)
    res = {"n": n, "m": m, "peak_bytes_per_s": PEAK, "ingest": {}, "whole_call": {}}
    for pname, prec in (("f32", _lib.PREC_F32), ("f64", _lib.PREC_F64)):
        tsz = 4 if prec == _lib.PREC_F32 else 8
        with _lib.Handle(0, prec) as h:
            host = base.cpu().numpy()
            ts = timed(lambda: h.set_matrix(host), args.reps + 1)[1:]
            res["ingest"][f"{pname}/host_upload_fp64"] = {"min_s": round(min(ts), 5)}
            del host
            for dname in ("float64", "float32", "float16", "bfloat16"):
                a = base.to(getattr(torch, dname))
                for route, x in layouts(a).items():
                    h.set_matrix_device(x)  # warm
                    h.profile_enable(True)
                    ts, ks = [], []
                    for _ in range(args.reps):
                        h.profile_reset()
                        ts += timed(lambda: h.set_matrix_device(x), 1)
                        ks.append(h.profile_get("ingest")[0])
                    h.profile_enable(False)
                    nbytes = n * m * (a.element_size() + tsz) + n * m // 8
                    t = min(ks) * 1e-3
                    res["ingest"][f"{pname}/{route}/{dname}"] = {"kernel_ms": round(min(ks), 4), "call_s": round(min(ts), 5), "bytes": nbytes,
                                                                 "fraction_of_peak": round(nbytes / t / PEAK, 4)}
                    print(pname, route, dname, round(min(ks), 4), round(min(ts), 5), file=sys.stderr, flush=True)
                    del x
                del a
    torch.cuda.empty_cache()
    warnings.simplefilter("ignore", RuntimeWarning)
    irng = np.random.default_rng(2)
    init = {"W": 0.01 * irng.random((n, 50)), "H": 0.01 * irng.random((50, m))}
    for pname in ("f64", "f32"):
        os.environ["NNLM_PRECISION"] = pname
        for dname in ("float64", "float32"):
            a = base.to(getattr(torch, dname)).contiguous()
            for iters in (20, 200):
                kw = dict(max_iter=iters, rel_tol=-1, show_warning=False, init=init)
                dev_call = lambda: api.nnmf(a, 50, rng=np.random.default_rng(1), **kw)  # noqa: E731
                host_call = lambda: api.nnmf(a.cpu().double().numpy(), 50, rng=np.random.default_rng(1), **kw)  # noqa: E731
                dev_call(), host_call()  # warm
                td, th = [], []
                for _ in range(args.reps):  # alternating
                    td += timed(dev_call, 1)
                    th += timed(host_call, 1)
                res["whole_call"][f"{pname}/{dname}/max_iter_{iters}"] = {
                    "device_s": round(min(td), 4), "host_s": round(min(th), 4), "device_over_host": round(min(td) / min(th), 3),
                    "device_all_s": [round(v, 4) for v in td], "host_all_s": [round(v, 4) for v in th]}
                print(pname, dname, iters, min(td), min(th), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
