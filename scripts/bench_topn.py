"""Top-N scores and listed entries of a fit without W H (nnlm_top_n / nnlm_predict_entries): device time of
topn_kernel by the library's event scopes, its share of the fp64 matrix rate, and what a user had before (numpy on the host).  One JSON
line, also written to profiles/topn_bench.json.

  * 138 000 x 27 000 at k = 16 and 50, the power-law pattern of scripts/bench_sparse_missing.py (2e7 stored entries) as `seen`;
  * 2 000 000 x 50 000 at k = 8, nothing excluded;
  * N = 10 and 100; all lines and a 1000-line subset; by column and by row;
  * predict_entries: 2e7 listed entries at k = 50;
  * host baseline: numpy W @ H[:, chunk] + argpartition + sort of the N kept, over a 2000-column chunk of the first shape.
Bound of a run: 2 candidates lines K4 fp64 flops at 78.6 TF (v_mfma_f64_16x16x4_f64).
Usage: python scripts/bench_topn.py [--only small|movielens|wide|entries|host] [--no-all-lines] [--no-write] [--out FILE]"""
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
from bench_sparse_missing import power_law_csc  # noqa: E402

F64_MATRIX_TF = 78.6


def top_n_run(h, n, m, k, n_top, by, lines, exclude):
    """One timed nnlm_top_n call: wall seconds, topn_kernel / topn_merge_kernel milliseconds by HIP events, fraction of the bound."""
    h.profile_reset()
    t0 = time.perf_counter()
    idx, score = h.top_n(n_top, by=by, lines=lines, exclude=exclude)
    wall = time.perf_counter() - t0
    ms, launches = h.profile_get("topn")
    ms_merge, _ = h.profile_get("topn_merge")
    L = (m if by == "column" else n) if lines is None else len(lines)
    cand = n if by == "column" else m
    k4 = 4 * ((k + 3) // 4)
    bound_ms = 2.0 * cand * L * k4 / (F64_MATRIX_TF * 1e12) * 1e3
    assert (idx[:, 0] >= 0).all()
    return dict(by=by, n_top=n_top, lines=L, candidates=cand, exclude=bool(exclude), wall_s=round(wall, 4), topn_ms=round(ms, 4),
                topn_launches=launches, topn_merge_ms=round(ms_merge, 4), slices=int(h.get_info("topn_slices")), bound_ms=round(bound_ms, 4),
                fraction_of_f64_matrix_rate=round(bound_ms / ms, 4) if ms > 0 else None)


def shape_runs(name, n, m, k, seen, all_lines, rng):
    W, H = rng.random((n, k)), rng.random((k, m))
    out = dict(shape=[n, m], k=k, nnz_seen=int(seen[1].size) if seen is not None else 0, runs=[])
    with nnlm_amd.Handle(0, _lib.PREC_F32) as h:
        if seen is None:
            h.set_matrix_csc(np.zeros(m + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), (n, m))
        else:
            h.set_matrix_csc(seen[0], seen[1], np.ones(seen[1].size), (n, m))
        h.set_factors(k, W, H)
        h.profile_enable(True)
        h.top_n(10, by="column", lines=[0], exclude=seen is not None)  # (loads the code object)
        for by in ("column", "row"):
            side = m if by == "column" else n
            sub = np.sort(rng.choice(side, size=1000, replace=False))
            for n_top in (10, 100):
                out["runs"].append(top_n_run(h, n, m, k, n_top, by, sub, seen is not None))
                print(name, k, out["runs"][-1], file=sys.stderr, flush=True)
                if all_lines:
                    out["runs"].append(top_n_run(h, n, m, k, n_top, by, None, seen is not None))
                    print(name, k, out["runs"][-1], file=sys.stderr, flush=True)
    return out


def entries_run(n, m, k, count, rng):
    W, H = rng.random((n, k)), rng.random((k, m))
    rows, cols = rng.integers(0, n, size=count).astype(np.int32), rng.integers(0, m, size=count).astype(np.int32)
    with nnlm_amd.Handle(0, _lib.PREC_F32) as h:
        h.set_matrix_csc(np.zeros(m + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), (n, m))
        h.set_factors(k, W, H)
        h.profile_enable(True)
        h.predict_entries(rows[:1000], cols[:1000])
        h.profile_reset()
        t0 = time.perf_counter()
        out = h.predict_entries(rows, cols)
        wall = time.perf_counter() - t0
        ms, launches = h.profile_get("predict_entries")
    e = np.arange(0, count, 9973)
    assert np.allclose(out[e], np.einsum("ek,ke->e", W[rows[e]], H[:, cols[e]]), rtol=1e-12)
    k4 = 4 * ((k + 3) // 4)
    gathered = count * (2.0 * k * 8 + 16)  # the two factor rows' k values, the two indices and the result
    return dict(shape=[n, m], k=k, entries=count, wall_s=round(wall, 4), kernel_ms=round(ms, 4), launches=launches, row_bytes=k4 * 8,
                gathered_GBps=round(gathered / (ms * 1e-3) / 1e9, 1) if ms > 0 else None)


def host_run(n, m, k, n_top, chunk, rng):
    """What a user of predict_nnmf(which = "A") had: the scores of a chunk of columns on the host, then a selection."""
    W, H = rng.random((n, k)), rng.random((k, m))
    t0 = time.perf_counter()
    S = W @ H[:, :chunk]
    t1 = time.perf_counter()
    part = np.argpartition(-S, n_top - 1, axis=0)[:n_top]
    sc_ = np.take_along_axis(S, part, axis=0)
    order = np.lexsort((part, -sc_), axis=0)
    idx = np.take_along_axis(part, order, axis=0).T
    t2 = time.perf_counter()
    return dict(shape=[n, m], k=k, n_top=n_top, lines=chunk, gemm_s=round(t1 - t0, 4), select_s=round(t2 - t1, 4), total_s=round(t2 - t0, 4)), idx, W, H


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("small", "movielens", "wide", "entries", "host"), default=None)
    ap.add_argument("--no-all-lines", action="store_true", help="1000-line subsets only")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topn_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(20251017)
    res = dict(bench="topn", f64_matrix_TF=F64_MATRIX_TF, shapes=[])
    want = lambda s: a.only in (None, s)  # noqa: E731
    if a.only == "small":  # (a quick look: the profiler run of the job script)
        n, m = 20000, 5000
        seen = power_law_csc(n, m, 1000000, rng)
        res["shapes"].append(shape_runs("small", n, m, 16, seen, True, rng))
    if want("movielens"):
        n, m = 138000, 27000
        seen = power_law_csc(n, m, 20000000, rng)
        for k in (16, 50):
            res["shapes"].append(shape_runs("movielens", n, m, k, seen, not a.no_all_lines, rng))
    if want("wide"):
        res["shapes"].append(shape_runs("wide", 2000000, 50000, 8, None, not a.no_all_lines, rng))
    if want("entries"):
        res["predict_entries"] = entries_run(138000, 27000, 50, 20000000, rng)
    if want("host"):
        n, m, k, n_top, chunk = 138000, 27000, 50, 10, 2000
        host, idx_host, W, H = host_run(n, m, k, n_top, chunk, rng)
        with nnlm_amd.Handle(0, _lib.PREC_F32) as h:
            h.set_matrix_csc(np.zeros(m + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), (n, m))
            h.set_factors(k, W, H)
            h.profile_enable(True)
            h.top_n(n_top, lines=[0])
            dev = top_n_run(h, n, m, k, n_top, "column", np.arange(chunk), False)
            idx_dev, _ = h.top_n(n_top, lines=np.arange(chunk))
        host["device"] = dev
        host["same_indices_share"] = float((idx_dev == idx_host).all(axis=1).mean())
        host["host_over_device_wall"] = round(host["total_s"] / dev["wall_s"], 1)
        host["host_over_device_kernel"] = round(host["total_s"] / (dev["topn_ms"] * 1e-3), 1)
        res["host_baseline"] = host
    line = json.dumps(res)
    print(line)
    if not a.no_write:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
