"""Ranking evaluation of top-N lists on the device (nnlm_top_n_eval) against what a user had before: nnlm_top_n for
the same lines, the lists copied to the host, and the same metrics there in numpy.  Per run: wall seconds of both ways (median of five alternating calls), the device time
of topn_kernel, topn_merge_kernel and the evaluation kernels by the library's event scopes ("topn", "topn_merge", "topn_eval"), and the
largest relative difference between the two ways' means.  One JSON line, also written to profiles/topn_eval_bench.json.

  * 138 000 x 27 000 at k = 16 and 50 (the shapes of scripts/bench_topn.py), its power-law pattern of 2e7 stored entries split by
    api.holdout_split (5 entries per column held out): the rest is `seen`;
  * N = 10 and 100 (cutoffs 1, 5, N); a 1000-line subset and all lines; by column and by row.
Usage: python scripts/bench_topn_eval.py [--only small|movielens] [--no-all-lines] [--no-write] [--out FILE]"""
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
from nnlm_amd import _lib, api  # noqa: E402
from bench_sparse_missing import power_law_csc  # noqa: E402


REPS = 5  # calls per configuration and way, alternating; the medians and the last call's scopes are reported


def host_metrics(lists, ptr, idx, lines, cutoffs, ncand):
    """The means of nnlm_top_n_eval from index lists, in numpy: [n_cut][6] and the number of evaluated lines."""
    L, N = lists.shape
    ls = np.arange(L, dtype=np.int64) if lines is None else np.asarray(lines, dtype=np.int64)
    t = (ptr[ls + 1] - ptr[ls]).astype(np.int64)
    keys = np.repeat(np.arange(ptr.size - 1, dtype=np.int64), np.diff(ptr)) * ncand + idx  # (ascending: lines, then indices)
    want = ls[:, None] * ncand + lists
    at = np.minimum(np.searchsorted(keys, want), max(keys.size - 1, 0))
    hit = (lists >= 0) & (keys[at] == want) if keys.size else np.zeros(lists.shape, dtype=bool)
    ev = t > 0
    disc = 1.0 / np.log2(np.arange(N) + 2.0)
    ideal = np.concatenate(([0.0], np.cumsum(disc)))
    run = np.cumsum(hit, axis=1)
    first = np.where(hit.any(axis=1), hit.argmax(axis=1), -1)
    out = np.full((len(cutoffs), 6), np.nan)
    if not ev.any():
        return out, 0
    te = t[ev]
    for q, c in enumerate(cutoffs):
        h = run[ev, c - 1]
        best = np.minimum(c, te)
        dcg = (hit[ev, :c] * disc[:c]).sum(axis=1)
        apn = (hit[ev, :c] * run[ev, :c] / np.arange(1, c + 1)).sum(axis=1)
        f = first[ev]
        rr = np.where((f >= 0) & (f < c), 1.0 / (np.maximum(f, 0) + 1.0), 0.0)
        out[q] = [np.mean(h / c), np.mean(h / te), np.mean(h > 0), np.mean(dcg / ideal[best]), np.mean(apn / best), np.mean(rr)]
    return out, int(ev.sum())


def one_run(h, n, m, by, n_top, lines, held):
    cutoffs = (1, 5, n_top)
    ptr, idx = held[by]
    ncand = n if by == "column" else m
    walls_eval, walls_topn = [], []
    for _ in range(REPS):  # (alternating: whichever call comes first in a new configuration pays for the first large allocations)
        h.profile_reset()
        t0 = time.perf_counter()
        out = h.top_n_eval(cutoffs, by=by, lines=lines, exclude=True, held_ptr=ptr, held_idx=idx)
        walls_eval.append(time.perf_counter() - t0)
        scopes = {s: h.profile_get(s) for s in ("topn", "topn_merge", "topn_eval")}
        h.profile_reset()
        t0 = time.perf_counter()
        lists, _ = h.top_n(n_top, by=by, lines=lines, exclude=True)
        walls_topn.append(time.perf_counter() - t0)
        topn_alone_ms = h.profile_get("topn")[0]
    wall_eval, wall_topn = float(np.median(walls_eval)), float(np.median(walls_topn))
    t0 = time.perf_counter()
    agg, n_eval = host_metrics(lists, ptr, idx, lines, cutoffs, ncand)
    wall_host = time.perf_counter() - t0
    dev = np.stack([out[k] for k in ("precision", "recall", "hit_rate", "ndcg", "map", "mrr")], axis=1)
    assert n_eval == out["n_evaluated"], (n_eval, out["n_evaluated"])
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(dev - agg) / np.abs(agg)
    return dict(by=by, n_top=n_top, lines=int(lists.shape[0]), evaluated=n_eval, eval_wall_s=round(wall_eval, 4),
                eval_walls_s=[round(w, 4) for w in walls_eval], top_n_walls_s=[round(w, 4) for w in walls_topn],
                topn_ms=round(scopes["topn"][0], 4), topn_merge_ms=round(scopes["topn_merge"][0], 4), topn_eval_ms=round(scopes["topn_eval"][0], 4),
                topn_eval_launches=scopes["topn_eval"][1], top_n_wall_s=round(wall_topn, 4), top_n_topn_ms=round(topn_alone_ms, 4),
                host_metrics_s=round(wall_host, 4), lists_bytes=int(lists.shape[0]) * n_top * 12,
                eval_over_topn_kernel=round(scopes["topn_eval"][0] / scopes["topn"][0], 5) if scopes["topn"][0] > 0 else None,
                max_rel_diff_of_means=float(np.nanmax(rel)) if np.isfinite(rel).any() else 0.0, ndcg=[float(v) for v in out["ndcg"]])


def shape_runs(name, n, m, k, stored, all_lines, rng):
    W, H = rng.random((n, k)), rng.random((k, m))
    A = api.CSC(stored[0], stored[1], np.ones(stored[1].size), (n, m))
    train, heldout = api.holdout_split(A, per_line=5, by="column", min_keep=1, rng=rng)
    held = dict(column=(heldout.indptr, heldout.indices), row=api._csc_transposed(heldout)[:2])
    out = dict(shape=[n, m], k=k, nnz_seen=int(train.indices.size), nnz_heldout=int(heldout.indices.size), runs=[])
    with nnlm_amd.Handle(0, _lib.PREC_F32) as h:
        h.set_matrix_csc(train.indptr, train.indices, train.data, (n, m))
        h.set_factors(k, W, H)
        h.profile_enable(True)
        h.top_n_eval((1,), by="column", lines=[0], exclude=True, held_ptr=held["column"][0], held_idx=held["column"][1])  # (loads the code object)
        for by in ("column", "row"):
            side = m if by == "column" else n
            sub = np.sort(rng.choice(side, size=1000, replace=False))
            for n_top in (10, 100):
                for lines in ((sub, None) if all_lines else (sub,)):
                    out["runs"].append(one_run(h, n, m, by, n_top, lines, held))
                    print(name, k, out["runs"][-1], file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("small", "movielens"), default="movielens")
    ap.add_argument("--no-all-lines", action="store_true", help="1000-line subsets only")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topn_eval_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(20261021)
    res = dict(bench="topn_eval", scopes=["topn", "topn_merge", "topn_eval"], shapes=[])
    if a.only == "small":  # (a quick look)
        n, m = 20000, 5000
        res["shapes"].append(shape_runs("small", n, m, 16, power_law_csc(n, m, 1000000, rng), not a.no_all_lines, rng))
    else:
        n, m = 138000, 27000
        stored = power_law_csc(n, m, 20000000, rng)
        for k in (16, 50):
            res["shapes"].append(shape_runs("movielens", n, m, k, stored, not a.no_all_lines, rng))
    print(json.dumps(res))
    if not a.no_write:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
