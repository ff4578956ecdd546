"""Cases and the numpy restatement for ranking evaluation of top-N lists against held-out entries (tests/test_topn_eval_host.py,
tests/test_gpu_topn_eval.py): numpy and plain Python only, importable without a GPU, deterministic.

eval_oracle is the definition, working from index lists (whoever made them).  For a line with held-out set T (t = |T|), list
L[0 .. n_top) (padding -1 never hits) and cutoff c:
  hits_c = #{p < c : L[p] in T};  first = the smallest p with L[p] in T, or -1
  dcg_c  = sum over hits p < c of d[p], d[p] = 1 / log2(p + 2), terms in ascending p
  apn_c  = sum over hits p < c of hits_{p+1} / (p + 1), in ascending p
  precision = hits_c / c, recall = hits_c / t, hit rate = [hits_c > 0], NDCG = dcg_c / sum_{p < min(c, t)} d[p],
  AP = apn_c / min(c, t), RR = 1 / (first + 1) if 0 <= first < c else 0
A line is evaluated iff t > 0; the aggregates are the means over the evaluated lines (NaN when there is none).

Floats compare at RTOL: the library's d[p] comes from the C library's log2 and numpy's from its own (an ulp or two apart), and the means
are summed in another order -- each a few eps on sums of at most 128 terms of like sign, far inside 1e-13."""
import math

import numpy as np

import sparse_cases as sc
import topn_cases as tc

RTOL = 1e-13
METRICS = ("precision", "recall", "hit_rate", "ndcg", "map", "mrr")  # columns of the aggregate, in the library's order


def discount(p):
    return 1.0 / math.log2(p + 2.0)


def eval_oracle(idx_lists, held_sets, cutoffs):
    """idx_lists: [L][n_top] indices (-1 = padding); held_sets: L sets (or sorted arrays) of held-out indices; cutoffs ascending, the
    last one <= n_top.  Returns dict(t, first int64 [L]; hits int64, dcg, apn float64 [L, n_cut]; agg float64 [n_cut, 6]; n_evaluated)."""
    cutoffs = [int(c) for c in cutoffs]
    L, nc = len(idx_lists), len(cutoffs)
    t, first = np.zeros(L, dtype=np.int64), np.full(L, -1, dtype=np.int64)
    hits, dcg, apn = np.zeros((L, nc), dtype=np.int64), np.zeros((L, nc)), np.zeros((L, nc))
    sums, n_eval = [[0.0] * 6 for _ in cutoffs], 0
    for l in range(L):
        T = set(int(v) for v in held_sets[l])
        lst = [int(v) for v in idx_lists[l]]
        assert len(lst) >= cutoffs[-1]
        t[l] = len(T)
        hit_at = [p for p, v in enumerate(lst) if v >= 0 and v in T]
        if hit_at:
            first[l] = hit_at[0]
        for q, c in enumerate(cutoffs):
            h, d, a = 0, 0.0, 0.0
            for p in hit_at:  # (ascending)
                if p < c:
                    h += 1
                    d += discount(p)
                    a += h / (p + 1.0)
            hits[l, q], dcg[l, q], apn[l, q] = h, d, a
        if not T:
            continue
        n_eval += 1
        for q, c in enumerate(cutoffs):
            best = min(c, len(T))
            ideal = 0.0
            for p in range(best):
                ideal += discount(p)
            rr = 1.0 / (first[l] + 1.0) if 0 <= first[l] < c else 0.0
            vals = (hits[l, q] / c, hits[l, q] / len(T), 1.0 if hits[l, q] > 0 else 0.0, dcg[l, q] / ideal, apn[l, q] / best, rr)
            for s in range(6):
                sums[q][s] += vals[s]
    agg = np.array(sums) / n_eval if n_eval else np.full((nc, 6), np.nan)
    return dict(t=t, first=first, hits=hits, dcg=dcg, apn=apn, agg=agg, n_evaluated=n_eval)


# ---- held-out patterns -------------------------------------------------------------------------------------------------------------------
def oriented(P, by):
    """(ptr int64, idx int32) of a boolean n x m pattern in the orientation of `by`: CSC for "column", CSR for "row"."""
    S = sc.csc_from_pattern(P if by == "column" else P.T, np.ones(P.shape if by == "column" else P.T.shape))
    return np.ascontiguousarray(S[0], dtype=np.int64), np.ascontiguousarray(S[1], dtype=np.int32)


def held_sets(ptr, idx, lines):
    """The held-out index arrays of the listed lines (lines = None: all)."""
    ls = range(ptr.size - 1) if lines is None else lines
    return [idx[ptr[l]:ptr[l + 1]] for l in ls]


def random_held(n, m, rng, density=0.08, avoid=None):
    """A boolean n x m held-out pattern disjoint from `avoid` (a boolean pattern or None); a few lines of either side keep nothing."""
    P = rng.random((n, m)) < density
    P[:, rng.choice(m, size=max(1, m // 10), replace=False)] = False
    P[rng.choice(n, size=max(1, n // 10), replace=False), :] = False
    if avoid is not None:
        P &= ~avoid
    return P


# ---- the consistency family (a): factors x `seen` pattern -----------------------------------------------------------------------------
def consistency_cases():
    """[(name, W, H, seen CSC tuple, seen boolean pattern)]: U(0, 1) factors at 300 x 200, k = 7, and integer factors (runs of tied
    scores) at 90 x 70, k = 3, each with the powerlaw and the empty_lines pattern of sparse_cases as the stored matrix."""
    out = []
    for fam, (n, m, k) in (("uniform", (300, 200, 7)), ("integer", (90, 70, 3))):
        for pname, maker in (("powerlaw", lambda n, m, r: sc._powerlaw(n, m, r, False)), ("empty_lines", sc._empty_lines)):
            rng = np.random.default_rng(8800 + len(out))
            W, H = (rng.random((n, k)), rng.random((k, m))) if fam == "uniform" else tc.integer_factors(n, m, k, rng)
            P = maker(n, m, rng)
            out.append((fam + "-" + pname, W, H, sc.csc_from_pattern(P, np.ones((n, m))), P))
    return out


# ---- nnlm_top_n must not move (i): three calls whose idx and scores are recorded under tests/golden ---------------------------------------
GOLDEN_FILE = "topn_parent_lists.npz"


def golden_calls():
    """[(key, case index of consistency_cases(), precision name, by, n_top, lines or None, exclude)]"""
    return [("uniform_powerlaw_f64_column_n20_excl", 0, "f64", "column", 20, None, True),
            ("integer_powerlaw_f32_row_n10", 2, "f32", "row", 10, None, False),
            ("uniform_empty_f32_row_n65_excl_lines", 1, "f32", "row", 65, np.arange(0, 300, 3), True)]


def golden_run(call):
    """(idx, score) of nnlm_top_n for one of golden_calls() on device 0 -- the code that recorded the fixture and the code that checks it."""
    import nnlm_amd
    from nnlm_amd import _lib
    _, ci, mode, by, n_top, lines, exclude = call
    _, W, H, seen, _ = consistency_cases()[ci]
    with nnlm_amd.Handle(0, _lib.PREC_F64 if mode == "f64" else _lib.PREC_F32) as h:
        h.set_matrix_csc(*seen)
        h.set_factors(W.shape[1], W, H)
        return h.top_n(n_top, by=by, lines=lines, exclude=exclude)
