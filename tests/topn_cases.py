"""Cases and the numpy restatement for the top-N / listed-entry scores (tests/test_topn_host.py, tests/test_gpu_topn.py): numpy only,
importable without a GPU, deterministic.

topn_oracle is the definition: S = W @ H, stored entries of `seen` removed, NaN never selected, then per line a stable argsort on
(-score, index) -- (score descending, index ascending) is a total order -- and (-1, NaN) behind a line with fewer candidates.

tau(W, H) is the bound on the distance between two fp64 evaluations of one score that sum its k products in different orders:
tau_ij = 4 k eps sum_q |w_iq h_qj| (each of the two is within (k + 1) eps sum |w h| of the exact sum to first order, k >= 1).

A line of a random case is EXEMPT from index equality with the oracle only when two consecutive oracle scores among its best N + 1
candidates are 2 tau or less apart (either evaluation may then order them the other way); exempt_share counts such lines from the oracle
alone."""
import numpy as np

import sparse_cases as sc

EPS = np.finfo(np.float64).eps

# (n, m, k, N) of the random family (U(0, 1) factors)
RANDOM_SHAPES = ((3000, 500, 8, 10), (20000, 300, 50, 20), (500, 3000, 3, 64), (4000, 400, 70, 10))
BYS = ("column", "row")


def pattern_lists(seen, n, m):
    """Boolean n x m pattern of a CSC tuple (indptr, indices, data, shape), or None."""
    if seen is None:
        return None
    assert tuple(seen[3]) == (n, m)
    return sc.pattern_of(seen)


def topn_oracle(W, H, n_top, by="column", lines=None, seen=None):
    """(idx int32 [L, n_top], score float64 [L, n_top]) by the definition; seen: a CSC tuple whose stored entries are excluded."""
    S = np.asarray(W, dtype=np.float64) @ np.asarray(H, dtype=np.float64)
    n, m = S.shape
    P = pattern_lists(seen, n, m)
    if by == "row":
        S, P = S.T, (None if P is None else P.T)
    elif by != "column":
        raise ValueError(by)
    # S[c, l]: score of candidate c on line l
    ls = np.arange(S.shape[1]) if lines is None else np.asarray(lines, dtype=np.int64)
    idx = np.full((ls.size, n_top), -1, dtype=np.int32)
    score = np.full((ls.size, n_top), np.nan)
    for r, l in enumerate(ls):
        s = S[:, l]
        ok = ~np.isnan(s)
        if P is not None:
            ok &= ~P[:, l]
        cand = np.flatnonzero(ok)
        order = cand[np.argsort(-s[cand], kind="stable")][:n_top]  # (cand ascends: stable = ties by ascending index)
        idx[r, :order.size] = order
        score[r, :order.size] = s[order]
    return idx, score


def tau(W, H):
    """tau_ij as an n x m array."""
    return 4.0 * W.shape[1] * EPS * (np.abs(W) @ np.abs(H))


def exempt_lines(W, H, n_top, by, seen=None):
    """Boolean per line (all lines of the side): two consecutive oracle scores among its best n_top + 1 are within 2 tau."""
    idx, score = topn_oracle(W, H, n_top + 1, by, None, seen)
    T = tau(W, H)
    if by == "row":
        T = T.T
    out = np.zeros(idx.shape[0], dtype=bool)
    for l in range(idx.shape[0]):
        have = idx[l] >= 0
        s, t = score[l, have], T[idx[l, have], l]
        if s.size > 1:
            out[l] = bool(np.any(s[:-1] - s[1:] <= 2.0 * np.maximum(t[:-1], t[1:])))
    return out


def smallest_gap(W, H, n_top, by, seen=None):
    """(smallest gap between consecutive oracle scores among the best n_top + 1 of any line, largest tau of an entry)."""
    idx, score = topn_oracle(W, H, n_top + 1, by, None, seen)
    d = score[:, :-1] - score[:, 1:]
    return float(np.nanmin(d)) if np.any(~np.isnan(d)) else np.inf, float(tau(W, H).max())


def random_case(i):
    """Random case i: U(0, 1) factors and a 5 % uniform `seen` pattern."""
    n, m, k, N = RANDOM_SHAPES[i]
    rng = np.random.default_rng(77000 + i)
    W, H = rng.random((n, k)), rng.random((k, m))
    seen = sc.csc_from_pattern(rng.random((n, m)) < 0.05, np.ones((n, m)))
    return dict(W=W, H=H, k=k, N=N, seen=seen, n=n, m=m)


def integer_factors(n, m, k, rng):
    """Small non-negative integers (0 .. 7): every score is an exact integer in fp64 whatever the summation order; ties are plentiful."""
    return rng.integers(0, 8, size=(n, k)).astype(np.float64), rng.integers(0, 8, size=(k, m)).astype(np.float64)


def exact_patterns():
    """[(name, CSC tuple)] of the `seen` patterns of the exact family: the powerlaw, heavy, empty_lines and boundary patterns of
    sparse_cases, plus a column and a row whose every entry is stored next to nearly empty ones."""
    rng = np.random.default_rng(5150)
    n, m = 300, 200
    ones = np.ones((n, m))
    out = [("powerlaw", sc.csc_from_pattern(sc._powerlaw(n, m, rng, False), ones)),
           ("powerlaw_rows", sc.csc_from_pattern(sc._powerlaw(n, m, rng, True), ones)),
           ("heavy", sc.csc_from_pattern(sc._heavy(n, m, rng), ones)),
           ("empty_lines", sc.csc_from_pattern(sc._empty_lines(n, m, rng), ones))]
    P = rng.random((n, m)) < 0.1
    P[:, 8] = False
    P[12, :] = False
    P[:, 7] = True   # a column whose every entry is stored: nothing is left to select (column 8 keeps one entry, row 12 one)
    P[11, :] = True  # and such a row
    out.append(("full_line", sc.csc_from_pattern(P, ones)))
    cases = sc.boundary_cases("missing")
    for c in (cases[0], cases[1], cases[-2], cases[-1]):  # chunk_edges and segment_counts, each with its transpose
        out.append(("boundary_" + c["name"], c["S"]))
    return out


EXACT_RANKS = (1, 3, 16, 50, 65, 70, 100)
EXACT_NTOPS = (1, 10, 64, 128)
