"""Cases of the batched factorisation on a sparse A (tests/test_gpu_sparse_batch.py) and the conditions on them
(tests/test_sparse_batch_host.py): numpy only, importable without a GPU, deterministic.

A batch case is a dict: S = the CSC tuple of sparse_cases, ks = the members' ranks, inits = [(W0_b, H0_b)], alpha, beta, max_iter, trace,
inner, method.  Absent entries are zeros; sparse_cases.densify(S, "zero") is the matrix the oracle sees."""
import numpy as np

import sparse_cases as sc

Z3 = [0.0, 0.0, 0.0]


def spb_waves(nnz, cus=sc.DEFAULT_CUS):
    """nnlm_spb_waves (tu_sparse.hip): a wavefront per 256 non-zeros (64 lanes x SPB_TILE = 4), at most 16 per CU."""
    return max(1, min((nnz + 255) // 256, 16 * (cus if cus > 0 else 256)))


def l1_where_lines_are_empty(S, alpha, beta):
    """sparse_cases.make_case's rule: a line without stored entries has the exact solution 0, which the coordinate descent without an L1
    term reaches as rounding dust whose sweep count is decided by the summation order of the Gram; the side that has such lines gets an
    L1 term (both sides then clamp to exact zeros)."""
    rows, cols = sc.line_counts(S)
    alpha, beta = list(alpha), list(beta)
    if (rows == 0).any() and alpha[2] == 0:
        alpha[2] = 0.01
    if (cols == 0).any() and beta[2] == 0:
        beta[2] = 0.01
    return alpha, beta


def values(n, m, rng):
    """A full-rank positive matrix with a rank-6 component (problem() of test_gpu_batch.py)."""
    return rng.random((n, m)) + 0.5 * rng.random((n, 6)) @ rng.random((6, m))


def thinned(n, m, density, ks, seed):
    """The matrix of values() thinned to `density`, random inits."""
    rng = np.random.default_rng(seed)
    V = values(n, m, rng)
    P = np.ones((n, m), dtype=bool) if density >= 1.0 else rng.random((n, m)) < density
    inits = [(rng.random((n, k)), rng.random((k, m))) for k in ks]
    return sc.csc_from_pattern(P, V), inits


def _choose(n, m, nnz, rng):
    P = np.zeros(n * m, dtype=bool)
    P[rng.choice(n * m, size=nnz, replace=False)] = True
    return P.reshape(n, m)


def pattern_edges():
    """[(name, S, ks)]: the edges of the pattern -- a lane's share of the non-zeros empty, partial or full, empty columns in front, at
    the end and in a run, one line holding half of all non-zeros, one-line shapes."""
    out = []
    rng = np.random.default_rng(515)

    def add(name, P, ks=(3, 1, 2)):
        out.append((name, sc.csc_from_pattern(P, values(*P.shape, rng)), list(ks)))

    for nnz in (0, 1, 63, 64, 65, 257):
        add("nnz%d" % nnz, _choose(60, 40, nnz, rng))
    P = rng.random((60, 40)) < 0.2
    P[:, [0, -1]] = False
    add("first_and_last_column_empty", P)
    P = rng.random((60, 40)) < 0.2
    P[:, 10:17] = False
    add("run_of_empty_columns", P)
    P = np.zeros((200, 41), dtype=bool)
    P[:, 5] = True
    P[:, np.arange(41) != 5] = _choose(200, 40, 200, rng)
    add("one_column_holds_half", P)
    add("one_row_holds_half", np.ascontiguousarray(P.T))
    add("33x1", rng.random((33, 1)) < 0.5, (1, 1, 1))
    add("1x40", rng.random((1, 40)) < 0.5, (1, 1, 1))
    return out


def split_case(c, max_iter=None):
    """A sparse_cases case of rank k run as a batch whose rank sum is k: members [k - k // 2, k // 2] on the matching columns of W0 / rows
    of H0 (a rank-1 case stays one member)."""
    k = c["k"]
    ks = [v for v in (k - k // 2, k // 2) if v > 0]
    off = np.concatenate([[0], np.cumsum(ks)])
    inits = [(np.ascontiguousarray(c["W0"][:, off[b]:off[b + 1]]), np.ascontiguousarray(c["H0"][off[b]:off[b + 1], :])) for b in range(len(ks))]
    alpha, beta = l1_where_lines_are_empty(c["S"], c.get("alpha", Z3), c.get("beta", Z3))
    return dict(S=c["S"], ks=ks, inits=inits, alpha=alpha, beta=beta, max_iter=max_iter or c.get("max_iter", 3), trace=c.get("trace", 2),
                inner=c.get("inner", 5), method=c.get("method", 1), name=c.get("name", "%s-%d" % (c["family"], c["seed"])))


def family_seeds(family, count=3):
    """The first `count` seeds of sparse_cases.make_case(seed, "zero") of `family` that a batch can take: small shapes, no masks, rank
    2 .. 64, no one-line corner."""
    seeds, seed = [], 0
    want = sc.FAMILIES.index(family)
    while len(seeds) < count:
        if seed % 4 == want and seed % 5 != 0 and seed % 16 not in (7, 11, 13, 14) and (seed // 3) % 3 != 1:
            c = sc.make_case(seed, "zero")
            if 2 <= c["k"] <= 64 and c["Wm"] is None:
                seeds.append(seed)
        seed += 1
    return seeds


def family_cases():
    return [split_case(sc.make_case(seed, "zero")) for fam in ("empty_lines", "powerlaw", "heavy") for seed in family_seeds(fam)]


def boundary_hits(c):
    """The SPMM_EVENTS the boundary case c hits at its stacked rank (= c["k"]) in the orientation that holds its designed lines."""
    indptr, _ = sc.designed_orientation(c)
    ev = sc.boundary_events(indptr, c["k"])
    return [e for e in sc.SPMM_EVENTS if ev[e]]


def boundary_batch_cases():
    """The boundary family as batches; only the cases that hit an event count."""
    out = []
    for i, c in enumerate(sc.boundary_cases("zero")):
        if boundary_hits(c):
            out.append(split_case(dict(c, method=1 + i % 2)))
    return out
