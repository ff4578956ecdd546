"""Cases of the batched factorisation on a sparse A whose absent entries are MISSING (tests/test_gpu_sparse_missing_batch.py) and the
rules of its kernel restated in numpy (tests/test_sparse_missing_batch_host.py): importable without a GPU, deterministic.

A batch case is a dict: name, S = the CSC tuple of sparse_cases, ks = the members' ranks, inits = [(W0_b, H0_b)], alpha, beta, max_iter,
rel_tol, trace, inner and, for the boundary family, slots (Gram slots nnlm_debug_alloc_limit leaves room for, 0 = no limit).  Both
methods run on every case.  sparse_cases.densify(S, "missing") is the matrix the oracle sees.

Every case here is shown well posed by the host test from the oracle alone (its run and its run on the row- and column-reversed problem
agree, sweep counts included); the GPU test has no skip rule."""
import numpy as np

import sparse_cases as sc
import sparse_batch_cases as sbc

Z3 = [0.0, 0.0, 0.0]
L2 = [0.01, 0.0, 0.0]  # (a line with fewer stored entries than the rank has a rank-deficient Gram: a small L2 term makes it definite)
KS_LISTS = ([5], [1, 4, 7], [1, 4, 7, 16, 3, 2, 8, 6])
DENSITIES = (0.01, 0.2, 1.0)
STACK_EDGES = ([1], [64], [16, 16, 16, 16], [30, 1, 33], [16, 1], [1, 16], [8, 9], [8] * 8, list(range(1, 11)))


# ---- the rules of sp_gram_batch_kernel and its host side, restated -------------------------------------------------------------------------
def goff_of(ks):
    """Slot layout: member b's Gram starts goff[b] doubles into a column's slot, compact at its own KP_b = 16 ceil(k_b / 16); goff[-1] is the
    slot."""
    return [int(v) for v in np.concatenate([[0], np.cumsum([sc.kp_of(k) ** 2 for k in ks])])]


def tile_pairs(ks, active=None):
    """(set pairs, pairs of the stacked upper triangle, gathered tiles): pair (ta, tb), ta <= tb, of 16 x 16 tiles is set when it meets an
    ACTIVE member's diagonal block [off_b, off_b + k_b)^2; a tile is gathered when a set pair touches it."""
    off = np.concatenate([[0], np.cumsum(ks)])
    NT = sc.kp_of(int(off[-1])) // 16
    active = [True] * len(ks) if active is None else active
    pairs = set()
    for ta in range(NT):
        for tb in range(ta, NT):
            for b in range(len(ks)):
                lo, hi = off[b], off[b + 1]
                if active[b] and lo < 16 * ta + 16 and hi > 16 * ta and lo < 16 * tb + 16 and hi > 16 * tb:
                    pairs.add((ta, tb))
    return pairs, NT * (NT + 1) // 2, sorted({t for p in pairs for t in p})


def slot_word(ks, i, j):
    """Word of a column's slot that element (i, j), i <= j, of the stacked Gram goes to, or None when i and j belong to different
    members."""
    off = np.concatenate([[0], np.cumsum(ks)])
    bi, bj = int(np.searchsorted(off, i, side="right")) - 1, int(np.searchsorted(off, j, side="right")) - 1
    if bi != bj or j >= off[-1]:
        return None
    return goff_of(ks)[bi] + (i - off[bi]) * sc.kp_of(ks[bi]) + (j - off[bi])


def gram_chunks_of_slot(indptr, slot, alloc_limit=0):
    """sc.gram_chunks for a slot of `slot` doubles (the batch: sum of KP_b^2)."""
    budget = 1 << 30
    if alloc_limit and alloc_limit < budget:
        budget = alloc_limit
    cap = max(1, budget // (slot * 8))
    out, c0, cols, segs = [], 0, 0, 0
    for c in range(len(indptr) - 1):
        ns = sc.segments_of(int(indptr[c + 1] - indptr[c]))
        if cols > 0 and cols + segs + 1 + ns > cap:
            out.append((c0, c))
            c0, cols, segs = c, 0, 0
        cols += 1
        segs += ns
    out.append((c0, len(indptr) - 1))
    return out


# ---- hold-out split ----------------------------------------------------------------------------------------------------------------------
def split(S, pos):
    """S without its stored entries at the sorted positions pos, and the pattern of those: (training S, (indptr, indices), values)."""
    indptr, idx, val, (n, m) = S
    cols = np.repeat(np.arange(m), np.diff(indptr))
    held = np.zeros(idx.size, dtype=bool)
    held[pos] = True
    hptr, tptr = np.zeros(m + 1, dtype=np.int64), np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols[held], minlength=m), out=hptr[1:])
    np.cumsum(np.bincount(cols[~held], minlength=m), out=tptr[1:])
    return (tptr, idx[~held].copy(), val[~held].copy(), (n, m)), (hptr, idx[held].copy()), val[held].copy()


def held_out(S, fraction, seed):
    pos = np.sort(np.random.default_rng(seed).choice(S[1].size, size=int(round(fraction * S[1].size)), replace=False))
    return split(S, pos)


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
def case(name, S, ks, inits, alpha=L2, beta=L2, max_iter=6, rel_tol=-1.0, trace=2, inner=50, slots=0):
    return dict(name=name, S=S, ks=list(ks), inits=inits, alpha=list(alpha), beta=list(beta), max_iter=max_iter, rel_tol=rel_tol, trace=trace,
                inner=inner, slots=slots)


def member_cases():
    out = []
    for ks in KS_LISTS:
        for d in DENSITIES:
            S, inits = sbc.thinned(150, 110, d, ks, 11 * len(ks) + int(100 * d))
            out.append(case("members-%d-%g" % (len(ks), d), S, ks, inits, max_iter=8, trace=3))
    return out


def stack_edge_cases():
    out = []
    for ks in STACK_EDGES:
        S, inits = sbc.thinned(180, 140, 0.25, ks, sum(ks) + 3 * len(ks))
        out.append(case("stack-" + "_".join(str(k) for k in ks), S, ks, inits, max_iter=4))
    return out


def content_cases():
    """Explicit stored zeros (observations), empty rows and columns, nothing stored, a column with one entry, penalties in each of the
    three positions."""
    out = []
    ks = [3, 1, 6]
    rng = np.random.default_rng(77)

    def inits_of(n, m):
        return [(rng.random((n, k)), rng.random((k, m))) for k in ks]

    n, m = 150, 160
    V = sbc.values(n, m, rng)
    P = rng.random((n, m)) < 0.2
    Vz = np.where(rng.random((n, m)) < 0.3, 0.0, V)  # (30 % of the stored entries are explicit zeros)
    out.append(case("stored_zeros", sc.csc_from_pattern(P, Vz), ks, inits_of(n, m)))
    Pe = P.copy()
    Pe[[0, 17, n - 1], :] = False
    Pe[:, [0, 40, 41, 42, m - 1]] = False
    out.append(case("empty_lines", sc.csc_from_pattern(Pe, V), ks, inits_of(n, m)))
    out.append(case("nothing_stored", sc.csc_from_pattern(np.zeros((n, m), dtype=bool), V), ks, inits_of(n, m)))
    Po = P.copy()
    Po[:, 7] = False
    Po[33, 7] = True
    out.append(case("one_entry_column", sc.csc_from_pattern(Po, V), ks, inits_of(n, m)))
    for pos in range(3):
        reg = [0.0, 0.0, 0.0]
        reg[pos] = 0.05
        base = [0.01 if pos else 0.0, 0.0, 0.0]  # (positions 1 and 2 keep a small L2 term: see L2)
        out.append(case("penalty_%d" % pos, sc.csc_from_pattern(P, V), ks, inits_of(n, m), alpha=[a + b for a, b in zip(reg, base)],
                        beta=[a + b for a, b in zip(reg[::-1], base)]))
    return out


def boundary_cases():
    """The deterministic boundary family of sparse_cases under absent = missing (tall thin matrices: columns and rows of 2047, 2048, 2049,
    4096 and 4097 stored entries, long columns first and last of a chunk) as batches whose rank sum is the case's k; slots = the Gram
    slots of the case's allocation limit, so the batch is cut into the chunks the family was designed for."""
    out = []
    for c in sc.boundary_cases("missing"):
        b = sbc.split_case(c)
        slots = c["alloc_limit"] // (sc.kp_of(c["k"]) ** 2 * 8)
        out.append(case("boundary-" + c["name"], c["S"], b["ks"], b["inits"], max_iter=2, trace=1, inner=5, slots=slots))
    return out


def alloc_limit_of(c):
    """nnlm_debug_alloc_limit for the case's slots at the batch's slot size (0: none)."""
    return c["slots"] * goff_of(c["ks"])[-1] * 8


def stop_case():
    """Members that stop at different iterations by their own rule (scaled inits, as test_gpu_sparse_batch.py)."""
    ks = [2, 6, 3, 10, 1]
    S, inits = sbc.thinned(160, 150, 0.3, ks, 21)
    inits = [(w * s, x * s) for (w, x), s in zip(inits, [1.0, 0.02, 3.0, 0.3, 0.01])]
    return case("stop", S, ks, inits, alpha=L2, beta=L2, max_iter=16, rel_tol=1e-2, trace=1)


def frozen_case():
    """Stacked padded rank 16 = every member's own: the SpMM splits alike, so each member must end with the bits of its solo run."""
    ks = [2, 6, 3]
    S, inits = sbc.thinned(160, 150, 0.3, ks, 21)
    inits = [(w * s, x * s) for (w, x), s in zip(inits, [1.0, 0.02, 3.0])]
    return case("frozen", S, ks, inits, alpha=L2, beta=L2, max_iter=16, rel_tol=1e-2, trace=1)


def mask_case():
    """Four members of rank 8 (tiles 0, 0, 1, 1 of the stack) of which all but member 0 stop early (oracle: iterations 16, 8, 7, 8 / 16, 8, 9, 11): the Gram
    kernel's mask shrinks from two tile pairs to one while member 0 goes on."""
    ks = [8, 8, 8, 8]
    S, inits = sbc.thinned(160, 150, 0.3, ks, 33)
    inits = [(w * s, x * s) for (w, x), s in zip(inits, [0.02, 0.3, 3.0, 1.0])]
    return case("mask", S, ks, inits, alpha=L2, beta=L2, max_iter=16, rel_tol=1e-2, trace=1)


def all_cases():
    return member_cases() + stack_edge_cases() + content_cases() + boundary_cases() + [stop_case(), frozen_case(), mask_case()]


def reversed_member(c, b):
    """Member b of case c on the row- and column-reversed matrix (another summation order for the oracle): (A, W0, H0)."""
    A = sc.densify(c["S"], "missing")
    W0, H0 = c["inits"][b]
    return np.ascontiguousarray(A[::-1, ::-1]), np.ascontiguousarray(W0[::-1, :]), np.ascontiguousarray(H0[:, ::-1])


# ---- the planted-rank case of nnmf_cv ------------------------------------------------------------------------------------------------------
PLANTED_SEED = 0     # (seeds 0 .. 7 all name k = 3 under the oracle; ratios 0.37 .. 0.83, this one the lowest)
PLANTED_RATIO = 0.367  # held-out MSE at k = 3 over the runner-up's (k = 4), from the oracle: test_sparse_missing_batch_host.py recomputes it
PLANTED_KS = list(range(1, 7))
PLANTED_OPTS = dict(max_iter=60, rel_tol=1e-5)  # (nnmf()'s other defaults: scd, no penalties, inner_max_iter 50, trace 2)


def planted(seed=PLANTED_SEED):
    """About 120 x 90, rank 3, roughly 40 % stored, sparse spikes as noise -> (S, n, m)."""
    rng = np.random.default_rng(1000 + seed)
    n, m, k = 120, 90, 3
    V = rng.random((n, k)) @ rng.random((k, m))
    spikes = (rng.random((n, m)) < 0.02) * rng.random((n, m)) * 0.5
    P = rng.random((n, m)) < 0.4
    return sc.csc_from_pattern(P, V + spikes), n, m


def planted_holdout(seed=PLANTED_SEED):
    """The planted case's 15 % hold-out set as api.nnmf_cv(holdout = 0.15, rng = default_rng(seed)) draws it: the positions come first
    from the generator."""
    S, n, m = planted(seed)
    g = np.random.default_rng(seed)
    pos = np.sort(g.choice(S[1].size, size=int(round(0.15 * S[1].size)), replace=False))
    return S, pos, g


def planted_inits(g, n, m, ks=PLANTED_KS):
    """The members' default inits as api.nnmf_cv draws them from the generator behind the hold-out positions: member by member, W first."""
    out = []
    for k in ks:
        W = 0.01 * g.random(n * k).reshape((n, k))
        out.append((W, 0.01 * g.random(k * m).reshape((k, m), order="F")))
    return out
