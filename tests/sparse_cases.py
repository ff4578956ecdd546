"""Case generators for the sparse fuzz (tests/test_gpu_fuzz_sparse.py) and the conditions on them (tests/test_sparse_cases_host.py):
numpy only, importable without a GPU, deterministic in (seed, semantics).

A case is a dict: S = the CSC tuple (indptr int64, indices int32, data float64, shape) and everything c_nnmf needs (k, W0, H0, Wm, Hm,
alpha, beta, max_iter, trace, inner, method in {1, 2}).  semantics is "zero" (nnlm_set_matrix_csc: absent entries are zeros) or "missing"
(nnlm_set_matrix_csc_missing: absent entries are not observed); densify() gives the matrix the fp64 oracle sees.

Values follow make_case of test_gpu_fuzz.py: a planted non-negative model of rank k + 3 plus noise, the start near its factors
(structureless data makes factors die on the way); under absent = zero the pattern multiplies the planted matrix.

The module also restates, in Python, how the kernels split their work (nnlm_sp_workers, nnlm_spg_workers, sp_worker_range, the segment
rule of sp_gram_kernel and the chunk plan of the per-column Grams) so that the `boundary` family can be CHECKED to put columns, segments
and empty runs exactly on worker boundaries; test_gpu_fuzz_sparse.py pins these restatements to the library's own counts."""
import numpy as np

SEMANTICS = ("zero", "missing")
FAMILIES = ("uniform", "powerlaw", "empty_lines", "heavy")
REGS = ([0, 0, 0], [0.01, 0, 0.01], [0.02, 0.01, 0.03], [0, 0.05, 0])  # the four penalty triples of the dense fuzz
SPG_SEG = 2048       # stored entries per Gram segment (tu_sweepq.h)
DEFAULT_CUS = 256    # compute units of the MI355X


# ---- CSC helpers (shared with test_gpu_sparse.py / test_gpu_sparse_missing.py) ---------------------------------------------------------
def csc_from_flat(flat, vals, n, m):
    """CSC from sorted, unique column-major flat indices j * n + i."""
    flat = np.asarray(flat, dtype=np.int64)
    cols, rows = flat // n, flat % n
    indptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=m), out=indptr[1:])
    return indptr, rows.astype(np.int32), np.asarray(vals, dtype=np.float64), (n, m)


def rand_csc(n, m, density, rng):
    """(indptr, indices, data, shape) of a random n x m matrix with round(density n m) stored entries in U(0, 1)."""
    nnz = int(round(density * n * m))
    flat = np.sort(rng.choice(n * m, size=nnz, replace=False)) if nnz < n * m else np.arange(n * m)
    return csc_from_flat(flat, rng.random(flat.size), n, m)


def csc_from_pattern(P, V):
    """CSC of the entries of V where the boolean pattern P is set."""
    n, m = P.shape
    flat = np.flatnonzero(P.T.ravel())
    return csc_from_flat(flat, V.T.ravel()[flat], n, m)


def pattern_of(S):
    indptr, idx, _, (n, m) = S
    P = np.zeros((n, m), dtype=bool)
    P[idx, np.repeat(np.arange(m), np.diff(indptr))] = True
    return P


def densify(S, semantics):
    """The matrix the oracle sees: stored entries in place, zeros ("zero") or NaN ("missing") at the absent ones."""
    indptr, idx, val, (n, m) = S
    A = np.zeros((n, m)) if semantics == "zero" else np.full((n, m), np.nan)
    A[idx, np.repeat(np.arange(m), np.diff(indptr))] = val
    return A


def transpose_csc(S):
    indptr, idx, val, (n, m) = S
    cols = np.repeat(np.arange(m), np.diff(indptr))
    order = np.lexsort((cols, idx))  # by row, then by column
    return csc_from_flat(idx[order].astype(np.int64) * m + cols[order], val[order], m, n)


def err(a, b):
    """Relative Frobenius error, absolute where the reference is (close to) zero."""
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1.0))


class Csc:
    """numpy-only duck-typed sparse matrix (what api.nnmf accepts from scipy)."""

    def __init__(self, csc):
        self.indptr, self.indices, self.data, self.shape = csc

    def tocsc(self):
        return self

    @property
    def T(self):
        return Csc(transpose_csc((self.indptr, self.indices, self.data, self.shape)))


# ---- the work split of the kernels, restated ---------------------------------------------------------------------------------------------
def kp_of(k):
    return 16 * ((k + 15) // 16)


def sp_lanes(KP):
    return 16 if KP == 16 else (32 if KP == 32 else 64)


def sp_workers(nnz, KP, cus=DEFAULT_CUS):
    """nnlm_sp_workers (tu_sparse.hip): about 64 non-zeros per worker, at most 16 wavefronts per CU."""
    ng = 64 // sp_lanes(KP)
    waves = (nnz + 64 * ng - 1) // (64 * ng)
    waves = max(1, min(waves, 16 * (cus if cus > 0 else 256)))
    return waves * ng


def spg_workers(nnz, cus=DEFAULT_CUS):
    """nnlm_spg_workers (tu_sparse.hip): one wavefront per 256 stored entries, at most 16 per CU."""
    return max(1, min((nnz + 255) // 256, 16 * (cus if cus > 0 else 256)))


def worker_range(e_begin, e_end, chunk, w):
    """sp_worker_range (k_sparse.h) / the range of sp_gram_kernel's worker w: non-zeros [e0, e1) of [e_begin, e_end)."""
    b = e_begin + w * chunk
    return min(b, e_end), min(b + chunk, e_end)


def split_of(nnz, nworkers):
    """(chunk, [(e0, e1)] of every worker) for nnz non-zeros counted from 0."""
    chunk = max(1, (nnz + nworkers - 1) // nworkers)
    return chunk, [worker_range(0, nnz, chunk, w) for w in range(nworkers)]


def segments_of(length):
    """Segment rule of sp_gram_kernel: a column of more than SPG_SEG stored entries is summed in ceil(length / SPG_SEG) segments."""
    return (length + SPG_SEG - 1) // SPG_SEG if length > SPG_SEG else 0


def gram_chunks(indptr, KP, alloc_limit=0):
    """spg_prepare (nnlm_mi355x.hip): column chunks [(c0, c1)] whose Gram slots (one per column + one per segment of a long column) fit
    in min(1 GiB, alloc_limit) bytes."""
    budget = 1 << 30
    if alloc_limit and alloc_limit < budget:
        budget = alloc_limit
    cap = max(1, budget // (KP * KP * 8))
    out, c0, cols, segs = [], 0, 0, 0
    for c in range(len(indptr) - 1):
        ns = segments_of(int(indptr[c + 1] - indptr[c]))
        if cols > 0 and cols + segs + 1 + ns > cap:
            out.append((c0, c))
            c0, cols, segs = c, 0, 0
        cols += 1
        segs += ns
    out.append((c0, len(indptr) - 1))
    return out


def predicted_counts(indptr, k, cus=DEFAULT_CUS, alloc_limit=0):
    """What the handle reports for one half-step over this orientation: spmm workers, Gram workers (summed over chunks), Gram chunks."""
    KP = kp_of(k)
    chunks = gram_chunks(indptr, KP, alloc_limit)
    return dict(sp_workers=sp_workers(int(indptr[-1]), KP, cus),
                sp_gram_workers=sum(spg_workers(int(indptr[c1] - indptr[c0]), cus) for c0, c1 in chunks), sp_gram_chunks=len(chunks))


SPMM_EVENTS = ("column_starts_on_boundary", "empty_run_on_boundary", "column_spans_3_workers", "head_ends_at_worker_end",
               "whole_range_is_head", "trailing_empty_columns", "leading_empty_columns")
GRAM_EVENTS = ("segment_starts_on_boundary", "column_of_2048", "column_of_2049", "long_column_first_of_chunk", "long_column_last_of_chunk")


def boundary_events(indptr, k, cus=DEFAULT_CUS, alloc_limit=0):
    """{event: [columns]} of one orientation (indptr of the CSC for the H half-step, of the CSR for the W half-step), from the
    restatements above.  Boundaries are those between two non-empty worker ranges."""
    ptr = np.asarray(indptr, dtype=np.int64)
    ncols, nnz, KP = len(ptr) - 1, int(ptr[-1]), kp_of(k)
    length = np.diff(ptr)
    ev = {e: [] for e in SPMM_EVENTS + GRAM_EVENTS}
    _, ranges = split_of(nnz, sp_workers(nnz, KP, cus))
    bounds = sorted({e0 for e0, e1 in ranges[1:] if e0 < e1})
    for c in range(ncols):
        s, t = int(ptr[c]), int(ptr[c + 1])
        if s in bounds:
            if t > s:
                ev["column_starts_on_boundary"].append(c)
            elif c + 1 < ncols and ptr[c + 2] == s and (c == 0 or ptr[c - 1] < s):
                ev["empty_run_on_boundary"].append(c)  # (first of a run of at least two empty columns sitting on the boundary)
        if t > s and sum(1 for e0, e1 in ranges if e0 < t and e1 > s) >= 3:
            ev["column_spans_3_workers"].append(c)
    for e0, e1 in ranges:
        if e0 >= e1:
            continue
        c = int(np.searchsorted(ptr, e0, side="right")) - 1  # the column holding non-zero e0
        while length[c] == 0:
            c -= 1
        if ptr[c] < e0:  # the range starts with a head of column c
            if ptr[c + 1] == e1:
                ev["head_ends_at_worker_end"].append(c)
            if ptr[c + 1] > e1:
                ev["whole_range_is_head"].append(c)
    if nnz > 0:
        if length[-1] == 0:
            ev["trailing_empty_columns"].append(ncols - 1)
        if length[0] == 0:
            ev["leading_empty_columns"].append(0)
    chunks = gram_chunks(ptr, KP, alloc_limit)
    for c0, c1 in chunks:
        E0, E1 = int(ptr[c0]), int(ptr[c1])
        nw = spg_workers(E1 - E0, cus)
        chunk = max(1, (E1 - E0 + nw - 1) // nw)
        gb = {E0 + w * chunk for w in range(1, nw) if E0 + w * chunk < E1}
        for c in range(c0, c1):
            for s in range(1, segments_of(int(length[c]))):
                if int(ptr[c]) + s * SPG_SEG in gb:
                    ev["segment_starts_on_boundary"].append(c)
        if len(chunks) >= 3:
            if length[c0] > SPG_SEG:
                ev["long_column_first_of_chunk"].append(c0)
            if length[c1 - 1] > SPG_SEG:
                ev["long_column_last_of_chunk"].append(c1 - 1)
    ev["column_of_2048"] = [int(c) for c in np.flatnonzero(length == SPG_SEG)]
    ev["column_of_2049"] = [int(c) for c in np.flatnonzero(length == SPG_SEG + 1)]
    return ev


def straddling_lines(indptr, k, cus=DEFAULT_CUS):
    """Columns whose non-zeros lie in more than one spmm worker range."""
    ptr = np.asarray(indptr, dtype=np.int64)
    nnz = int(ptr[-1])
    chunk, _ = split_of(nnz, sp_workers(nnz, kp_of(k), cus))
    s, t = ptr[:-1], ptr[1:]
    return [int(c) for c in np.flatnonzero((t > s) & (s // chunk != (np.maximum(t, 1) - 1) // chunk))]


# ---- patterns ----------------------------------------------------------------------------------------------------------------------------
def _uniform(n, m, density, rng):
    return np.ones((n, m), dtype=bool) if density >= 1.0 else rng.random((n, m)) < density


def _powerlaw(n, m, rng, by_rows):
    """Column (by_rows: row) counts proportional to 1 / (rank + 3), ranks in random order, about 10 % stored overall."""
    if by_rows:
        return _powerlaw(m, n, rng, False).T
    w = 1.0 / (rng.permutation(m) + 3.0)
    counts = np.minimum(n, np.rint(0.1 * n * m * w / w.sum()).astype(np.int64))
    P = np.zeros((n, m), dtype=bool)
    for j in np.flatnonzero(counts):
        P[rng.choice(n, size=int(counts[j]), replace=False), j] = True
    return P


def _empty_lines(n, m, rng):
    """30 % stored; the first and last row and column empty, a few inside, among them runs of adjacent empty columns and rows."""
    P = rng.random((n, m)) < 0.3
    for axis, size in ((0, n), (1, m)):
        if size < 3:
            continue  # (the n = 1 and m = 1 corners keep their only line)
        lines = {0, size - 1}
        if size >= 12:
            r = int(rng.integers(2, size - 6))
            lines |= {r, r + 1, r + 2, int(rng.integers(1, size - 1))}  # a run of three and a single one
        if size >= 40:
            r = int(rng.integers(2, size - 4))
            lines |= {r, r + 1}
        ix = sorted(lines)
        if axis == 0:
            P[ix, :] = False
        else:
            P[:, ix] = False
    return P


def _heavy(n, m, rng):
    """One fully stored column and one fully stored row on a thin background (3 %)."""
    P = rng.random((n, m)) < 0.03
    P[:, int(rng.integers(0, m))] = True
    P[int(rng.integers(0, n)), :] = True
    return P


def _top_up(P, need, rng):
    """Every non-empty line gets at least `need` stored entries (as far as the non-empty lines of the other direction allow); fully
    empty lines stay empty."""
    rows, cols = np.flatnonzero(P.any(axis=1)), np.flatnonzero(P.any(axis=0))
    for j in cols:
        have = int(P[:, j].sum())
        if have < min(need, rows.size):
            free = rows[~P[rows, j]]
            P[rng.choice(free, size=min(need, rows.size) - have, replace=False), j] = True
    for i in rows:
        have = int(P[i, :].sum())
        if have < min(need, cols.size):
            free = cols[~P[i, cols]]
            P[i, rng.choice(free, size=min(need, cols.size) - have, replace=False)] = True
    return P


# ---- whole-run cases ---------------------------------------------------------------------------------------------------------------------
def _planted(n, m, k, rng):
    Wp, Hp = rng.random((n, k + 3)) ** 2 + 0.05, rng.random((k + 3, m)) ** 2 + 0.05
    V = Wp @ Hp / (k + 3) * 4 + 0.02 * rng.random((n, m)) + 0.01
    sc = 2.0 / np.sqrt(k + 3)
    return V, Wp[:, :k] * sc * (0.7 + 0.6 * rng.random((n, k))), Hp[:k, :] * sc * (0.7 + 0.6 * rng.random((k, m)))


def family_of(seed):
    fam = FAMILIES[seed % 4]
    if fam == "uniform":
        return fam, [0.05, 0.2, 0.5, 1.0][(seed // 4) % 4]
    return fam, None


def make_case(seed, semantics, large=None):
    """Random whole-run case number `seed` under `semantics`.  large: None = every fifth seed is 400..3000 x 300..1500."""
    assert semantics in SEMANTICS
    miss = semantics == "missing"
    rng = np.random.default_rng(88000 + 2 * seed + int(miss))
    fam, density = family_of(seed)
    corner = {13: "n1", 14: "m1", 7: "k1"}.get(seed % 16)
    if large is None:
        large = seed % 5 == 0
    band = (seed + seed // 4) % 4  # the KP form: k in 1..16, 17..32, 33..48, 49..64
    if large or corner:
        band = 0
    k = int(rng.integers(16 * band + 1, 16 * band + 17))
    if not miss and seed % 16 == 11:
        k = int(rng.integers(65, 71))  # rank > 64: one SpMM launch per 64 coordinates
    if large:
        n, m = int(rng.integers(400, 3001)), int(rng.integers(300, 1501))
    else:
        lo = 2 if seed % 7 in (3, 6) else min(6 * k, 330)  # (two seeds in seven: ranks up to the smaller dimension)
        n, m = int(rng.integers(max(2, lo), 401)), int(rng.integers(max(2, lo), 401))
    if corner == "n1":
        n = 1
    if corner == "m1":
        m = 1
    if corner == "k1":
        k = 1
    k = max(1, min(k, n, m))
    if fam == "uniform":
        P = _uniform(n, m, density, rng)
    elif fam == "powerlaw":
        P = _powerlaw(n, m, rng, by_rows=(seed // 4) % 2 == 1)
    elif fam == "empty_lines":
        P = _empty_lines(n, m, rng)
    else:
        P = _heavy(n, m, rng)
    topped = miss and (seed // 2) % 4 != 1  # three seeds out of four (naive patterns: most cases rank deficient somewhere)
    if topped:
        P = _top_up(P, k + 2, rng)
    V, W0, H0 = _planted(n, m, k, rng)
    S = csc_from_pattern(P, V)
    Wm = Hm = None
    if (seed // 3) % 3 == 1 and min(n, m) > 1:  # masks: a few coordinates pinned to zero (not where one pin empties a whole factor)
        Wm = (rng.random((n, k)) < 0.1).astype(np.int32)
        Hm = (rng.random((k, m)) < 0.1).astype(np.int32)
        W0[Wm != 0] = 0.0
        H0[Hm != 0] = 0.0
    alpha, beta = list(REGS[seed % 4]), list(REGS[(seed // 2) % 4])
    if not miss:
        # absent = zero: a line without stored entries has the exact solution 0.  Without an L1 term the coordinate descent leaves it at
        # the rounding dust of G x / G_qq, and whether that dust still counts as a change -- the sweep count -- is decided by the summation
        # order of the shared Gram (4 of 600 strict cases of a deep run differed in average_epoch alone, all of this kind).  With
        # an L1 term both sides clamp to exact zeros, so the side that has empty lines gets one.
        rows, cols = P.sum(axis=1), P.sum(axis=0)
        if (rows == 0).any() and alpha[2] == 0:
            alpha[2] = 0.01
        if (cols == 0).any() and beta[2] == 0:
            beta[2] = 0.01
    return dict(S=S, semantics=semantics, family=fam, density=density, topped=topped, k=k, W0=W0, H0=H0, Wm=Wm, Hm=Hm, alpha=alpha, beta=beta,
                max_iter=int(rng.integers(1, 6)), trace=int(rng.integers(1, 4)), inner=int(rng.integers(1, 8)),
                method=1 + (seed + seed // 4) % 2, rel_tol=-1.0, seed=seed)


def make_stop_case(seed, semantics):
    """The case of the stopping-rule test: make_case (large shapes on every tenth seed only: up to 80 iterations each) with
    max_iter 80 and rel_tol from {1e-2, 1e-3}."""
    c = make_case(seed, semantics, large=seed % 10 == 0)
    c["max_iter"] = 80
    c["rel_tol"] = [1e-2, 1e-3][(seed // 2) % 2]
    return c


def make_cap_case(semantics):
    """More than 16 * 64 * 256 non-zeros at one worker per wavefront (k > 32): the cap on the worker count binds and a worker's range
    is no longer about 64 non-zeros."""
    rng = np.random.default_rng(4242 + int(semantics == "missing"))
    n, m, k = 3000, 2000, 40
    V, W0, H0 = _planted(n, m, k, rng)
    P = rng.random((n, m)) < 0.1
    return dict(S=csc_from_pattern(P, V), semantics=semantics, family="cap", density=0.1, topped=False, k=k, W0=W0, H0=H0, Wm=None, Hm=None,
                alpha=[0.01, 0, 0], beta=[0, 0, 0.01], max_iter=3, trace=2, inner=5, method=1, rel_tol=-1.0, seed=-1)


def nnmf_args(c, max_iter=None, n_threads=1):
    """The arguments of c_nnmf behind the matrix (the oracle: ref.c_nnmf(densify(...), *nnmf_args(c)); the library: c_nnmf_csc(*S, ...))."""
    return (c["k"], c["W0"], c["H0"], c["Wm"], c["Hm"], c["alpha"], c["beta"], c["max_iter"] if max_iter is None else max_iter, c["rel_tol"],
            n_threads, 0, False, c["inner"], 1e-9, c["method"], c["trace"])


def line_counts(S):
    """Stored entries per row and per column."""
    indptr, idx, _, (n, m) = S
    return np.bincount(idx, minlength=n), np.diff(indptr)


def rank_deficient(c):
    """absent = missing: a non-empty row or column with fewer stored entries than k -- its Gram is rank deficient and sweep counts are
    decided by rounding; there, and only there, average_epoch is compared with a tolerance."""
    if c["semantics"] != "missing":
        return False
    rows, cols = line_counts(c["S"])
    return bool(((rows > 0) & (rows < c["k"])).any() or ((cols > 0) & (cols < c["k"])).any())


def describe(c):
    indptr, idx, _, shape = c["S"]
    rows, cols = line_counts(c["S"])
    return dict(seed=c["seed"], semantics=c["semantics"], family=c["family"], density=c["density"], shape=shape, nnz=int(idx.size), k=c["k"],
                method=c["method"], masks=c["Wm"] is not None, alpha=c["alpha"], beta=c["beta"], max_iter=c["max_iter"], trace=c["trace"],
                inner=c["inner"], rel_tol=c["rel_tol"], topped=c["topped"], empty_rows=int((rows == 0).sum()), empty_cols=int((cols == 0).sum()),
                max_row=int(rows.max(initial=0)), max_col=int(cols.max(initial=0)))


def degenerate(c, ref, n_threads=1):
    """degenerate() of the dense fuzz on the densified matrix, with the oracle alone: a factor dies on the oracle's way (a column of W /
    row of H at 1e-8 of the median norm, or not finite).  For a case with a stopping rule the first three iterations are looked at."""
    A = densify(c["S"], c["semantics"])
    for it in range(1, min(c["max_iter"], 3 if c["rel_tol"] > 0 else c["max_iter"]) + 1):
        o = ref.c_nnmf(A, *nnmf_args(dict(c, rel_tol=-1.0), it, n_threads))
        W, H = o["W"], o["H"]
        if not (np.isfinite(W).all() and np.isfinite(H).all()):
            return True
        dw, dh = (W * W).sum(axis=0), (H * H).sum(axis=1)
        # (<=, not the dense fuzz's <: when more than half of a factor's columns are exactly zero the median is zero too -- zero seed 96,
        #  inner = 1: the oracle's W after iteration 1; the dense F32 path then differs from the oracle exactly as the sparse one does)
        if dw.min() <= 1e-8 * np.median(dw) or dh.min() <= 1e-8 * np.median(dh):
            return True
    return False


# ---- the boundary family -----------------------------------------------------------------------------------------------------------------
COUNTS = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 2047, 2048, 2049, 4096, 4097)

# (name, s = stored entries of the column in front, the columns behind it, k, nnlm_debug_alloc_limit in Gram slots or 0)
# The s values and the order of the columns were found by a search over the restatements above (boundary_events) and are pinned by
# test_sparse_cases_host.py: every event of SPMM_EVENTS and GRAM_EVENTS occurs, the worker-boundary ones at 16, 32 and 64 lanes per worker.
_BOUNDARY_SPECS = (
    ("chunk_edges", 0, (64, 0, 64, 0, 0, 65, 0, 64, 17, 9, 4, 2049, 4097), 64, 5),
    ("one_2048", 63, (0, 0, 5, 2048, 0, 0), 20, 5),
    ("segment_on_boundary", 52, (9, 5, 8, 65, 4097, 4, 65, 4, 63, 0, 0), 3, 0),
    ("head_fills_workers", 61, (4097, 63, 0, 0, 8), 3, 5),
    ("short_columns", 0, (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 0, 0), 16, 0),
    ("segment_counts", 5, (2047, 2048, 2049, 0, 4096, 4097, 1), 33, 6),
)


def _columns_case(name, counts, k, slots, semantics, transposed):
    """A matrix whose column j holds counts[j] stored entries at rows spread by a fixed rule; transposed: its transpose (the designed
    lines are then rows: the W half-step's CSR sees them)."""
    n = max(max(counts) + 103, 8)
    m = len(counts)
    rng = np.random.default_rng(sum((i + 1) * c for i, c in enumerate(counts)) % (2 ** 31) + 7 * k)
    P = np.zeros((n, m), dtype=bool)
    for j, cnt in enumerate(counts):
        if cnt:
            P[(j * 37 + (np.arange(cnt) * n) // cnt) % n, j] = True  # cnt distinct rows, evenly spread, shifted per column
    V, W0, H0 = _planted(n, m, k, rng)
    S = csc_from_pattern(P, V)
    if transposed:
        S, W0, H0 = transpose_csc(S), np.ascontiguousarray(H0.T), np.ascontiguousarray(W0.T)
    designed = [j for j, cnt in enumerate(counts)]
    return dict(S=S, semantics=semantics, family="boundary", name=name + ("^T" if transposed else ""), transposed=transposed, k=k, W0=W0, H0=H0,
                designed=designed, alloc_limit=slots * kp_of(k) ** 2 * 8, density=None, topped=False, Wm=None, Hm=None, seed=-1)


def boundary_specs():
    return _BOUNDARY_SPECS


def boundary_cases(semantics):
    """The deterministic boundary family: every spec and its transpose."""
    return [_columns_case(name, (s,) + tuple(cols), k, slots, semantics, tr) for name, s, cols, k, slots in _BOUNDARY_SPECS for tr in (False, True)]


def designed_orientation(c):
    """(indptr of the orientation that holds the designed lines, which half-step reads it: 1 = H over the CSC, 0 = W over the CSR)."""
    return (transpose_csc(c["S"])[0], 0) if c["transposed"] else (c["S"][0], 1)


# ---- nnlm (one-shot fold-in) cases -------------------------------------------------------------------------------------------------------
def make_nnlm_case(seed, semantics):
    """The generator of test_random_nnlm_runs (test_gpu_fuzz.py) restricted to methods 1, 2, y sparsified by the pattern families."""
    miss = semantics == "missing"
    rng = np.random.default_rng(66000 + 2 * seed + int(miss))
    n, p, q = int(rng.integers(3, 600)), int(rng.integers(1, 81 if not miss else 65)), int(rng.integers(1, 40))
    if seed % 3 == 0:
        p = int(rng.integers(1, min(n, 20) + 1))  # (a well-determined regression)
    method = 1 + seed % 2
    x = rng.random((n, p)) + 0.02
    b = rng.random((p, q)) * (rng.random((p, q)) > 0.3)
    b[rng.integers(0, p, q), np.arange(q)] += 0.3
    y = x @ b + 0.02 * rng.random((n, q)) + 0.01
    fam, density = family_of(seed // 2)
    if fam == "uniform":
        P = _uniform(n, q, density, rng)
    elif fam == "powerlaw":
        P = _powerlaw(n, q, rng, by_rows=False)
    elif fam == "empty_lines":
        P = _empty_lines(n, q, rng)
    else:
        P = _heavy(n, q, rng)
    if miss and seed % 4 != 1:
        cols = np.flatnonzero(P.any(axis=0))
        for j in cols:  # every non-empty response gets at least p + 2 observations
            have = int(P[:, j].sum())
            if have < min(p + 2, n):
                P[rng.choice(np.flatnonzero(~P[:, j]), size=min(p + 2, n) - have, replace=False), j] = True
    alpha = [[0, 0, 0], [0.01, 0, 0.001], [0.02, 0.01, 0.03]][seed % 3]
    if not miss and alpha[2] == 0:
        # (absent = zero without an L1 term: a response of zeros only has the solution 0, which the coordinate descent reaches as rounding
        #  dust whose sweep count is decided by the summation order of the Gram -- DESIGN 2; such a response gets one stored entry)
        for j in np.flatnonzero(~P.any(axis=0)):
            P[int(rng.integers(0, n)), j] = True
    mask = (rng.random((p, q)) < 0.15) if (seed // 2) % 3 == 1 else None
    b0 = None if seed % 5 == 0 else rng.random((p, q)) + 0.01
    if mask is not None and b0 is not None:
        b0[mask] = 0.0
    return dict(x=x, S=csc_from_pattern(P, y), semantics=semantics, family=fam, alpha=alpha, mask=mask, b0=b0, max_iter=int(rng.integers(1, 30)),
                method=method, seed=seed)


def describe_nnlm(c):
    n, q = c["S"][3]
    return dict(seed=c["seed"], semantics=c["semantics"], family=c["family"], n=n, p=c["x"].shape[1], q=q, nnz=int(c["S"][1].size), method=c["method"],
                mask=c["mask"] is not None, b0=c["b0"] is not None, alpha=c["alpha"], max_iter=c["max_iter"])


# ---- batch cases -------------------------------------------------------------------------------------------------------------------------
def make_batch_case(seed):
    """Random batch on a dense A: B in 1..8 members, ranks with sum <= 64 (a sum of exactly 64 and a rank-1 member on some seeds), methods
    1, 2, penalties, trace 1..3, rel_tol from {-1, 1e-2, 1e-3} (members stop at different iterations)."""
    rng = np.random.default_rng(99000 + seed)
    B = int(rng.integers(1, 9))
    n, m = int(rng.integers(40, 300)), int(rng.integers(40, 300))
    kmax = max(1, min(64 // B, min(n, m) // 6))
    ks = [int(v) for v in rng.integers(1, kmax + 1, B)]
    if seed % 4 == 1:
        ks[0] = 1
    if seed % 4 == 2:  # a rank sum of exactly 64, in equal members (ranks stay at a sixth of the smaller dimension)
        B = [2, 4, 8][(seed // 4) % 3]
        ks = [64 // B] * B
        n, m = max(n, 6 * ks[0]), max(m, 6 * ks[0])
    r = max(ks) + 3
    Wp, Hp = rng.random((n, r)) ** 2 + 0.05, rng.random((r, m)) ** 2 + 0.05
    A = Wp @ Hp / r * 4 + 0.02 * rng.random((n, m)) + 0.01
    sc = 2.0 / np.sqrt(r)
    # (member b starts from a perturbation of its own width: members of one rank still stop at different iterations)
    inits = []
    for k in ks:
        sel = rng.permutation(r)[:k]
        amp = [0.6, 0.1, 1.5][int(rng.integers(0, 3))]
        inits.append((Wp[:, sel] * sc * (1 - amp / 2 + amp * rng.random((n, k))), Hp[sel, :] * sc * (1 - amp / 2 + amp * rng.random((k, m)))))
    rel_tol = [-1.0, 1e-2, 1e-3][seed % 3]
    return dict(A=A, ks=ks, inits=inits, alpha=list(REGS[seed % 4]), beta=list(REGS[(seed // 2) % 4]), max_iter=int(rng.integers(2, 7)) if rel_tol < 0 else 60,
                rel_tol=rel_tol, method=1 + (seed // 3) % 2, trace=int(rng.integers(1, 4)), inner=int(rng.integers(1, 8)), seed=seed)


def describe_batch(c):
    return dict(seed=c["seed"], shape=c["A"].shape, ks=c["ks"], alpha=c["alpha"], beta=c["beta"], max_iter=c["max_iter"], rel_tol=c["rel_tol"],
                method=c["method"], trace=c["trace"], inner=c["inner"])
