"""Cases for every instantiation behind the per-entry-weights door (tests/test_gpu_weighted_forms.py) and the conditions on them
(tests/test_weighted_form_cases_host.py): numpy only, importable without a GPU, deterministic in (door, k, variant).

nnlm_set_matrix_csc_weighted solves every column with a Gram of its own, G_j = c0 G_full + sum over the stored entries of
(c_e - c0) y y^T, c0 = 0 (door "weighted_missing": an absent entry is missing) or 1 ("weighted_zero": a zero of weight 1).  Besides the
solvers of tests/na_solver_cases.py it reaches (nnlm_amd/csrc):
  "spw"    sp_gram_kernel<T, NT, WT = true>       k_sparse_na.h   both doors, 2 types x NT 1 .. 4                            =  8
  "fixup"  sp_gram_fixup_kernel<KP>               k_sparse_na.h   columns of more than 2048 stored entries, 4 KP x Gfull     =  8
  "strict" colsolve_strict_kernel<NKQ, MASK, KR>  k_missing.h     weighted_zero with SCD in BOTH modes (colsolve_fast_ok)    = 14
The dispatch is restated here (solver_of, gram_of, fixup_of) next to nc.solver_of / nc.gram_of; test_gpu_weighted_forms.py pins it to
what the library reports ("na_solver_*", "na_gram_*", "sparse_weighted" of nnlm_get_info).

The main case is nc.make_case(k, variant) unchanged -- 150 x 165, the finite entries are the stored ones, five special lines with an
empty and a full one among them -- with one weight per stored entry (weights_of).  weighted_zero: confidences 1 + 40 u, about 10 %
exactly 1 (c - c0 = 0), about 10 % in (0.05, 0.95) (c - c0 < 0), about 5 % exactly 0.  weighted_missing: {0, 0.25, 1, 3.5}.  Line
ZERO_LINE of the orientation that has the special lines is one more special line: its stored entries all carry weight 0, so its cross
product is zero although entries are stored; under weighted_missing its Gram is zero too, under weighted_zero it is G_full minus the
whole sum over the stored rows (c - c0 = -1 throughout: the Gram of the absent rows, formed by cancellation), and the solution is 0 as for
the line without stored entries.  The lines with KEEP = 72
stored entries keep full rank at k = 64 as in na_solver_cases.py: their weights of 0 are replaced by 0.25.

The reference is weighted_cases.half_step: the C oracle on the sqrt(c)-scaled one-column problems."""
import functools

import numpy as np

import na_solver_cases as nc
import sparse_cases as spc
import weighted_cases as wc
from oracle import nnlm_oracle, ref

DOORS = ("weighted_missing", "weighted_zero")
ABSENT = {"weighted_missing": "missing", "weighted_zero": "zero"}
C0 = {"weighted_missing": 0.0, "weighted_zero": 1.0}
MODES = nc.MODES
KS, RANK_ENDS = nc.KS, nc.RANK_ENDS
TIGHT, LOOSE = nc.TIGHT, nc.LOOSE
# columns stop BETWEEN sweeps: at (30, 1e-9) nearly every column runs to the limit and the count says little
MID = (300, 1e-5)
ZERO_LINE = 5                   # the line whose stored entries all carry weight 0 (see the module docstring)
MISSING_WEIGHTS = (0.0, 0.25, 1.0, 3.5)
TYPE_OF = {"f64": "double", "f32": "float"}


# ---- the dispatch, restated -----------------------------------------------------------------------------------------------------------------
def solver_of(mode, door, method, k, masked):
    """(instantiation, family code, KR) of the per-column solver: weighted_missing is the sparse door's; weighted_zero solves SCD in fp64
    (colsolve_strict_kernel with its KR rule) in both modes -- colsolve_fast_ok is false there."""
    if door == "weighted_zero" and method == 1:
        return nc.solver_of("f64", 1, k, masked)
    return nc.solver_of(mode, method, k, masked)


def gram_of(mode, door, k):
    """(instantiation, family code, NT): sp_gram_kernel<T, NT, true>; "na_gram" reports the sp family (3), "sparse_weighted" tells the WT form."""
    assert door in DOORS and 1 <= k <= 64
    NKQ = (k + 15) // 16
    return ("spw", TYPE_OF[mode], NKQ), nc.GRAM_CODE["sp"], NKQ


def fixup_of(door, k):
    """sp_gram_fixup_kernel<KP> and whether its Gfull branch adds the shared Gram."""
    return ("fixup", spc.kp_of(k), door == "weighted_zero")


def info_of(mode, door, method, k, masked):
    _, s, kr = solver_of(mode, door, method, k, masked)
    _, g, nt = gram_of(mode, door, k)
    return (s, kr, g, nt)


def all_gram_instantiations():
    return {("spw", t, nt) for t in ("double", "float") for nt in (1, 2, 3, 4)}


def all_strict_instantiations():
    return {i for i in nc.all_instantiations() if i[0] == "strict"}


def all_fixup_instantiations():
    return {("fixup", kp, g) for kp in (16, 32, 48, 64) for g in (False, True)}


def settings_of(k):
    """(name, setting, method) of the every-rank test."""
    s = (("tight", TIGHT, 1), ("loose", LOOSE, 1), ("lee", TIGHT, 2))
    return s + ((("mid", MID, 1),) if k in RANK_ENDS else ())


def case_name(door, k, variant, setting, side):
    return f"{door}-{nc.case_name(k, variant, setting)}-{side}"


# Strict sweep counts of weighted_zero that differ between the sqrt(c)-scaled problem and the library's formulation G_full + sum (c - 1) y y^T,
# both in fp64 on the CPU (test_weighted_form_cases_host.py asserts that this is the set and that it holds at most 3): names of
# case_name(); the GPU count is compared exactly everywhere else.
FORMULATION_DEPENDENT = frozenset()
MAX_FORMULATION_DEPENDENT = 3
EMPTY_LINE = 4                  # the line of nc.make_case without an observed entry


def rounding_decided_columns(door, variant, side):
    """The columns whose sweep count no formulation fixes.  Under weighted_zero the line without stored entries is an all-zero column of
    weight 1 -- G = G_full, b = 0, the solution is 0 -- and ZERO_LINE, whose stored entries all carry weight 0, is an all-zero column
    over its absent rows.  With an L1 penalty every formulation clamps them to exact zeros in the same sweep; without one the
    coordinate descent leaves them at the rounding dust of G x / G_qq, and the sweep at which that dust stops counting as a change is
    decided by the rounding of the Gram itself (sparse_cases.make_case says the same of the plain zero door): the two fp64
    formulations on the CPU give 5 against 9 sweeps for the empty line at k = 20 and 30 against 4 at k = 50, and agree on every
    other column.  The variants without penalties have the special lines among the rows, so these are rows EMPTY_LINE and ZERO_LINE of
    the W half-step.  The GPU count is compared with those columns taken out: each may take any 1 .. limit sweeps, the rest must add
    up exactly."""
    masked, pen = nc.VARIANTS[variant]
    return (EMPTY_LINE, ZERO_LINE) if door == "weighted_zero" and not pen and nc.ROWS_SPECIAL[variant] and side == "w" else ()


def count_bounds(total_ref, counts_ref, columns, limit):
    """(lo, hi) of a half-step's sweep count: the reference's, with each of rounding_decided_columns() free within 1 .. limit."""
    if not columns or limit == 0:
        return total_ref, total_ref
    rest = total_ref - sum(counts_ref[j] for j in columns)
    return rest + len(columns), rest + limit * len(columns)


# ---- weights and problems -------------------------------------------------------------------------------------------------------------------
def line_entries(S, by_rows, line):
    """Stored entries (bool over the CSC order) of row / column `line`."""
    indptr, idx, _, (n, m) = S
    if by_rows:
        return idx == line
    return np.repeat(np.arange(m), np.diff(indptr)) == line


def draw_weights(door, size, rng):
    if door == "weighted_missing":
        return rng.choice(MISSING_WEIGHTS, size)
    w = 1.0 + 40.0 * rng.random(size)
    r, u = rng.random(size), rng.random(size)
    w[r < 0.10] = 1.0
    below = (r >= 0.10) & (r < 0.20)
    w[below] = 0.05 + 0.9 * u[below]
    w[(r >= 0.20) & (r < 0.25)] = 0.0
    return w


@functools.lru_cache(maxsize=16)
def weights_of(door, k, variant):
    """One weight per stored entry of nc.csc_of(nc.make_case(k, variant)["A"]), in its order."""
    c = nc.make_case(k, variant)
    S = nc.csc_of(c["A"])
    rng = np.random.default_rng(9000000 + 1000000 * DOORS.index(door) + 100000 * list(nc.VARIANTS).index(variant) + 1000 * k)
    w = draw_weights(door, S[2].size, rng)
    rows = c["rows_special"]
    if door == "weighted_missing":
        for by_rows, line in ((rows, 3), (not rows, 2)):   # the lines with KEEP stored entries
            e = line_entries(S, by_rows, line)
            w[e & (w == 0.0)] = 0.25
    w[line_entries(S, rows, ZERO_LINE)] = 0.0
    w.setflags(write=False)
    return w


def _problem(door, c, S, w):
    A, C, obs = wc.dense_parts(S, w, ABSENT[door])
    St = wc.transpose(*S)
    wt = wc.transpose(S[0], S[1], w, S[3])[2]
    return dict(door=door, c=c, S=S, w=w, St=St, wt=wt, A=A, C=C, obs=obs, At=np.ascontiguousarray(A.T), Ct=np.ascontiguousarray(C.T),
                obst=np.ascontiguousarray(obs.T))


@functools.lru_cache(maxsize=8)
def problem(door, k, variant):
    """dict(door, c = nc.make_case(k, variant), S the CSC of its finite entries, w, St / wt the CSR side, and the dense A, C, obs of
    weighted_cases.dense_parts with their transposes)."""
    c = nc.make_case(k, variant)
    return _problem(door, c, nc.csc_of(c["A"]), weights_of(door, k, variant))


# ---- the reference --------------------------------------------------------------------------------------------------------------------------
def oracle_w(P, inner, tol, method=1, counts=None):
    """(W n x k, sweeps) of the reference's W half-step from (W0, H0)."""
    c = P["c"]
    Wt, it = wc.half_step(c["W0"].T, c["H0"], P["At"], P["Ct"], P["obst"], None if c["Wm"] is None else c["Wm"].T, c["reg"], inner, tol, method,
                          P["door"] == "weighted_missing", counts)
    return np.ascontiguousarray(Wt.T), int(it)


def oracle_h(P, W, inner, tol, method=1, counts=None):
    """(H k x m, sweeps) of the reference's H half-step from the factor W."""
    c = P["c"]
    H, it = wc.half_step(c["H0"], np.ascontiguousarray(W.T), P["A"], P["C"], P["obs"], c["Hm"], c["reg"], inner, tol, method,
                         P["door"] == "weighted_missing", counts)
    return np.ascontiguousarray(H), int(it)


@functools.lru_cache(maxsize=64)
def oracle_w_cached(door, k, variant, setting, method=1):
    return oracle_w(problem(door, k, variant), setting[0], setting[1], method)


def stop_oracles(P):
    """(oracle_w, oracle_h) with the signatures scd_sweep_cases.stop_slack calls."""
    return (lambda ref_, c, inner, tol: oracle_w(P, inner, tol)), (lambda ref_, c, W, inner, tol: oracle_h(P, W, inner, tol))


def stop_slack(P, which, X, X_ref, W_fixed, setting, bar):
    return nc.sc.stop_slack(ref, P["c"], which, X, X_ref, W_fixed, setting, bar, oracles=stop_oracles(P))


def library_form_half_step(P, which, W, inner, tol, solver=None):
    """The SCD half-step `which` (0: W from (W0, H0); 1: H from the factor W) in the LIBRARY's formulation, in numpy fp64:
    G_j = c0 G_full + sum over the stored entries of (c_e - c0) y y^T, b_j = sum of c_e a_e y, nnlm_oracle._gram_edits, then the reference's
    per-column solver (solver: nnlm_oracle.scd_ls_update's signature; default its C twin ref.scd_ls_update).  Returns (X, [sweeps of
    every column])."""
    c, c0 = P["c"], C0[P["door"]]
    solver = solver or ref.scd_ls_update
    if which == 0:
        (ptr, idx, val, _), w, X, Yt, mask = P["St"], P["wt"], np.array(c["W0"].T), c["H0"], None if c["Wm"] is None else c["Wm"].T
    else:
        (ptr, idx, val, _), w, X, Yt, mask = P["S"], P["w"], np.array(c["H0"]), np.ascontiguousarray(W.T), c["Hm"]
    reg = c["reg"]
    Gfull = Yt @ Yt.T
    counts = []
    for j in range(X.shape[1]):
        if mask is not None and mask[:, j].all():
            counts.append(0)
            continue
        e0, e1 = int(ptr[j]), int(ptr[j + 1])
        Yj, cj = Yt[:, idx[e0:e1]], w[e0:e1]
        G = (Yj * (cj - c0)) @ Yj.T
        if c0:
            G = Gfull + G
        G = nnlm_oracle._gram_edits(G, reg)
        x = np.ascontiguousarray(X[:, j])
        mu = G @ x - Yj @ (cj * val[e0:e1])
        if reg[2] != 0:
            mu += reg[2]
        counts.append(int(solver(x, G, mu, None if mask is None else mask[:, j], inner, tol)))
        X[:, j] = x
    return (np.ascontiguousarray(X.T) if which == 0 else X), counts


# ---- segments and the fix-up ----------------------------------------------------------------------------------------------------------------
WIDE_N = 4200
WIDE_LENS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 4200)
# The order of the columns (found by a search over sparse_cases.boundary_events, pinned by the host test): 255 + 1 entries put the start of
# the 4096-entry column on a worker boundary of the unchunked launch (256 entries per worker), so its second segment starts on one too;
# under WIDE_SLOTS Gram slots per chunk a long column is first in a chunk and another is last.
WIDE_ORDER = (255, 1, 4096, 0, 2, 3, 4097, 4, 5, 7, 8, 9, 12, 13, 15, 16, 2049, 4200, 17, 31, 32, 33, 4095, 63, 64, 65, 256, 257, 2047, 2048)
WIDE_SLOTS = 8
WIDE_KS = nc.ROWLIST_KS
WIDE_T_KS = (16, 32, 48, 64)
WIDE_SETTING = nc.ROWLIST_SETTING


def wide_alloc_limit(k):
    return WIDE_SLOTS * spc.kp_of(k) ** 2 * 8


@functools.lru_cache(maxsize=4)
def wide_problem(door, k, transposed=False):
    """A 4200 x 30 matrix with WIDE_ORDER[j] stored entries in column j, values U(0.1, 1.1), the door's weights, reg = REG; transposed: its
    transpose (30 x 4200: the W half-step's CSR holds the long lines)."""
    rng = np.random.default_rng(515000 + 100 * DOORS.index(door) + k)
    n, m = WIDE_N, len(WIDE_ORDER)
    P = np.zeros((n, m), dtype=bool)
    for j, L in enumerate(WIDE_ORDER):
        P[rng.choice(n, L, replace=False), j] = True
    S = spc.csc_from_pattern(P, 0.1 + rng.random((n, m)))
    w = draw_weights(door, S[2].size, rng)
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    if transposed:
        w = wc.transpose(S[0], S[1], w, S[3])[2]
        S = wc.transpose(*S)
        W0, H0, n, m = np.ascontiguousarray(H0.T), np.ascontiguousarray(W0.T), m, n
    c = dict(k=k, n=n, m=m, variant="wide" + ("^T" if transposed else ""), W0=W0, H0=H0, Wm=None, Hm=None, reg=list(nc.REG))
    return _problem(door, c, S, w)


def segment_starts(indptr, slots=0, cus=spc.DEFAULT_CUS):
    """[(column, segment s >= 1, on a worker boundary)] of every later segment of every long column, per chunk of the Gram plan under
    `slots` Gram slots per chunk (0: one chunk)."""
    ptr = np.asarray(indptr, dtype=np.int64)
    out = []
    for c0, c1 in spc.gram_chunks(ptr, 16, slots * 16 * 16 * 8):
        E0, E1 = int(ptr[c0]), int(ptr[c1])
        nw = spc.spg_workers(E1 - E0, cus)
        chunk, ranges = spc.split_of(E1 - E0, nw)
        bounds = {E0 + e0 for e0, e1 in ranges[1:] if e0 < e1}
        for c in range(c0, c1):
            for s in range(1, spc.segments_of(int(ptr[c + 1] - ptr[c]))):
                out.append((c, s, int(ptr[c]) + s * spc.SPG_SEG in bounds))
    return out
