"""Cases for every instantiation of the square-loss half-step with missing entries (tests/test_gpu_na_forms.py) and the conditions on them
(tests/test_na_solver_cases_host.py): numpy only, importable without a GPU, deterministic in (k, variant).

update_with_missing solves every column with a Gram of its own.  Dense A with NaN (set_matrix) and sparse A whose absent entries are
missing (set_matrix_csc_missing) end in the same per-column solvers and one of three per-column Gram families (nnlm_amd/csrc), 47
template instantiations at ranks up to 64:
  "row"     colsolve_row_kernel<CPL, HAS_MASK, KR>      k_colsolve_row.h / tu_colsolve.hip   fp32-operand mode, SCD      5 classes x mask = 10
  "strict"  colsolve_strict_kernel<NKQ, HAS_MASK, KR>   k_missing.h                          strict mode, SCD            7 x mask         = 14
  "ls"      colsolve_ls_kernel<NKQ, 2>                  k_missing.h                          Lee's updates, both modes                    =  4
  "lds"     na_gram_lds_kernel<double, NT, TAIL>        k_missing.h                          strict mode, dense A with NaN                =  7
  "f16"     na_gram_f16_kernel<NKQ>                     k_missing.h                          fp32-operand mode, dense A with NaN          =  4
  "sp"      sp_gram_kernel<T, NT> (plain form)          k_sparse_na.h                        sparse A, absent = missing   2 types x 4     =  8
The dispatch rules of launch_colsolve, nnlm_tu_colsolve_row, launch_colsolve_strict_m, launch_na_gram and the sparse door's Gram launch
(nnlm_mi355x.hip, tu_colsolve.hip, tu_sparse.hip) are restated here (solver_of, gram_of) so that a test can say which instantiation a
case reaches; test_gpu_na_forms.py pins the restatement to what the library reports ("na_solver_*", "na_gram_*" of nnlm_get_info).

The main case is a 150 x 165 matrix with values U(0.1, 1.1) and 20 % NaN: the W half-step solves 150 columns over a contraction of 165,
the H half-step 165 columns over 150; 150 = 9 * 16 + 6 = 37 * 4 + 2 and 165 = 10 * 16 + 5 = 41 * 4 + 1 are ragged for both workgroup
shapes (16 columns: colsolve_row_kernel; 4: every other kernel).  Five lines are special: nothing missing (an empty row list), exactly
one missing, seven (4 + 3), all but 72 missing (the list then holds the present rows; 72 >= 64 keeps the Gram of full rank) and
everything missing.  A line with nothing missing in one orientation and a line with everything missing in the other cannot live in one
matrix, so a case has the five in ONE orientation -- lines 0 .. 4 -- and, in the other, lines 0 .. 2 with one, seven and all but 72
missing: the variants "plain" and "mask_nopen" have the five among the rows (the W half-step), "masked" and "pen_nomask" among the
columns (the H half-step), so every rank sees both."""
import collections
import functools

import numpy as np

import scd_sweep_cases as sc

N, M = 150, 165
KS = tuple(range(1, 65))
REG, NOREG = sc.REG, sc.NOREG
TIGHT, LOOSE = (30, 1e-9), (30, 1e-1)
SETTINGS = (("tight", TIGHT), ("loose", LOOSE))
# inner limits 0 and 1, and a negative tolerance (the `0.0 > tol` branch: no column stops before the limit) with a limit of 7
LIMIT_SETTINGS = (("limit0", (0, 1e-9)), ("limit1", (1, 1e-9)), ("negtol", (7, -1.0)))
# both ends of every class of every solver family: k <= 16, 32, 48, 50, 64 (row); 16 NKQ and the short forms 17 .. 20, 33 .. 36, 49 .. 52
# with the first rank beyond each (strict)
RANK_ENDS = (1, 16, 17, 18, 19, 20, 21, 32, 33, 34, 35, 36, 37, 48, 49, 50, 51, 52, 53, 64)
VARIANTS = sc.VARIANTS      # variant -> (masked, penalties)
ROWS_SPECIAL = {"plain": True, "masked": False, "mask_nopen": True, "pen_nomask": False}   # the five special lines: rows or columns of A
KEEP = 72                   # observed entries of the "all but 72 missing" line
MASK_RATE = 0.15
MASKED_LINE_W, MASKED_LINE_H = 9, 14   # fully masked lines, inside the wavefronts of lines 8 .. 11 and 12 .. 15

SOLVER_CODE = {"row": 0, "strict": 1, "ls": 2, "generic": 3}              # "na_solver_*" of nnlm_get_info
GRAM_CODE = {"f16": 0, "lds": 1, "lds_tail": 2, "sp": 3, "generic": 4}    # "na_gram_*"
ROW_CLASSES = ((1, 16), (2, 32), (3, 48), (4, 50), (4, 64))               # (CPL, KR) of colsolve_row_kernel (tu_colsolve.hip)
MODES, DOORS = ("f64", "f32"), ("dense", "sparse")


# ---- the dispatch, restated -----------------------------------------------------------------------------------------------------------------
def row_class(k):
    """(CPL, KR) of nnlm_tu_colsolve_row."""
    return next(c for c in ROW_CLASSES if k <= c[1])


def solver_of(mode, method, k, masked):
    """(instantiation, family code, KR) of the per-column solver launch_colsolve launches: mode "f64" / "f32", method 1 SCD / 2 Lee."""
    assert 1 <= k <= 64 and method in (1, 2)
    NKQ = (k + 15) // 16
    if method == 2:
        return ("ls", NKQ), SOLVER_CODE["ls"], 16 * NKQ
    if mode == "f32":
        cpl, kr = row_class(k)
        return ("row", cpl, bool(masked), kr), SOLVER_CODE["row"], kr
    ks = 16 * (NKQ - 1) + 4
    kr = ks if NKQ > 1 and k <= ks else 16 * NKQ
    return ("strict", NKQ, bool(masked), kr), SOLVER_CODE["strict"], kr


def gram_of(mode, door, k):
    """(instantiation, family code, NT) of the per-column Gram launch: launch_na_gram (door "dense") or nnlm_tu_sp_gram ("sparse")."""
    assert 1 <= k <= 64
    NKQ = (k + 15) // 16
    if door == "sparse":
        return ("sp", "double" if mode == "f64" else "float", NKQ), GRAM_CODE["sp"], NKQ
    if mode == "f32":
        return ("f16", NKQ), GRAM_CODE["f16"], NKQ
    if NKQ >= 2 and k - 16 * (NKQ - 1) in (1, 2):   # tail coordinates on the VALU: k = 17, 18, 33, 34, 49, 50
        return ("lds", NKQ - 1, True), GRAM_CODE["lds_tail"], NKQ - 1
    return ("lds", NKQ, False), GRAM_CODE["lds"], NKQ


def info_of(mode, door, method, k, masked):
    """What nnlm_get_info reports for a half-step: (na_solver, na_solver_kr, na_gram, na_gram_nt)."""
    _, s, kr = solver_of(mode, method, k, masked)
    _, g, nt = gram_of(mode, door, k)
    return (s, kr, g, nt)


def all_instantiations():
    """The 47 instantiations of the six families."""
    out = set()
    for mk in (False, True):
        for cpl, kr in ROW_CLASSES:
            out.add(("row", cpl, mk, kr))
        out.add(("strict", 1, mk, 16))
        for nkq in (2, 3, 4):
            out.add(("strict", nkq, mk, 16 * nkq))
            out.add(("strict", nkq, mk, 16 * (nkq - 1) + 4))
    for nkq in (1, 2, 3, 4):
        out.add(("ls", nkq))
        out.add(("f16", nkq))
        out.add(("lds", nkq, False))
        if nkq < 4:
            out.add(("lds", nkq, True))
        for t in ("double", "float"):
            out.add(("sp", t, nkq))
    return out


def variants_of(k):
    return tuple(VARIANTS) if k in RANK_ENDS else ("plain", "masked")


def case_name(k, variant, setting):
    return f"k{k}-{variant}-{setting}"


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
def missing_pattern(nl, nc, rng):
    """bool [nl][nc], True = missing: 20 % at random; lines (rows) 0 .. 4 with nothing, one, seven, all but KEEP and all of their entries
    missing; cross lines (columns) 0 .. 2 with one (the entry of line 4), seven and all but KEEP."""
    miss = rng.random((nl, nc)) < 0.20
    miss[:, 0] = False
    miss[:, 1] = False
    miss[5 + rng.choice(nl - 5, 6, replace=False), 1] = True         # + line 4 below: seven
    miss[:, 2] = True
    miss[5 + rng.choice(nl - 5, KEEP - 4, replace=False), 2] = False  # + lines 0 .. 3 below: KEEP present
    miss[0] = False
    miss[1] = False
    miss[1, 5 + rng.integers(nc - 5)] = True
    miss[2] = False
    miss[2, 5 + rng.choice(nc - 5, 7, replace=False)] = True
    miss[3] = True
    miss[3, :5] = False
    miss[3, 5 + rng.choice(nc - 5, KEEP - 5, replace=False)] = False
    miss[4] = True
    return miss


def masks(n, m, k, rng):
    """Wm n x k, Hm k x m: MASK_RATE of the entries, one fully masked line per orientation whose three wavefront neighbours keep a free
    coordinate."""
    Wm, Hm = rng.random((n, k)) < MASK_RATE, rng.random((k, m)) < MASK_RATE
    HmT = Hm.T
    for Xm, line in ((Wm, MASKED_LINE_W), (HmT, MASKED_LINE_H)):
        Xm[line] = True
        for nb in range(line // 4 * 4, line // 4 * 4 + 4):
            if nb != line and Xm[nb].all():
                Xm[nb, 0] = False
    return Wm, np.ascontiguousarray(HmT.T)


@functools.lru_cache(maxsize=8)
def make_case(k, variant):
    """dict(A n x m with NaN, W0 n x k, H0 k x m, Wm, Hm (bool or None), reg).  The start is U(0, 1) scaled so that W0 H0 is of A's size, with
    5 % zeros; masked entries of the start hold values other than zero."""
    masked, pen = VARIANTS[variant]
    rng = np.random.default_rng(7000000 + 100000 * list(VARIANTS).index(variant) + 1000 * k)
    n, m = N, M
    A = 0.1 + rng.random((n, m))
    miss = missing_pattern(n, m, rng) if ROWS_SPECIAL[variant] else np.ascontiguousarray(missing_pattern(m, n, rng).T)
    A[miss] = np.nan
    s = np.sqrt(2.4 / k)
    W0, H0 = s * rng.random((n, k)), s * rng.random((k, m))
    W0[rng.random((n, k)) < 0.05] = 0.0
    H0[rng.random((k, m)) < 0.05] = 0.0
    Wm = Hm = None
    if masked:
        Wm, Hm = masks(n, m, k, rng)
        W0[Wm] = 0.3 * W0[Wm] + 0.02
        H0[Hm] = 0.3 * H0[Hm] + 0.02
    for a in (A, W0, H0):
        a.setflags(write=False)
    return dict(k=k, n=n, m=m, variant=variant, A=A, W0=W0, H0=H0, Wm=Wm, Hm=Hm, reg=list(REG if pen else NOREG), rows_special=ROWS_SPECIAL[variant])


def live_columns(c):
    """Columns of the W half-step (rows of W) that are not masked entirely: the ones update_with_missing solves."""
    return c["n"] if c["Wm"] is None else int((~c["Wm"].all(axis=1)).sum())


def live_columns_h(c):
    return c["m"] if c["Hm"] is None else int((~c["Hm"].all(axis=0)).sum())


def csc_of(A):
    """(indptr, indices, data, shape) of the observed (finite) entries of A: the sparse door's view of the same problem."""
    obs = np.isfinite(A)
    indptr = np.concatenate(([0], np.cumsum(obs.sum(axis=0)))).astype(np.int64)
    cols, rows = np.nonzero(obs.T)   # column-major order, rows ascending within a column
    return indptr, rows.astype(np.int32), np.ascontiguousarray(A.T[obs.T]), A.shape


def oracle_w(ref, c, inner, tol, method=1, perm=None):
    """(W n x k, sweeps) of the oracle's W half-step.  perm: the contraction (the m columns of A and of H) in that order -- the same sums
    in another order of addition."""
    A, H0 = (c["A"], c["H0"]) if perm is None else (c["A"][:, perm], c["H0"][:, perm])
    Wt, it = ref.update(c["W0"].T, H0, A.T, None if c["Wm"] is None else c["Wm"].T, c["reg"], inner, tol, method, missing=True)
    return np.ascontiguousarray(Wt.T), int(it)


def oracle_h(ref, c, W, inner, tol, method=1, perm=None):
    """(H k x m, sweeps) of the oracle's H half-step from the factor W; perm: the n rows of A and of W in that order."""
    A, W = (c["A"], W) if perm is None else (c["A"][perm], W[perm])
    H, it = ref.update(c["H0"], W.T, A, c["Hm"], c["reg"], inner, tol, method, missing=True)
    return np.ascontiguousarray(H), int(it)


@functools.lru_cache(maxsize=64)
def oracle_w_cached(ref, k, variant, setting, method=1):
    return oracle_w(ref, make_case(k, variant), setting[0], setting[1], method)


def column_counts_w(ref, c, inner, tol, A=None, W0=None, H0=None):
    """Sweeps of every column of the W half-step, one ref.update per column (SCD); A, W0, H0: other inputs than the case's (rounded ones)."""
    A, W0, H0 = (c["A"] if A is None else A), (c["W0"] if W0 is None else W0), (c["H0"] if H0 is None else H0)
    out = np.zeros(c["n"], dtype=np.int64)
    for j in range(c["n"]):
        mk = None if c["Wm"] is None else c["Wm"][j:j + 1].T
        out[j] = ref.update(W0[j:j + 1].T, H0, A[j:j + 1].T, mk, c["reg"], inner, tol, 1, missing=True)[1]
    return out


def stop_slack(ref, c, which, X, X_ref, W_fixed, setting, bar):
    """scd_sweep_cases.stop_slack on these cases' oracle (fp32-operand mode, loose setting: the sweep at which a column stops is
    tolerance-only; a column that misses the bar is held to it against the oracle's own trajectory)."""
    return sc.stop_slack(ref, c, which, X, X_ref, W_fixed, setting, bar, oracles=(oracle_w, oracle_h))


# Cases whose oracle sweep counts differ between two orders of the contraction (test_na_solver_cases_host.py asserts that this is the set
# and that it holds at most 3 cases): the strict GPU count is compared exactly everywhere else.
ORDER_DEPENDENT = frozenset()
MAX_ORDER_DEPENDENT = 3


# ---- the row-list case ----------------------------------------------------------------------------------------------------------------------
# missing rows per column: the list of test_missing_values_row_lists_around_the_gather_steps (tests/test_gpu_parity.py: around the 32-row
# gather steps, the fold every 256 rows, the switch between listing the missing and the present rows at one half of 1300) and the lengths
# around the four-row groups with their three-deep gather pipeline and clamped prologue.  A column with L > 650 missing rows lists its
# 1300 - L present rows; the sparse door gathers the 1300 - L stored rows of every column.
ROWLIST_N = 1300
ROWLIST_LENS = (0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 255, 256, 257, 288, 511, 512, 513, 600, 649, 650, 651, 700,
                1299) + (2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17)
ROWLIST_KS = (1, 16, 17, 18, 32, 33, 34, 48, 49, 64)
ROWLIST_SETTING = (4, 1e-9)


@functools.lru_cache(maxsize=4)
def make_rowlist_case(k):
    """dict(A 1300 x len(ROWLIST_LENS) with exactly ROWLIST_LENS[j] NaN in column j, W0, H0, reg = REG): the H half-step solves one column
    per length.  The column with one observed row has a Gram of rank 1: always with penalties."""
    rng = np.random.default_rng(4242 + k)
    n, m = ROWLIST_N, len(ROWLIST_LENS)
    A = rng.random((n, m)) + 0.1
    for j, L in enumerate(ROWLIST_LENS):
        A[rng.choice(n, L, replace=False), j] = np.nan
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    for a in (A, W0, H0):
        a.setflags(write=False)
    return dict(k=k, n=n, m=m, variant="rowlist", A=A, W0=W0, H0=H0, Wm=None, Hm=None, reg=list(REG))
