"""Cases for the two- and one-lane forms of the Lee sweep (tests/test_gpu_lee_forms.py) and the conditions on them
(tests/test_lee_cases_host.py): numpy only, importable without a GPU, deterministic in (n, k).

sweep_ls_kernel<R, L, 2> (nnlm_amd/csrc/k_sweep.h) solves every square-loss half-step of method 2 at ranks up to 64.  launch_sweep()
picks L from the END column of the launch alone and R from k and L; the rule is restated here (lanes_of, regs_of) so that a test can say
which of the 24 instantiations a case reaches, and test_gpu_lee_forms.py pins the restatement to what the library reports
("lee_lanes_w" / "lee_regs_w" of nnlm_get_info).

A case is the W half-step of an n x 24 matrix: n is the number of columns the sweep solves.  The oracle sees it as
ref.update(W0.T, H0, A.T, Wm.T, ...)."""
import functools

import numpy as np

M = 24
REG = [0.02, 0.01, 0.03]
SLOTS = 4096  # wavefronts the launch may have before it takes fewer lanes per column (sweep_lanes_per_column)

# (n, the form it takes, why)
NS = (65536,    # L = 4: last count of the form the rest of the suite runs (control)
      65537,    # L = 2: first; the last wavefront holds one column
      131072,   # L = 2: last
      131073,   # L = 1: first
      131110)   # L = 1: ragged, 38 columns in the last wavefront
# both ends of each of the eight R values of L = 2 and of L = 1; the odd ranks leave one live coordinate in L = 2's last pair; 64 takes the
# kmask = ~0 branch and mask bit 63
KS = (1, 8, 9, 16, 17, 24, 25, 32, 33, 40, 41, 48, 49, 56, 57, 64)
KS_FEW = (9, 40, 64)

# every (n, k) the oracle-parity test runs
PARITY_CASES = tuple((n, k) for n in (65537, 131110) for k in KS) + tuple((n, k) for n in (131072, 131073, 65536) for k in KS_FEW)


# ---- the dispatch rule of launch_sweep(), restated -----------------------------------------------------------------------------------------
def lanes_of(ncols):
    """sweep_lanes_per_column: the largest L of 4, 2, 1 whose ceil(L ncols / 64) wavefronts fit SLOTS."""
    for L in (4, 2):
        if (L * ncols + 63) // 64 <= SLOTS:
            return L
    return 1


def regs_of(k, L):
    """Coordinate registers per lane: ceil(k / L) rounded up to the instantiated step 8 / L."""
    step = 8 // L
    need = (k + L - 1) // L
    return step * ((need + step - 1) // step)


def form_of(ncols, k):
    """(L, R) of the sweep_ls_kernel<R, L, 2> launch that solves columns ending at ncols at rank k."""
    L = lanes_of(ncols)
    return L, regs_of(k, L)


def masked_rows(n):
    """The fully masked rows of a case: row 3, the last row, and the last row of the last full wavefront."""
    cpw = 64 // lanes_of(n)
    return sorted({3, n - 1, (n // cpw) * cpw - 1})


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
def make_case(n, k):
    """dict(A n x 24, W0 n x k, H0 k x 24, Wm bool n x k): low-rank data plus noise, factors on the scale of the data and bounded away
    from zero, 5 % of W masked and three rows of it masked entirely."""
    rng = np.random.default_rng(n + k)
    A = rng.random((n, 5)) @ rng.random((5, M)) + 0.1 * rng.random((n, M))
    W0 = 0.3 * rng.random((n, k)) + 0.05
    H0 = 0.3 * rng.random((k, M)) + 0.05
    Wm = rng.random((n, k)) < 0.05
    Wm[masked_rows(n), :] = True
    return dict(n=n, m=M, k=k, A=A, W0=W0, H0=H0, Wm=Wm)


def live_columns(c):
    """Columns of the W half-step (rows of W) that are not fully masked: the ones update() solves."""
    return int((~c["Wm"].all(axis=1)).sum())


def oracle_w(ref, c, inner, tol, mask=True, reg=REG, reverse=False):
    """(W n x k, sweeps) of the oracle's W half-step by Lee's updates.  reverse: the contraction (the 24 columns of A and of H) in the
    opposite order -- the same sums in another order of addition."""
    A, H0 = (c["A"][:, ::-1], c["H0"][:, ::-1]) if reverse else (c["A"], c["H0"])
    Wt, it = ref.update(c["W0"].T, H0, A.T, c["Wm"].T if mask else None, reg, inner, tol, 2)
    return np.ascontiguousarray(Wt.T), int(it)


# the other orientation (an H half-step on the transposed problem): one rank with more than one register chunk per form
H_CASES = ((65537, 40), (131110, 40))
# no penalties, no mask: the widest instantiation of each form (R = 32 at L = 2, R = 64 at L = 1)
PLAIN_CASES = ((65537, 57), (131110, 57))
# form against form: the first n - 1 rows of the case as a matrix of their own take the next wider form
PAIR_CASES = tuple((n, k) for n in (65537, 131073) for k in (17, 64))


def head_of(c, rows):
    """The first `rows` rows of the case as a case of their own: same fixed factor, same Gram."""
    return dict(c, n=rows, A=np.ascontiguousarray(c["A"][:rows]), W0=np.ascontiguousarray(c["W0"][:rows]), Wm=np.ascontiguousarray(c["Wm"][:rows]))


def sparse_case(n=131110, k=20, density=0.3):
    """The case with about 30 % of A kept and the rest zero: (case on the dense form, boolean pattern)."""
    c = make_case(n, k)
    P = np.random.default_rng(n + k + 1).random(c["A"].shape) < density
    return dict(c, A=c["A"] * P), P


def nnlm_case(q=131110, k=20, rows=30):
    """nnlm(x rows x k, y rows x q): q regressions sharing x -- update() with rank k on q columns.  dict(x, y, b0, mask)."""
    rng = np.random.default_rng(q + k + rows)
    x = rng.random((rows, k)) + 0.02
    b = rng.random((k, q)) * (rng.random((k, q)) > 0.3)
    y = x @ b + 0.02 * rng.random((rows, q)) + 0.01
    b0 = 0.3 * rng.random((k, q)) + 0.05
    mask = rng.random((k, q)) < 0.05
    mask[:, masked_rows(q)] = True
    return dict(x=x, y=y, b0=b0, mask=mask)


# ---- early finishers -------------------------------------------------------------------------------------------------------------------------
# (n, k): one case per form with more than one register chunk (R = 20 at L = 2, R = 40 at L = 1)
EARLY_CASES = ((65537, 40), (131110, 40))
# (inner sweeps, inner tolerance) tried in this order; the first at which some but not all live columns stop before the budget is taken.
# (30, 1e-2) is not in the list: from this start Lee's updates move some coordinate of every column by more than 1 % per sweep for 30
# sweeps at k >= 33 -- the oracle runs the whole budget on every column and only k = 1 stops early; at 3e-2 a few dozen columns do.
EARLY_SETTINGS = ((30, 1e-1), (30, 3e-1), (60, 1e-1))


def early_ok(c, inner, sweeps):
    """Some column stopped early, and not every column after its first sweep."""
    live = live_columns(c)
    return live < sweeps < inner * live


@functools.lru_cache(maxsize=None)
def early_setting(ref, n, k):
    """(inner, tol, W, sweeps) of the first setting of EARLY_SETTINGS at which the oracle's sweep total lies strictly between the number
    of live columns and inner times that number; None if there is none."""
    c = make_case(n, k)
    for inner, tol in EARLY_SETTINGS:
        W, it = oracle_w(ref, c, inner, tol)
        if early_ok(c, inner, it):
            return inner, tol, W, it
    return None


@functools.lru_cache(maxsize=None)
def early_order_slack(ref, n, k):
    """By how many sweeps the oracle's total differs between its two summation orders at the early-finisher setting (measured: 0)."""
    inner, tol, _, it = early_setting(ref, n, k)
    _, itr = oracle_w(ref, make_case(n, k), inner, tol, reverse=True)
    return abs(it - itr)
