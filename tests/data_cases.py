"""Case generators for the data-content families (tests/test_gpu_data_families.py) and the conditions on them
(tests/test_data_cases_host.py): numpy only, importable without a GPU, deterministic in their arguments.

Every other dense parity test draws A from U(0, 1) or from a planted positive model plus a positive offset.  The families here keep the
planted model of test_gpu_fuzz.make_case (M = Wp Hp / (k + 3) * 4, starts near its factors) and change what A CONTAINS:

  counts      A = Poisson(s M), mean rate 0.5 / 1.5 / 4.0 by seed % 3 (about 60 %, 25 %, 3 % exact zeros); W0, H0 scaled by sqrt(s)
  zero_lines  M + 0.02 noise with rows 0, n // 2, n - 1 and columns 0, m // 2, m - 1 exactly zero
  na_lines    10 % NaN at random, rows 0, n - 1 and columns 0, m - 1 wholly NaN
  heavy       M exp(3 N(0, 1)): 1e-4 and 1e+4 in one column (every column spans at least 1e6)
  dup         columns 15, 16, 127, 128, m - 1 copies of column 0 (A and H0), rows 255, 256, n - 1 copies of row 0 (A and W0)
  exact_state deterministic, KL only: after the first coordinate step the state vector of a third of the rows is EXACTLY zero

Two combinations are not generated, both because of what the fp64 oracle itself does there (pinned in test_data_cases_host.py):
heavy x method 3 (two summation orders of the oracle differ by 0.2 .. 0.99) and na_lines x method 4 without an L1 term (the oracle's
result is NaN: 0 / 0 on a line with nothing observed)."""
import numpy as np

FAMILIES = ("counts", "zero_lines", "na_lines", "heavy")
SHAPES = ((257, 129, 17), (515, 131, 50), (131, 2100, 8))  # KP = 32, 64, 16; a ragged last 128-column tile; a contraction beyond 2048
SEEDS = (1, 2, 12)  # (seeds 0, 3, 6, 9: at 515 x 131, k = 50 a column of W is exactly 0 on the oracle's way under SCD-MSE -- factor_dies)
METHODS = (1, 2, 3, 4)
PENALTIES = ([0.0, 0.0, 0.0], [0.0, 0.0, 0.02])
RATES = (0.5, 1.5, 4.0)
MAX_ITER, TRACE = 4, 2
DUP_COLS, DUP_ROWS = (15, 16, 127, 128, -1), (255, 256, -1)  # a wavefront edge, a 128-column tile edge, the last line


def excluded(family, method, pen):
    return (family == "heavy" and method == 3) or (family == "na_lines" and method == 4 and PENALTIES[pen][2] == 0)


def _planted(rng, n, m, k):
    Wp, Hp = rng.random((n, k + 3)) ** 2 + 0.05, rng.random((k + 3, m)) ** 2 + 0.05
    M = Wp @ Hp / (k + 3) * 4
    sc = 2.0 / np.sqrt(k + 3)
    return M, Wp[:, :k] * sc * (0.7 + 0.6 * rng.random((n, k))), Hp[:k, :] * sc * (0.7 + 0.6 * rng.random((k, m)))


def _case(A, k, W0, H0, method, pen, **extra):
    reg = list(PENALTIES[pen])
    return dict(A=A, k=k, W0=W0, H0=H0, alpha=reg, beta=list(reg), method=method, inner=5 if method < 3 else 2, max_iter=MAX_ITER,
                trace=TRACE, pen=pen, **extra)


def make_case(family, seed, shape, method=None, pen=None):
    """Case `seed` of `family` at shape (n, m, k).  method (1 .. 4) and pen (index into PENALTIES, both sides alike) default to
    1 + seed % 4 and (seed // 4) % 2; the data depends on (family, seed, shape) only."""
    n, m, k = shape
    method = 1 + seed % 4 if method is None else method
    pen = (seed // 4) % 2 if pen is None else pen
    rng = np.random.default_rng(31000 + 100 * FAMILIES.index(family) + seed + 7 * n + m)
    M, W0, H0 = _planted(rng, n, m, k)
    if family == "counts":
        s = RATES[seed % 3] / M.mean()
        A = rng.poisson(s * M).astype(np.float64)
        W0, H0 = W0 * np.sqrt(s), H0 * np.sqrt(s)
    elif family == "zero_lines":
        A = M + 0.02 * rng.random((n, m))
        A[[0, n // 2, n - 1], :] = 0.0
        A[:, [0, m // 2, m - 1]] = 0.0
    elif family == "na_lines":
        A = M + 0.02 * rng.random((n, m)) + 0.01
        A[rng.random((n, m)) < 0.1] = np.nan
        A[[0, n - 1], :] = np.nan
        A[:, [0, m - 1]] = np.nan
    elif family == "heavy":
        Z = rng.standard_normal((n, m))
        cols = np.arange(m)
        Z[M.argmax(axis=0), cols], Z[M.argmin(axis=0), cols] = 2.6, -2.6  # (every column spans at least exp(15.6) = 6e6)
        A = M * np.exp(3.0 * Z)
    else:
        raise ValueError(family)
    return _case(A, k, W0, H0, method, pen, family=family, seed=seed, shape=shape)


def cases():
    """(family, seed, shape, method, pen) of every generated whole-run case: nothing but the two documented exclusions is left out."""
    return [(f, s, sh, me, p) for f in FAMILIES for sh in SHAPES for s in SEEDS for me in METHODS for p in range(len(PENALTIES))
            if not excluded(f, me, p)]


def case_id(t):
    f, s, sh, me, p = t
    return f"{f}-s{s}-{sh[0]}x{sh[1]}k{sh[2]}-m{me}-p{p}"


def dup_lines(n, m):
    """(rows, columns) that copy row 0 / column 0 at this size."""
    rows = sorted({r % n for r in DUP_ROWS if -n <= r < n} - {0})
    cols = sorted({c % m for c in DUP_COLS if -m <= c < m} - {0})
    return rows, cols


def make_dup_case(shape, method, with_na, pen=0):
    """Planted A with copies of column 0 and row 0 at a wavefront edge, a tile edge and the last line; with_na: 15 % NaN in column 0 and
    row 0 before the copying, so the copies share their pattern.  The crossing entries are equal by construction (columns are copied
    first: A[r, c] = A[0, c] = A[0, 0] = A[r, 0])."""
    n, m, k = shape
    rng = np.random.default_rng(47000 + 7 * n + m + int(with_na))
    M, W0, H0 = _planted(rng, n, m, k)
    A = M + 0.02 * rng.random((n, m)) + 0.01
    if with_na:
        A[rng.random(n) < 0.15, 0] = np.nan
        A[0, rng.random(m) < 0.15] = np.nan
    rows, cols = dup_lines(n, m)
    A[:, cols] = A[:, [0]]
    H0[:, cols] = H0[:, [0]]
    A[rows, :] = A[[0], :]
    W0[rows, :] = W0[[0], :]
    return _case(A, k, W0, H0, method, pen, family="dup", rows=rows, cols=cols, shape=shape)


def make_exact_state_case(method=3):
    """k = 2, n = 300, m = 40, every number a small dyadic rational so that the fp32 and the fp64 arithmetic are both exact on the way
    in.  W[:, 0] in {0.5, 1, 2}; W[:, 1] = 0 on every third row and in {16, 32, 64} elsewhere; H0[:, j] = (1, 0.5); A[:, j] = c_j W[:, 1] / 16
    with c_j in {5, 6, 7}: integers, zero where W[:, 1] is zero, and W H0 over-predicts them everywhere.  The first coordinate step of
    the KL coordinate descent therefore clamps coordinate 0 of every column to 0, the state w0 * 1 + 0 * 0.5 of the rows with
    W[:, 1] = 0 returns to EXACTLY 0 (x w is representable), and the step of coordinate 1 meets the quotient 0 / (0 + 1e-16) there."""
    n, m, k = 300, 40, 2
    i = np.arange(n)
    W = np.empty((n, k))
    W[:, 0] = np.array([0.5, 1.0, 2.0])[(i // 3) % 3]
    W[:, 1] = np.where(i % 3 == 0, 0.0, np.array([16.0, 32.0, 64.0])[(i // 5) % 3])
    H0 = np.tile(np.array([[1.0], [0.5]]), (1, m))
    c = 5.0 + np.arange(m) % 3
    A = np.outer(W[:, 1] / 16.0, c)
    reg = [0.0, 0.0, 0.0]
    return dict(A=A, k=k, W0=W, H0=H0, alpha=reg, beta=list(reg), method=method, inner=2, max_iter=3, trace=2, family="exact_state",
                shape=(n, m, k), pen=0)


def nnmf_args(c, max_iter=None):
    return (c["A"], c["k"], c["W0"], c["H0"], None, None, c["alpha"], c["beta"], c["max_iter"] if max_iter is None else max_iter, -1.0, 1, 0,
            False, c["inner"], 1e-9, c["method"], c["trace"])


def reversed_case(c):
    """The same problem with rows and columns reversed (A, W0, H0): another summation order for every sum the solver forms."""
    return dict(c, A=np.ascontiguousarray(c["A"][::-1, ::-1]), W0=np.ascontiguousarray(c["W0"][::-1, :]),
                H0=np.ascontiguousarray(c["H0"][:, ::-1]))


def relF(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


_ORACLE = {}


def oracle_runs(c, key=None):
    """(oracle run, oracle run of the reversed case with the reversal undone); cached under `key` for the tests that share it."""
    from oracle import ref
    if key is not None and key in _ORACLE:
        return _ORACLE[key]
    o = ref.c_nnmf(*nnmf_args(c))
    r = ref.c_nnmf(*nnmf_args(reversed_case(c)))
    r = dict(r, W=np.ascontiguousarray(r["W"][::-1, :]), H=np.ascontiguousarray(r["H"][:, ::-1]))
    if key is not None:
        _ORACLE[key] = (o, r)
    return o, r


def well_posed_deviation(c, key=None):
    """The larger relative Frobenius difference of W and H between the oracle's run and its run on the reversed problem: how far the
    reference's own answer depends on the summation order.  inf if either run is not finite."""
    o, r = oracle_runs(c, key)
    if not all(np.isfinite(x[f]).all() for x in (o, r) for f in ("W", "H")):
        return float("inf")
    return max(relF(r["W"], o["W"]), relF(r["H"], o["H"]))


def factor_dies(c):
    """The fuzz's rule (test_gpu_fuzz.degenerate), from the oracle alone: after some iteration a column of W or a row of H is at 1e-8 of the
    median norm or not finite.  The next half-step's Gram diagonal is then 1e-16 and the coordinate's value mu / 1e-16 is rounding dust (DESIGN
    2); the reversed problem can carry the SAME dust, so well_posed_deviation alone does not see it (zero_lines, seed 0, 515 x 131, method 1
    without L1: deviation 1e-12 between the two orders, yet a column of W exactly 0 after iteration 1)."""
    from oracle import ref
    for it in range(1, c["max_iter"] + 1):
        o = ref.c_nnmf(*nnmf_args(c, it))
        W, H = o["W"], o["H"]
        if not (np.isfinite(W).all() and np.isfinite(H).all()):
            return True
        dw, dh = (W * W).sum(axis=0), (H * H).sum(axis=1)
        if dw.min() <= 1e-8 * np.median(dw) or dh.min() <= 1e-8 * np.median(dh):
            return True
    return False


def describe(c):
    A = c["A"]
    return dict(family=c["family"], shape=c["shape"], method=c["method"], pen=c["pen"], zeros=float((A == 0).mean()), na=float(np.isnan(A).mean()))
