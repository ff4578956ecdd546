"""Case builders for KL loss on a sparse A (nnlm_set_matrix_csc_kl, k_sparse_kl.h): tests/test_gpu_sparse_kl.py runs them on the GPU,
tests/test_sparse_kl_host.py shows each of them well posed from the oracle alone.  numpy only, deterministic.

Data is Poisson counts of a planted non-negative model W H; zeros are dropped from the structure, so every stored value is a positive
integer and the KL problem is well posed.  Where a test needs a PATTERN of its own (exact stored counts per line, the families of
sparse_cases.py) the stored values are 1 + Poisson, which keeps the pattern as designed.  The start is near the planted factors
(structureless starts let factors die on the way, see sparse_cases.py).

The module restates the dispatch rule of k_sparse_kl.h: a line of at most SHORT_MAX stored entries is solved by the short form (a
wavefront per line), a longer one by the long form (a workgroup per line); the GPU file pins the restatement to nnlm_get_info."""
import numpy as np

import sparse_cases as sc

SHORT_MAX = 256            # SPKL_SHORT_MAX (k_sparse_kl.h): 64 lanes x 4 stored entries per lane
FORM_SHORT, FORM_LONG = 1, 2  # bits of nnlm_get_info "sparse_kl_form_h" / "sparse_kl_form_w"
THRESHOLD_COUNTS = (0, 1, 63, 64, 65, SHORT_MAX - 1, SHORT_MAX, SHORT_MAX + 1)
REGS = {"none": [0, 0, 0], "l2": [0.05, 0, 0], "angle": [0, 0.02, 0], "l1": [0, 0, 0.03], "all": [0.02, 0.01, 0.03]}


def form_of(length):
    """The solver form of a line with `length` stored entries."""
    return FORM_SHORT if length <= SHORT_MAX else FORM_LONG


def forms_of(indptr):
    """The bit mask a half-step over the lines of `indptr` reports: every form that at least one line takes."""
    out = 0
    for length in np.diff(np.asarray(indptr, dtype=np.int64)):
        out |= form_of(int(length))
    return out


def line_forms(S):
    """(forms of the W half-step -- rows, the CSR --, forms of the H half-step -- columns, the CSC)."""
    return forms_of(sc.transpose_csc(S)[0]), forms_of(S[0])


def _planted(n, m, k, rng, mean):
    """Planted factors whose product has mean `mean`, and a start near them."""
    Wp, Hp = rng.random((n, k)) ** 2 + 0.05, rng.random((k, m)) ** 2 + 0.05
    sc_ = np.sqrt(mean / float(np.mean(Wp @ Hp)))
    Wp, Hp = Wp * sc_, Hp * sc_
    return Wp, Hp, Wp * (0.7 + 0.6 * rng.random((n, k))), Hp * (0.7 + 0.6 * rng.random((k, m)))


def _case(S, k, W0, H0, name, **extra):
    c = dict(S=S, k=k, W0=W0, H0=H0, name=name, Wm=None, Hm=None, alpha=[0, 0, 0], beta=[0, 0, 0], inner=1)
    c.update(extra)
    return c


def count_case(n, m, k, density, seed, mean=4.0):
    """Poisson counts of a planted model on a random pattern of the given density; the zeros among them leave the structure."""
    rng = np.random.default_rng(770000 + seed)
    Wp, Hp, W0, H0 = _planted(n, m, k, rng, mean)
    C = rng.poisson(Wp @ Hp) * (rng.random((n, m)) < density)
    W0, H0 = W0 * np.sqrt(density), H0 * np.sqrt(density)  # (the absent entries are zeros: the fit's level is density x the model's)
    return _case(sc.csc_from_pattern(C > 0, C.astype(np.float64)), k, W0, H0, "counts %dx%d k%d d%g" % (n, m, k, density))


def pattern_case(P, k, seed, name):
    """1 + Poisson counts of a planted model at the entries of the boolean pattern P."""
    n, m = P.shape
    rng = np.random.default_rng(780000 + seed)
    Wp, Hp, W0, H0 = _planted(n, m, k, rng, 3.0)
    V = 1.0 + rng.poisson(Wp @ Hp)
    lvl = np.sqrt(max(float(P.mean()), 1e-3))  # (the absent entries are zeros: the fit's level is the pattern's density x the model's)
    return _case(sc.csc_from_pattern(P, V), k, W0 * lvl, H0 * lvl, name)


def lines_case(counts, k, transposed, seed=0):
    """Column j holds exactly counts[j] stored entries (rows by the rule of sparse_cases._columns_case); transposed: the designed lines
    are rows, which the W half-step reads from the CSR."""
    n, m = max(max(counts) + 103, 8), len(counts)
    P = np.zeros((n, m), dtype=bool)
    for j, cnt in enumerate(counts):
        if cnt:
            P[(j * 37 + (np.arange(cnt) * n) // cnt) % n, j] = True
    c = pattern_case(P.T.copy() if transposed else P, k, 100 + seed + int(transposed), "lines %s%s" % (list(counts), "^T" if transposed else ""))
    c["designed_counts"] = tuple(counts)
    c["transposed"] = transposed
    return c


def half_case(n, m, k, transposed, seed=0):
    """One line (column 3; transposed: row 3) holds half of all stored entries."""
    rng = np.random.default_rng(790000 + seed)
    P = np.zeros((n, m), dtype=bool)
    P[:, 3] = True
    fl = rng.choice(n * m, size=n, replace=False)
    P[fl % n, fl // n] = True
    P[:, 3] = True
    return pattern_case(P.T.copy() if transposed else P, k, 200 + seed + int(transposed), "half%s" % ("^T" if transposed else ""))


def family_case(family, seed=0):
    """The pattern families of sparse_cases.py with count data: empty_lines, powerlaw (by columns / by rows), heavy."""
    rng = np.random.default_rng(800000 + seed)
    n, m, k = 310, 290, 7
    if family == "empty_lines":
        P = sc._empty_lines(n, m, rng)
    elif family == "powerlaw":
        P = sc._powerlaw(n, m, rng, by_rows=False)
    elif family == "powerlaw_rows":
        P = sc._powerlaw(n, m, rng, by_rows=True)
    elif family == "heavy":
        P = sc._heavy(n, m, rng)
    else:
        raise ValueError(family)
    c = pattern_case(P, k, 300 + seed, family)
    if family == "empty_lines":
        # (a line without stored entries: SCD clamps it to an exact 0 on both sides; Lee multiplies by tmp = 0 -- exact on both sides too)
        rows, cols = sc.line_counts(c["S"])
        assert (rows == 0).any() and (cols == 0).any()
    return c


BOUNDARY_NAMES = ("short_columns", "segment_counts")


def boundary_family():
    """The `boundary` family of sparse_cases.py (both orientations) with count data on its patterns: the specs whose columns sit at 0, 1, 63,
    64, 65 and at 2047 ... 4097 stored entries."""
    out = []
    for c in sc.boundary_cases("zero"):
        if c["name"].rstrip("^T") not in BOUNDARY_NAMES:
            continue
        d = pattern_case(sc.pattern_of(c["S"]), min(c["k"], 16), 400 + len(out), "boundary " + c["name"])
        d["transposed"] = c["transposed"]
        out.append(d)
    return out


def exact_state_case(seed=0):
    """The `exact_state` situation: dyadic data and factors, and a fixed factor W with a column that is 0 on a third of its
    rows -- a KL state can return to exactly 0 when a coordinate is clamped."""
    rng = np.random.default_rng(810000 + seed)
    n, m, k = 96, 40, 4
    W0 = rng.integers(1, 9, (n, k)) / 8.0
    W0[rng.permutation(n)[: n // 3], 1] = 0.0
    rows = rng.permutation(n)[: n // 3]
    W0[rows, 0] = 0.0
    W0[rows, 2] = 0.0
    W0[rows, 3] = 0.0  # (on these rows only coordinate 1 is live: clamping it empties the state)
    W0[rows, 1] = np.maximum(W0[rows, 1], 0.125)
    H0 = rng.integers(1, 9, (k, m)) / 8.0
    C = rng.poisson(4.0 * W0 @ H0) * (rng.random((n, m)) < 0.5)
    return _case(sc.csc_from_pattern(C > 0, C.astype(np.float64)), k, W0, H0, "exact_state")


def option_cases():
    """Masks on W and H, a known profile, each penalty position alone and together, inner_max_iter 1 and 5 -- on one 150 x 90 matrix."""
    out = []
    for i, (rname, reg) in enumerate(REGS.items()):
        for inner in (1, 5):
            c = count_case(150, 90, 4, 0.1, 32)  # (seed 10: five SCD sweeps leave rounding dust in W1, see test_sparse_kl_host.py)
            c.update(alpha=list(reg), beta=list(reg[::-1]) if rname == "all" else list(reg), inner=inner, name="reg %s inner %d" % (rname, inner))
            out.append(c)
    rng = np.random.default_rng(820000)
    c = count_case(150, 90, 4, 0.1, 17)  # (seeds 11, 12: the oracle's own SCD result moves by 1e-8 / 1e-6 under a 1e-13 perturbation; 13-16: dust in W1)
    Wm, Hm = rng.random((150, 4)) < 0.15, rng.random((4, 90)) < 0.15
    Wm[7, :] = True   # a fully masked line: passed by, no sweep counted
    Hm[:, 5] = True
    c["W0"][Wm], c["H0"][Hm] = 0.0, 0.0
    c.update(Wm=Wm.astype(np.int32), Hm=Hm.astype(np.int32), inner=5, name="masks")
    out.append(c)
    c = count_case(150, 90, 4, 0.1, 12)  # a known profile: column 0 of W given and masked (what reformat_input makes of init$W0)
    Wm = np.zeros((150, 4), dtype=np.int32)
    Wm[:, 0] = 1
    c.update(Wm=Wm, Hm=None, inner=5, name="known profile")
    out.append(c)
    return out


def perturbed(c, rng, size=1e-13):
    """Case c with its start moved by `size` relative noise: what the oracle makes of it measures how well posed the case is."""
    return dict(c, W0=c["W0"] * (1 + size * rng.standard_normal(c["W0"].shape)), H0=c["H0"] * (1 + size * rng.standard_normal(c["H0"].shape)))


def dense_of(c):
    return sc.densify(c["S"], "zero")


def half_step_refs(c, ref, method, rel_tol=1e-9):
    """The oracle's two half-steps of case c on the densified matrix: (W1, sweeps of the W half-step, H1 with W1 fixed, its sweeps)."""
    A = dense_of(c)
    Wm = None if c["Wm"] is None else np.ascontiguousarray(np.asarray(c["Wm"]).T)
    Wt, it1 = ref.update(c["W0"].T.copy(), c["H0"], A.T.copy(), Wm, c["alpha"], c["inner"], rel_tol, method, missing=False)
    H1, it2 = ref.update(c["H0"].copy(), Wt, A, c["Hm"], c["beta"], c["inner"], rel_tol, method, missing=False)
    return Wt.T.copy(), it1, H1, it2


def all_half_step_cases():
    """Every case the GPU file runs single half-steps on, by name."""
    cases = [count_case(150, 90, 4, 0.1, 1)]
    cases += [count_case(300, 200, k, 0.1, 20 + k) for k in (1, 16, 17, 50, 64)]
    cases += [lines_case(THRESHOLD_COUNTS, 5, tr) for tr in (False, True)]
    cases += [half_case(700, 60, 6, tr) for tr in (False, True)]
    cases += [family_case(f) for f in ("empty_lines", "powerlaw", "powerlaw_rows", "heavy")]
    cases += boundary_family()
    cases += option_cases()
    return cases
