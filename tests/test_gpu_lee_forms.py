"""The two- and one-lane forms of the Lee sweep, sweep_ls_kernel<R, 2, 2> and <R, 1, 2> (nnlm_amd/csrc/k_sweep.h): launch_sweep() takes
them beyond 65 536 and 131 072 columns, so every test here solves that many columns -- the W half-step of an n x 24 matrix (25 MB at
most; cases and the restated dispatch rule: tests/lee_cases.py, their conditions: tests/test_lee_cases_host.py).

Every test asks the handle which instantiation ran ("lee_lanes_*" / "lee_regs_*" of nnlm_get_info) before it looks at a number.  Bars:
those of test_gpu_parity.PRECS, 1e-10 relative Frobenius in strict fp64 mode and 2e-5 in fp32-operand mode; 1e-11 where two launches
differ only in the order of a few fp64 additions.  Each test prints its deviation (`pytest -s`); the largest per form and mode are in
DESIGN.md section 4.5.

The oracle's result of a case is computed once and shared by both modes (the mode varies fastest).  A is drawn from the case's own
generator, default_rng(n + k), so it is uploaded per test; a half-step and its upload take well under a second."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lee_cases as lc  # noqa: E402
from helpers import relF  # noqa: E402
from sparse_cases import csc_from_pattern  # noqa: E402
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib  # noqa: E402
from oracle import ref  # noqa: E402

pytestmark = pytest.mark.gpu

PRECS = [("f64", _lib.PREC_F64, 1e-10), ("f32", _lib.PREC_F32, 2e-5)]
ORDER = {"f64": 1e-11, "f32": 2e-5}  # two launches of the same arithmetic that differ in the order of summation


@pytest.fixture(autouse=True)
def _default_precision(monkeypatch):
    monkeypatch.delenv("NNLM_PRECISION", raising=False)


@functools.lru_cache(maxsize=2)
def case(n, k):
    return lc.make_case(n, k)


@functools.lru_cache(maxsize=2)
def oracle(n, k, inner=5, tol=1e-9, plain=False):
    return lc.oracle_w(ref, case(n, k), inner, tol, mask=not plain, reg=[0, 0, 0] if plain else lc.REG)


def form(h, side):
    return int(h.get_info("lee_lanes_" + side)), int(h.get_info("lee_regs_" + side))


def gpu_w(prec, c, inner, tol, mask=True, reg=lc.REG, csc=None):
    """One W half-step of the case by Lee's updates: (W, sweeps, (L, R) the handle reports)."""
    with nnlm_amd.Handle(0, prec) as h:
        if csc is None:
            h.set_matrix(c["A"])
        else:
            h.set_matrix_csc(*csc)
        h.set_factors(c["k"], c["W0"], c["H0"], c["Wm"] if mask else None, None)
        assert form(h, "w") == (-1, -1) and form(h, "h") == (-1, -1)  # no Lee sweep yet
        h.half_step(0, reg, inner, tol, 2)
        W, _ = h.get_factors()
        return W, h.take_sweeps(), form(h, "w")


def check_factor(W, W_ref, c, bar, what, mask=True):
    d = relF(W, W_ref)
    print(f"LEEDEV {what}: relF {d:.3e} (bar {bar:g})")
    assert np.isfinite(W).all() and (W >= 0).all()
    if mask:
        assert np.array_equal(W[c["Wm"]], c["W0"][c["Wm"]])  # masked entries: the input, bit for bit
    assert d < bar
    return d


# ---- a. every instantiation against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", PRECS)
@pytest.mark.parametrize("n,k", lc.PARITY_CASES)
def test_every_form_matches_the_oracle(n, k, pname, prec, tol):
    """65 537 (L = 2) and 131 110 (L = 1) columns at both ends of every R; the last / first counts of each form and the L = 4 control
    at three ranks.  5 sweeps at tolerance 1e-9: no column stops early, the strict count is 5 per column that is not fully masked."""
    c = case(n, k)
    W_ref, it = oracle(n, k)
    W, sweeps, got = gpu_w(prec, c, 5, 1e-9)
    assert got == lc.form_of(n, k)
    check_factor(W, W_ref, c, tol, f"parity L={got[0]} R={got[1]} n={n} k={k} {pname}")
    if pname == "f64":
        assert sweeps == it == 5 * lc.live_columns(c)


# ---- b. columns that finish early -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", PRECS)
@pytest.mark.parametrize("n,k", lc.EARLY_CASES)
def test_early_finishers(n, k, pname, prec, tol):
    """A tolerance at which the oracle stops some columns after a few sweeps and runs others to the budget (lee_cases.early_setting;
    test_lee_cases_host.py asserts that it exists): finished columns share wavefronts with running ones."""
    inner, itol, W_ref, it = lc.early_setting(ref, n, k)
    c = case(n, k)
    W, sweeps, got = gpu_w(prec, c, inner, itol)
    assert got == lc.form_of(n, k) and got[1] > 16
    check_factor(W, W_ref, c, tol, f"early L={got[0]} R={got[1]} n={n} k={k} inner={inner} tol={itol:g} {pname}")
    print(f"LEEDEV early sweeps {sweeps} oracle {it} of {inner * lc.live_columns(c)}")
    if pname == "f64":
        assert abs(sweeps - it) <= 2 + lc.early_order_slack(ref, n, k)


# ---- c. the other orientation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", PRECS)
@pytest.mark.parametrize("n,k", lc.H_CASES)
def test_h_half_step_of_the_transposed_problem(n, k, pname, prec, tol):
    """The same update() as an H half-step: A^T is 24 x n, the solved factor is H = W0^T with the mask on H."""
    c = case(n, k)
    W_ref, it = oracle(n, k)
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix(np.ascontiguousarray(c["A"].T))
        h.set_factors(k, np.ascontiguousarray(c["H0"].T), np.ascontiguousarray(c["W0"].T), None, np.ascontiguousarray(c["Wm"].T))
        h.half_step(1, lc.REG, 5, 1e-9, 2)
        _, H = h.get_factors()
        sweeps, got, other = h.take_sweeps(), form(h, "h"), form(h, "w")
    assert got == lc.form_of(n, k) and got[1] > 16 and other == (-1, -1)
    check_factor(H.T, W_ref, c, tol, f"transposed L={got[0]} R={got[1]} n={n} k={k} {pname}")
    if pname == "f64":
        assert sweeps == it


# ---- d. no penalties, no mask ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", PRECS)
@pytest.mark.parametrize("n,k", lc.PLAIN_CASES)
def test_no_penalties_and_no_mask(n, k, pname, prec, tol):
    """a.mask == NULL and r2 == 0: every column is live, the L1 term drops out of the quotient."""
    c = case(n, k)
    W_ref, it = oracle(n, k, plain=True)
    W, sweeps, got = gpu_w(prec, c, 5, 1e-9, mask=False, reg=[0, 0, 0])
    assert got == lc.form_of(n, k)
    check_factor(W, W_ref, c, tol, f"plain L={got[0]} R={got[1]} n={n} k={k} {pname}", mask=False)
    if pname == "f64":
        assert sweeps == it == 5 * n


# ---- e. form against form, without the oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", PRECS)
@pytest.mark.parametrize("n,k", lc.PAIR_CASES)
def test_two_forms_agree_on_the_rows_they_share(n, k, pname, prec, tol):
    """The W half-step of the n-row case and of its first n - 1 rows as a matrix of their own: same fixed factor, same Gram, the next
    wider form (65 537: L = 2 against 4; 131 073: L = 1 against 2).  The shared rows differ only in how the lanes of a column add up a
    dot product."""
    c = case(n, k)
    head = lc.head_of(c, n - 1)
    W, s1, got = gpu_w(prec, c, 5, 1e-9)
    Wh, s2, got_head = gpu_w(prec, head, 5, 1e-9)
    assert got == lc.form_of(n, k) and got_head == lc.form_of(n - 1, k) and got_head[0] == 2 * got[0]
    d = relF(W[:n - 1], Wh)
    print(f"LEEDEV pair L={got[0]} vs L={got_head[0]} n={n} k={k} {pname}: relF {d:.3e} (bar {ORDER[pname]:g})")
    assert d < ORDER[pname]
    assert np.array_equal(Wh[head["Wm"]], head["W0"][head["Wm"]]) and np.array_equal(W[c["Wm"]], c["W0"][c["Wm"]])
    if pname == "f64":
        assert s1 == s2 + 5 * (lc.live_columns(c) - lc.live_columns(head))


# ---- f. three forms in one factor -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", PRECS)
@pytest.mark.parametrize("k", [13, 50])
def test_three_virtual_ranks_take_three_forms(pname, prec, tol, k):
    """The recipe of test_virtual_ranks_run_column_sharded_half_steps (test_gpu_parity.py) at 131 110 rows: launch_sweep() sees the END
    column of each rank's slab -- 43 776, 87 552, 131 110 -- so the ranks solve their thirds of W with L = 4, 2 and 1, and the one-rank
    run they are compared with solves all of it with L = 1."""
    n, world = 131110, 3
    c = lc.make_case(n, k)
    A, W0, H0, Wm = c["A"], c["W0"], c["H0"], c["Wm"]
    with nnlm_amd.Handle(0, prec) as h1:
        h1.set_matrix(A)
        h1.set_factors(k, W0, H0, Wm, None)
        h1.iterate(2, lc.REG, lc.REG, 5, 1e-9, 2)
        W_ref, H_ref = h1.get_factors()
        sw_ref = h1.take_sweeps()
        assert form(h1, "w") == lc.form_of(n, k) and form(h1, "h") == lc.form_of(lc.M, k)
    hs = [nnlm_amd.Handle(0, prec) for _ in range(world)]
    try:
        for rk, h in enumerate(hs):
            h.comm_init(None, rk, world)
            h.set_matrix(A)
            h.set_factors(k, W0, H0, Wm, None)
        for _ in range(2):
            for which in (0, 1):
                for phase in (1, 2):
                    for h in hs:
                        h.debug_phase(which, phase, lc.REG, 5, 1e-9, 2)
                _lib.debug_exchange(hs, which, 2)
                for h in hs:
                    h.debug_phase(which, 3, lc.REG, 5, 1e-9, 2)
        forms = [form(h, "w") for h in hs]
        res = [h.get_factors() for h in hs]
        sweeps = sum(h.take_sweeps() for h in hs)
    finally:
        for h in hs:
            h.close()
    ends = [_lib.shard_cols(n, rk, world)[2] for rk in range(world)]
    assert forms == [lc.form_of(e, k) for e in ends] and [f[0] for f in forms] == [4, 2, 1], (forms, ends)
    for W, H in res[1:]:
        assert np.array_equal(W, res[0][0]) and np.array_equal(H, res[0][1])
    dw, dh = relF(res[0][0], W_ref), relF(res[0][1], H_ref)
    print(f"LEEDEV ranks L=4,2,1 vs L=1 k={k} {pname}: relF W {dw:.3e} H {dh:.3e} (bar {ORDER[pname]:g})")
    assert dw < ORDER[pname] and dh < ORDER[pname]
    assert np.array_equal(res[0][0][Wm], W0[Wm])
    assert abs(sweeps - sw_ref) <= (0 if pname == "f64" else 2)


# ---- g. the other doors to the same launch --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", PRECS)
def test_sparse_matrix_reaches_the_one_lane_form(pname, prec, tol):
    """nnlm_set_matrix_csc of a 131 110 x 24 matrix with 30 % stored entries: the cross product comes from the SpMM kernels, the sweep
    is the same launch.  Rows without a stored entry go to exact zero on both sides."""
    c, P = lc.sparse_case()
    W_ref, it = lc.oracle_w(ref, c, 5, 1e-9)
    W, sweeps, got = gpu_w(prec, c, 5, 1e-9, csc=csc_from_pattern(P, c["A"]))
    assert got == lc.form_of(c["n"], c["k"]) == (1, 24)
    check_factor(W, W_ref, c, tol, f"csc L={got[0]} R={got[1]} n={c['n']} k={c['k']} {pname}")
    if pname == "f64":
        assert sweeps == it


@pytest.mark.parametrize("pname,prec,tol", PRECS)
def test_nnlm_with_131110_responses(monkeypatch, pname, prec, tol):
    """c_nnlm(x 30 x 20, y 30 x 131 110, method 2) against the oracle's c_nnlm.  The one-shot entry owns its handle, so the form is
    read from the same solve on a resident handle (W = x fixed, H = the coefficients), which must give the one-shot entry's answer."""
    c = lc.nnlm_case()
    x, y, b0, mask = c["x"], c["y"], c["b0"], c["mask"]
    p, q = b0.shape
    o = ref.c_nnlm(x, y, lc.REG, mask, b0, 5, 1e-9, 1, 2)
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix(y)
        h.set_factors(p, x, b0, None, mask)
        h.half_step(1, lc.REG, 5, 1e-9, 2)
        _, B = h.get_factors()
        assert form(h, "h") == lc.form_of(q, p) == (1, 24)
    monkeypatch.setenv("NNLM_PRECISION", pname)
    r = nnlm_amd.c_nnlm(x, y, lc.REG, mask, b0, 5, 1e-9, 1, 2)
    d, dres = relF(r["coefficient"], o["coefficient"]), relF(r["coefficient"], B)
    print(f"LEEDEV nnlm L=1 R=24 q={q} p={p} {pname}: relF {d:.3e} (bar {tol:g}), one-shot vs resident {dres:.3e}")
    assert d < tol and dres < ORDER[pname]
    assert np.isfinite(r["coefficient"]).all() and (r["coefficient"] >= 0).all()
    assert np.array_equal(r["coefficient"][mask], b0[mask])
    if pname == "f64":
        assert r["n_iteration"] == o["n_iteration"]
