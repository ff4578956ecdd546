"""Whole-driver parity on what A CONTAINS (tests/data_cases.py): count data with up to 60 % exact zeros, zero rows and columns, wholly
missing rows and columns, six decades inside one column, the same column at several positions, and a state vector that returns to
exactly zero.  nnlm_amd.c_nnmf against ref.c_nnmf with NO skip rule: tests/test_data_cases_host.py has shown every case well posed for
the oracle itself (two summation orders agree to 1e-11).

Strict mode: the bounds of test_gpu_fuzz.test_random_driver_runs_strict_mode (factors at 1e-9 relative Frobenius, iteration counts and
trace lengths equal, traces at rtol 1e-8); sweep counts exact where the oracle's own two summation orders count alike, within the fuzz's
(2 inner) / (n + m) elsewhere.  F32 mode: the mode's contract, 1e-4 on W and H, traces at rtol 1e-3.  Each test prints what it measured
before it asserts (pytest -s, or tests/fuzz_table.py --families for one line per case)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import data_cases as dc  # noqa: E402
from helpers import relF  # noqa: E402
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib  # noqa: E402
from oracle import ref  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = [("f64", _lib.PREC_F64, 1e-9), ("f32", _lib.PREC_F32, 1e-4)]


def check_lines_of_zeros(c, r, o, tol, tag):
    """Rows / columns of zeros in A (zero_lines): the factor lines the oracle has, at the tolerance of the whole factor; where the oracle's
    line is exactly zero by construction (an L1 term clamps it, Lee's update multiplies by an empty numerator) it is exactly zero here."""
    A = c["A"]
    with np.errstate(invalid="ignore"):
        zr, zc = np.flatnonzero((A == 0).all(axis=1)), np.flatnonzero((A == 0).all(axis=0))
    for name, ours, theirs in (("W", r["W"][zr, :], o["W"][zr, :]), ("H", r["H"][:, zc], o["H"][:, zc])):
        if theirs.size == 0:
            continue
        dev = float(np.abs(ours - theirs).max()) / float(np.abs(o[name]).max())
        print(f"  {tag} zero lines of {name}: max dev {dev:.2e} oracle max {np.abs(theirs).max():.2e}")
        assert dev < tol, (name, dev)
        if (c["pen"] == 1 or c["method"] in (2, 4)) and (theirs == 0).all():
            assert (ours == 0).all(), name


@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("case", dc.cases(), ids=dc.case_id)
def test_family_runs_match_the_oracle(monkeypatch, pname, prec, tol, case):
    """Measured on the MI355X, worst relF over W and H (strict / F32): counts 3.1e-14 / 1.3e-6, zero_lines 8.5e-14 / 7.4e-6, na_lines
    8.4e-14 / 7.6e-6, heavy 3.7e-13 / 7.4e-5.
    (A case in which a factor dies on the oracle's way -- zero_lines seed 0 at 515 x 131, SCD-MSE without L1 -- is not reproducible beyond
    2.5e-2 / 1.8e-1 in either mode although the oracle's two orders agree on it; the host file excludes such seeds by data_cases.factor_dies.)"""
    monkeypatch.setenv("NNLM_PRECISION", pname)
    c = dc.make_case(*case)
    o, orev = dc.oracle_runs(c, key=case)
    r = nnlm_amd.c_nnmf(*dc.nnmf_args(c))
    d = dc.describe(c)
    n, m, _ = c["shape"]
    ew, eh = relF(r["W"], o["W"]), relF(r["H"], o["H"])
    print(f"\n  {pname} {dc.case_id(case)} W {ew:.2e} H {eh:.2e} nit {r['n_iteration']}/{o['n_iteration']} "
          f"epoch dev {np.abs(r['average_epoch'] - o['average_epoch']).max() if r['average_epoch'].shape == o['average_epoch'].shape else 'shape'}")
    assert np.isfinite(r["W"]).all() and np.isfinite(r["H"]).all(), d
    assert (r["W"] >= 0).all() and (r["H"] >= 0).all(), d
    assert r["n_iteration"] == o["n_iteration"], d
    for key in ("mse_error", "mkl_error", "target_error", "average_epoch"):
        assert r[key].shape == o[key].shape, (key, d)
    assert ew < tol and eh < tol, (ew, eh, d)
    if pname == "f64":
        if np.array_equal(o["average_epoch"], orev["average_epoch"]):
            assert np.array_equal(r["average_epoch"], o["average_epoch"]), d
        else:  # (the rounding dust of a line of zeros: whether its last 1e-17 counts as a change depends on the summation order)
            assert np.allclose(r["average_epoch"], o["average_epoch"], rtol=0, atol=(2.0 * c["inner"] + 1e-9) / (n + m)), d
        assert np.allclose(r["mse_error"], o["mse_error"], rtol=1e-8, atol=1e-13), d
        assert np.allclose(r["mkl_error"], o["mkl_error"], rtol=1e-8, atol=1e-11), d
        assert np.allclose(r["target_error"], o["target_error"], rtol=1e-8, atol=1e-11), d
    else:
        assert np.allclose(r["mse_error"], o["mse_error"], rtol=1e-3, atol=1e-12), d
        assert np.allclose(r["target_error"], o["target_error"], rtol=1e-3, atol=1e-9), d
    if c["family"] == "zero_lines":
        check_lines_of_zeros(c, r, o, tol, pname)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("with_na", [False, True])
@pytest.mark.parametrize("method", dc.METHODS)
@pytest.mark.parametrize("shape", dc.SHAPES)
def test_a_column_gives_the_same_result_wherever_it_sits(monkeypatch, pname, prec, tol, shape, method, with_na):
    """Copies of column 0 at a wavefront edge (15, 16), a 128-column tile edge (127, 128) and the last column, copies of row 0 at 255,
    256 and the last row: one W and one H half-step, then the 4-iteration run.  The arithmetic of a column does not depend on where
    the column sits, so every copy is BIT-IDENTICAL to its original, in both modes."""
    monkeypatch.setenv("NNLM_PRECISION", pname)
    c = dc.make_dup_case(shape, method, with_na)
    rows, cols = c["rows"], c["cols"]
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix(c["A"])
        h.set_factors(c["k"], c["W0"], c["H0"])
        h.half_step(0, c["alpha"], c["inner"], 1e-9, method)
        W1, _ = h.get_factors()
        h.half_step(1, c["beta"], c["inner"], 1e-9, method)
        _, H1 = h.get_factors()
    r = nnlm_amd.c_nnmf(*dc.nnmf_args(c))
    o = ref.c_nnmf(*dc.nnmf_args(c))
    ew, eh = relF(r["W"], o["W"]), relF(r["H"], o["H"])
    dw = max(float(np.abs(W[i, :] - W[0, :]).max()) for W in (W1, r["W"]) for i in rows)
    dh = max(float(np.abs(H[:, j] - H[:, 0]).max()) for H in (H1, r["H"]) for j in cols)
    print(f"\n  {pname} dup {shape} method {method} na {with_na}: W {ew:.2e} H {eh:.2e}; copies differ by W {dw:.2e} H {dh:.2e}")
    assert np.isfinite(W1).all() and np.isfinite(H1).all() and np.isfinite(r["W"]).all() and np.isfinite(r["H"]).all()
    for W in (W1, r["W"]):
        for i in rows:
            assert _same(W[i, :], W[0, :]), (i, np.abs(W[i, :] - W[0, :]).max())
    for H in (H1, r["H"]):
        for j in cols:
            assert _same(H[:, j], H[:, 0]), (j, np.abs(H[:, j] - H[:, 0]).max())
    assert ew < tol and eh < tol, (ew, eh)


def _exact_state_checks(tag, H, H_ref, tol, W=None, W_ref=None):
    eh = relF(H, H_ref)
    ew = relF(W, W_ref) if W is not None else 0.0
    lost = int(((H == 0) & (H_ref > 0)).sum()) + (int(((W == 0) & (W_ref > 0)).sum()) if W is not None else 0)
    print(f"  {tag}: H {eh:.2e} W {ew:.2e} coordinates at 0 where the oracle's are positive: {lost}")
    assert np.isfinite(H).all() and (H >= 0).all()
    assert lost == 0, tag
    assert eh < tol and ew < tol, (tag, eh, ew)


@pytest.mark.parametrize("pname,prec,tol", [("f64", _lib.PREC_F64, 1e-10), ("f32", _lib.PREC_F32, 1e-4)])  # (the KL bars of test_half_step_matches_oracle)
@pytest.mark.parametrize("method", [3, 4])
def test_a_state_that_returns_to_exactly_zero(pname, prec, tol, method):
    """exact_state (data_cases.make_exact_state_case): the first coordinate step clamps coordinate 0 of every column to 0 and the state of
    a third of the rows is then EXACTLY 0.  The reference's quotient there is w / (0 + 1e-16) = 0 for the rows' w = 0; a reciprocal
    of the bare state gives 0 * inf = NaN, which the clamp `!(tmp > 0)` turns into a silent zero of a live coordinate.  One H half-step and the
    3-iteration run against the oracle; no coordinate may be 0 where the oracle's is positive."""
    c = dc.make_exact_state_case(method)
    H_ref, _ = ref.update(c["H0"], c["W0"].T.copy(), c["A"], None, c["beta"], c["inner"], 1e-9, method)
    o = ref.c_nnmf(*dc.nnmf_args(c))
    print()
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix(c["A"])
        h.set_factors(c["k"], c["W0"], c["H0"])
        h.half_step(1, c["beta"], c["inner"], 1e-9, method)
        _, H1 = h.get_factors()
        form = h.get_info("kl_form_h")
        h.set_factors(c["k"], c["W0"], c["H0"])
        h.iterate(c["max_iter"], c["alpha"], c["beta"], c["inner"], 1e-9, method)
        W3, H3 = h.get_factors()
    assert form == (2 if pname == "f64" else 0), form  # (kl_reg64_kernel / kl_tile_kernel on the GEMM's starting states)
    _exact_state_checks(f"{pname} method {method} half-step", H1, H_ref, tol)
    _exact_state_checks(f"{pname} method {method} run", H3, o["H"], tol, W3, o["W"])


@pytest.mark.parametrize("method", [3, 4])
def test_a_state_that_returns_to_exactly_zero_in_the_own_init_form_of_the_tile_kernel(method):
    """The same through kl_tile_kernel with Yinit = NULL (it forms its starting states itself when the matrix-sized buffer does not fit):
    the dance of test_gpu_edges.test_kl_tile_kernel_forms_its_own_starting_states_when_what_does_not_fit."""
    c = dc.make_exact_state_case(method)
    k, W0, H0 = c["k"], c["W0"], c["H0"]
    H_ref, _ = ref.update(H0, W0.T.copy(), c["A"], None, c["beta"], c["inner"], 1e-9, method)
    o = ref.c_nnmf(*dc.nnmf_args(c))
    print()
    with nnlm_amd.Handle(0, _lib.PREC_F32) as h:
        h.set_matrix(c["A"])
        h.set_factors(k + 1, np.hstack([W0, W0[:, :1]]), np.vstack([H0, H0[:1]]))
        h.iterate(1, c["alpha"], c["beta"], c["inner"], 1e-9, method)  # (leaves the transposed copy of A behind; set_factors drops the state buffer)
        h.set_factors(k, W0, H0)
        _lib.debug_alloc_limit(1 << 13)
        try:
            h.half_step(1, c["beta"], c["inner"], 1e-9, method)
            _, H1 = h.get_factors()
            h.set_factors(k, W0, H0)
            h.iterate(c["max_iter"], c["alpha"], c["beta"], c["inner"], 1e-9, method)
        finally:
            _lib.debug_alloc_limit(0)
        W3, H3 = h.get_factors()
        forms = (h.get_info("kl_form_w"), h.get_info("kl_form_h"))
    assert forms == (1, 1), forms
    _exact_state_checks(f"own-init method {method} half-step", H1, H_ref, 1e-4)
    _exact_state_checks(f"own-init method {method} run", H3, o["H"], 1e-4, W3, o["W"])
