"""Every instantiation of the dense KL solvers (nnlm_amd/csrc/k_kl.h) at the ends of its last piece, against the fp64 oracle.

kl_tile_kernel<EPT4, C, METHOD, ONEBUF> (fp32-operand mode, 20 exact piece counts) and kl_reg64_kernel<EPT2, C, METHOD> (strict mode, 11
instantiated counts that take 20 exact ones) decide per wavefront whether their last piece exists, count their own outstanding row
requests and pad the last slot; the rest of the suite runs them at a handful of arbitrary lengths.  The cases of tests/kl_piece_cases.py put
the end of the contraction where those decisions change, and weight the rows there so that one lost element would move every column by
~1e-2 (tests/test_kl_piece_cases_host.py) -- a hundred times the fp32 bar.  A case is ONE half-step of 3 .. 17 columns: the other half-step
would solve up to 40193 columns in the oracle and is never run.

Bars: the KL half-step bars of tests/test_gpu_parity.py (test_half_step_matches_oracle, test_kl_contraction_longer_than_32768) -- 1e-10 strict,
1e-4 fp32-operand -- here for EVERY column as well as for the whole factor.  Each test prints its figures before it asserts."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import relF  # noqa: E402
import kl_piece_cases as kc  # noqa: E402
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib  # noqa: E402
from oracle import ref  # noqa: E402

pytestmark = pytest.mark.gpu

MODE = {"tile": (_lib.PREC_F32, 1e-4), "reg64": (_lib.PREC_F64, 1e-10)}
OWN_INIT_LIMIT = 1 << 19  # nnlm_debug_alloc_limit of test_kl_tile_kernel_forms_its_own_starting_states_when_what_does_not_fit


def run_case(c, alloc_limit=0):
    """The case's half-step on the GPU: (X 3 x ncols, sweeps, (kl_form, kl_pieces, kl_cols) of the side that ran)."""
    d = kc.make_data(c)
    h_side = c["orient"] == "H"
    with nnlm_amd.Handle(0, MODE[c["kind"]][0]) as h:
        if h_side:
            h.set_matrix(d["Ac"])
            h.set_factors(kc.K, np.ascontiguousarray(d["Y"].T), d["X0"], None, d["mask"])
        else:
            h.set_matrix(np.ascontiguousarray(d["Ac"].T))
            h.set_factors(kc.K, np.ascontiguousarray(d["X0"].T), d["Y"], None if d["mask"] is None else np.ascontiguousarray(d["mask"].T), None)
        _lib.debug_alloc_limit(alloc_limit)
        try:
            h.half_step(1 if h_side else 0, kc.REG, kc.INNER, kc.TOL, c["method"])
        finally:
            _lib.debug_alloc_limit(0)
        W, H = h.get_factors()
        sweeps = h.take_sweeps()
        s = "h" if h_side else "w"
        ran = tuple(int(h.get_info(key + s)) for key in ("kl_form_", "kl_pieces_", "kl_cols_"))
        other = int(h.get_info("kl_form_" + ("w" if h_side else "h")))
    assert other == -1  # (the other half-step never ran)
    return (H if h_side else np.ascontiguousarray(W.T)), sweeps, ran


def check(c, X, sweeps, ran, form):
    d = kc.make_data(c)
    Xr, it = kc.oracle(ref, c["id"])
    bar = MODE[c["kind"]][1]
    errs, whole = kc.col_err(X, Xr), relF(X, Xr)
    print("KLP %s kernel=%d pieces=%d cols=%d form=%d maxcol=%.3e relF=%.3e sweeps=%d/%d" % ((c["id"],) + tuple(c["plan"]) + (ran[0], errs.max(), whole, sweeps, it)))
    assert ran == (form, c["plan"][1], c["plan"][2]), (c["id"], ran)  # the instantiation under test is the one that executed
    assert np.all(np.isfinite(X)) and np.all(X >= 0)
    assert errs.max() < bar and whole < bar, (c["id"], errs, whole)
    if d["mask"] is not None:
        assert np.array_equal(X[d["mask"]], d["X0"][d["mask"]])  # masked coordinates exactly as given
        full = d["mask"].all(axis=0)
        assert full[1] and np.array_equal(X[:, full], d["X0"][:, full])  # 0 sweeps, values copied through
    if c["kind"] == "reg64":
        assert sweeps == it, (c["id"], sweeps, it)
    return errs.max()


def plain_form(c):
    return {kc.TILE2: 0, kc.TILE1: 0, kc.REG64: 2, kc.STREAM: 3}[c["plan"][0]]


@pytest.mark.parametrize("cid", [c["id"] for c in kc.H_CASES])
def test_h_half_step_at_a_piece_edge_matches_the_oracle_in_every_column(cid):
    """H orientation (A is p x ncols, the contraction runs over rows; the leading dimension is a whole number of wavefront pieces): p_lo /
    p_mid / p_hi of every exact piece count of both kernels, and the first length past each switch point on kl_stream_kernel."""
    c = kc.BY_ID[cid]
    X, sweeps, ran = run_case(c)
    check(c, X, sweeps, ran, plain_form(c))


@pytest.mark.parametrize("cid", [c["id"] for c in kc.W_CASES])
def test_w_half_step_at_a_piece_edge_matches_the_oracle_in_every_column(cid):
    """W orientation (A is ncols x p, the contraction runs over columns through the transposed copy and What^T).  Tile kernel: the row ends
    in the lower half of a wavefront piece whose upper 32 lanes lie beyond the 128-element leading dimension -- zero-filled, never loaded
    (L4 < P4, reachable in this orientation only) -- and just past that half; strict kernel: one length per instantiated piece count."""
    c = kc.BY_ID[cid]
    X, sweeps, ran = run_case(c)
    check(c, X, sweeps, ran, plain_form(c))


@pytest.mark.parametrize("cid", [c["id"] for c in kc.OWN_INIT_CASES])
def test_two_buffer_tile_kernel_on_its_own_starting_states_at_4_to_10_pieces(cid):
    """The matrix-sized starting-state buffer "does not fit" (nnlm_debug_alloc_limit): kl_tile_kernel forms y = sum_q x[q] * row q itself
    ("kl_form_h" = 1), elsewhere tested at 1 .. 3 pieces only.  Same oracle bar, and the roomy run's factor to 5e-6."""
    c = kc.BY_ID[cid]
    X1, s1, ran1 = run_case(c)
    X2, s2, ran2 = run_case(c, OWN_INIT_LIMIT)
    assert ran1[0] == 0
    check(c, X2, s2, ran2, 1)
    both = relF(X2, X1)
    print("KLP %s own-init against roomy relF=%.3e" % (c["id"], both))
    assert both < 5e-6 and s1 == s2, (c["id"], both, s1, s2)
