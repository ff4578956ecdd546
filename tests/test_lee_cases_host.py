"""Conditions on the cases of tests/lee_cases.py, from the restated dispatch rule and the fp64 oracle alone (no GPU): the cases reach
every two- and one-lane instantiation of sweep_ls_kernel, are well posed (the oracle agrees with itself under another order of summation
and under fp32 rounding of A far inside the bars the GPU tests hold the kernels to), and the early-finisher cases do stop early."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lee_cases as lc  # noqa: E402
from helpers import relF  # noqa: E402
from oracle import ref  # noqa: E402


def test_dispatch_rule_thresholds_and_register_counts():
    assert [lc.lanes_of(n) for n in lc.NS] == [4, 2, 2, 1, 1]
    assert lc.lanes_of(1) == 4 and lc.lanes_of(2_000_000) == 1
    for L in (4, 2, 1):
        step = 8 // L
        for k in range(1, 65):
            R = lc.regs_of(k, L)
            assert R % step == 0 and R * L >= k > (R - step) * L and step <= R <= 8 * step, (k, L, R)
    assert {lc.regs_of(k, 4) for k in range(1, 65)} == set(range(2, 17, 2))


def test_cases_reach_every_two_and_one_lane_instantiation():
    """{65537, 131072} x KS covers all eight <R, 2>, {131073, 131110} x KS all eight <R, 1>, each R from both ends of its rank range;
    so do the two column counts that the parity test runs at every rank."""
    for ns, L in (((65537, 131072), 2), ((131073, 131110), 1)):
        step = 8 // L
        for n in ns:
            forms = [lc.form_of(n, k) for k in lc.KS]
            assert {f[0] for f in forms} == {L}
            assert sorted({f[1] for f in forms}) == [step * i for i in range(1, 9)]
            for R in {f[1] for f in forms}:
                ks = [k for k in lc.KS if lc.regs_of(k, L) == R]
                assert min(ks) == max(1, (R - step) * L + 1) and max(ks) == R * L, (L, R, ks)
    ran = {lc.form_of(n, k) for n, k in lc.PARITY_CASES}
    assert {(2, 4 * i) for i in range(1, 9)} | {(1, 8 * i) for i in range(1, 9)} <= ran
    assert {lc.form_of(65536, k)[0] for k in lc.KS_FEW} == {4}
    # more than one 16-register chunk per lane: R >= 20 at L = 2, R >= 24 at L = 1; never at L = 4
    assert max(lc.regs_of(k, 4) for k in lc.KS) == 16 and lc.form_of(65537, 33)[1] == 20 and lc.form_of(131110, 17)[1] == 24
    for n, k in lc.EARLY_CASES + lc.H_CASES:
        assert lc.form_of(n, k)[1] > 16
    for n, k in lc.PAIR_CASES:
        assert lc.lanes_of(n - 1) == 2 * lc.lanes_of(n)


def test_masked_rows_sit_on_the_wavefront_edges():
    assert lc.masked_rows(65537) == [3, 65535, 65536]      # 32 columns per wavefront: 2048 full ones, one column in the last
    assert lc.masked_rows(131110) == [3, 131071, 131109]   # 64 per wavefront: 2048 full ones, 38 columns in the last
    assert lc.masked_rows(131072) == [3, 131071] and lc.masked_rows(65536) == [3, 65535]
    c = lc.make_case(65537, 9)
    assert c["Wm"][lc.masked_rows(65537)].all() and 0.03 < c["Wm"].mean() < 0.07
    assert lc.live_columns(c) == 65537 - 3


def test_virtual_rank_split_of_131110_columns_takes_three_forms():
    """nnlm_shard_cols (a host function of the library) gives three ranks the END columns 43776, 87552 and 131110."""
    from nnlm_amd import _lib
    ends = [_lib.shard_cols(131110, rk, 3)[2] for rk in range(3)]
    assert [lc.lanes_of(e) for e in ends] == [4, 2, 1], ends


@pytest.mark.parametrize("n,k", lc.PARITY_CASES)
def test_case_is_well_posed(n, k):
    """The oracle's half-step and the same half-step with the contraction summed in the opposite order agree to 1e-13 with equal sweep
    counts (measured: 5.4e-15 at most), every column runs its five sweeps, and the result is finite and positive off the mask."""
    c = lc.make_case(n, k)
    W, it = lc.oracle_w(ref, c, 5, 1e-9)
    Wr, itr = lc.oracle_w(ref, c, 5, 1e-9, reverse=True)
    d = relF(Wr, W)
    print(f"n={n} k={k}: order {d:.2e}, sweeps {it}")
    assert d < 1e-13 and it == itr == 5 * lc.live_columns(c)
    assert np.isfinite(W).all() and W.min() > 0
    assert np.array_equal(W[c["Wm"]], c["W0"][c["Wm"]])
    if k in lc.KS_FEW:
        # A rounded through fp32 moves the oracle by 1e-6 at most (measured 5e-8): the F32 mode's 2e-5 bar rests on the kernel
        W32, _ = lc.oracle_w(ref, dict(c, A=c["A"].astype(np.float32).astype(np.float64)), 5, 1e-9)
        d32 = relF(W32, W)
        print(f"   fp32-rounded A {d32:.2e}")
        assert d32 < 1e-6


@pytest.mark.parametrize("n,k", lc.PLAIN_CASES)
def test_case_without_penalties_and_mask_is_well_posed(n, k):
    c = lc.make_case(n, k)
    W, it = lc.oracle_w(ref, c, 5, 1e-9, mask=False, reg=[0, 0, 0])
    Wr, itr = lc.oracle_w(ref, c, 5, 1e-9, mask=False, reg=[0, 0, 0], reverse=True)
    assert relF(Wr, W) < 1e-13 and it == itr == 5 * n and np.isfinite(W).all() and W.min() > 0
    assert lc.form_of(n, k) == ((2, 32) if n == 65537 else (1, 64))


def test_sparse_and_nnlm_cases_are_well_posed():
    c, P = lc.sparse_case()
    assert 0.29 < P.mean() < 0.31 and 0 < (~P.any(axis=1)).sum() < 100  # a few rows without a stored entry: exact zeros
    W, it = lc.oracle_w(ref, c, 5, 1e-9)
    Wr, itr = lc.oracle_w(ref, c, 5, 1e-9, reverse=True)
    assert relF(Wr, W) < 1e-13 and it == itr == 5 * lc.live_columns(c) and np.isfinite(W).all() and W.min() >= 0
    assert lc.form_of(c["n"], c["k"]) == (1, 24)
    c = lc.nnlm_case()
    o = ref.c_nnlm(c["x"], c["y"], lc.REG, c["mask"], c["b0"], 5, 1e-9, 1, 2)
    orev = ref.c_nnlm(c["x"][::-1], c["y"][::-1], lc.REG, c["mask"], c["b0"], 5, 1e-9, 1, 2)
    assert relF(orev["coefficient"], o["coefficient"]) < 1e-13 and o["n_iteration"] == orev["n_iteration"]
    assert np.isfinite(o["coefficient"]).all() and o["coefficient"].min() > 0


@pytest.mark.parametrize("n,k", lc.EARLY_CASES)
def test_early_finisher_case_stops_early(n, k):
    """A setting of EARLY_SETTINGS exists at which the oracle's sweep total lies strictly between one sweep and the whole budget per
    live column; the two summation orders agree on the factor and (measured) on the count -- test_gpu_lee_forms.py allows the library
    that difference plus 2."""
    found = lc.early_setting(ref, n, k)
    assert found is not None
    inner, tol, W, it = found
    c = lc.make_case(n, k)
    live = lc.live_columns(c)
    assert live < it < inner * live
    assert 0.05 * inner * live < it < 0.95 * inner * live  # a real mix of early and late columns, not a handful on the tolerance
    Wr, itr = lc.oracle_w(ref, c, inner, tol, reverse=True)
    print(f"n={n} k={k}: inner {inner} tol {tol}: sweeps {it} / {itr} of {inner * live}, order {relF(Wr, W):.2e}")
    assert relF(Wr, W) < 1e-13 and abs(it - itr) <= 2
    assert lc.early_order_slack(ref, n, k) == abs(it - itr)


def test_tolerance_one_percent_stops_nothing_at_high_rank():
    """Why (30, 1e-2) is not among EARLY_SETTINGS: at k = 40 the oracle runs the whole budget on every live column."""
    c = lc.make_case(65537, 40)
    _, it = lc.oracle_w(ref, c, 30, 1e-2)
    assert it == 30 * lc.live_columns(c)
