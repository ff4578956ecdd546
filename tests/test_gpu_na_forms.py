"""Every instantiation of the square-loss half-step with missing entries against the oracle: the per-column solvers colsolve_row_kernel
(k_colsolve_row.h, fp32-operand mode), colsolve_strict_kernel and colsolve_ls_kernel (k_missing.h) and the per-column Gram kernels
na_gram_lds_kernel, na_gram_f16_kernel (k_missing.h) and sp_gram_kernel (k_sparse_na.h) at every rank 1 .. 64, in both modes, through
both doors (set_matrix with NaN, set_matrix_csc_missing), with and without masks and penalties (cases and the restated dispatch:
tests/na_solver_cases.py; that they reach all 47 instantiations and the conditions relied on here: tests/test_na_solver_cases_host.py).

A case is the W half-step of a 150 x 165 matrix with 20 % NaN, then the H half-step on the same handle.  Every run asks the handle
which solver and which Gram kernel ran ("na_solver_*", "na_solver_kr_*", "na_gram_*", "na_gram_nt_*" of nnlm_get_info) before it looks
at a number.  W is compared with ref.update(W0.T, H0, A.T, Wm.T, ...), H with the oracle's H half-step from the DEVICE's W, so that the H
check does not inherit W's deviation.  Bars, relative Frobenius: 1e-10 in the strict mode, the mode's 1e-4 contract in the fp32-operand
mode; masked entries and fully masked lines equal the input to the bit; strict sweep counts equal the oracle's; fp32-operand mode at the
tight setting |s - s_ref| <= 2 + s_ref // 1000 (tests/test_gpu_fuzz.py), at the loose setting a factor that misses the bar is held
column by column to the bar against the oracle's trajectory (scd_sweep_cases.stop_slack), at most MAX_FLIPS columns per launch.
Each test prints its largest deviations (`pytest -s`, lines "NADEV"); the largest per family are in DESIGN.md section 4.8."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import na_solver_cases as nc  # noqa: E402
from helpers import relF  # noqa: E402
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib  # noqa: E402
from oracle import ref  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = [("f64", _lib.PREC_F64, 1e-10), ("f32", _lib.PREC_F32, 1e-4)]
MAX_FLIPS = 3  # columns of one launch that may stop at another sweep than the oracle's (fp32-operand mode, loose setting): tests/test_gpu_scd_forms.py
INFO_KEYS = ("na_solver", "na_solver_kr", "na_gram", "na_gram_nt")

Run = collections.namedtuple("Run", "W sw iw H sh ih")


@pytest.fixture(autouse=True)
def _default_precision(monkeypatch):
    monkeypatch.delenv("NNLM_PRECISION", raising=False)


def info(h, side):
    return tuple(int(h.get_info(f"{key}_{side}")) for key in INFO_KEYS)


def chain(prec, door, c, w_setting, h_setting=None, method=1, which=(0, 1)):
    """The half-steps `which` (W, then H) on one fresh handle: Run(W, its sweeps, its info keys, H, its sweeps, its info keys)."""
    with nnlm_amd.Handle(0, prec) as h:
        assert info(h, "w") == info(h, "h") == (-1, -1, -1, -1)
        h.set_matrix_csc_missing(*nc.csc_of(c["A"])) if door == "sparse" else h.set_matrix(c["A"])
        h.set_factors(c["k"], c["W0"], c["H0"], c["Wm"], c["Hm"])
        W = H = sw = sh = iw = ih = None
        if 0 in which:
            h.half_step(0, c["reg"], w_setting[0], w_setting[1], method)
            W, _ = h.get_factors()
            sw, iw = h.take_sweeps(), info(h, "w")
            assert info(h, "h") == (-1, -1, -1, -1)
        if 1 in which:
            h.half_step(1, c["reg"], *(h_setting or w_setting), method)
            _, H = h.get_factors()
            sh, ih = h.take_sweeps(), info(h, "h")
    return Run(W, sw, iw, H, sh, ih)


def check_info(r, mode, door, method, c, what):
    """The eight info keys against the restated dispatch: before any number is compared."""
    k = c["k"]
    if r.iw is not None:
        assert r.iw == nc.info_of(mode, door, method, k, c["Wm"] is not None), (what, "W", r.iw)
    if r.ih is not None:
        assert r.ih == nc.info_of(mode, door, method, k, c["Hm"] is not None), (what, "H", r.ih)


def check_factor(X, X0, Xm, line, what):
    """Finite, non-negative; masked entries and the fully masked line equal the input bit for bit (X, X0, Xm: one line per row)."""
    assert np.isfinite(X).all() and (X >= 0).all(), what
    if Xm is not None:
        assert np.array_equal(X[Xm], X0[Xm]), what
        assert np.array_equal(X[line], X0[line]), what


def check_run(r, c, mode, bar, what, setting, method=1, slack=False, counts=True):
    """One chain against the oracle: (deviation of W, of H).  slack: fp32-operand mode at the loose setting (see the module docstring)."""
    W_ref, itw = nc.oracle_w(ref, c, *setting, method=method)
    H_ref, ith = nc.oracle_h(ref, c, r.W, *setting, method=method)
    dw, dh = relF(r.W, W_ref), relF(r.H, H_ref)
    # the line with nothing observed (its Gram is zero but for the penalties): the oracle's, to the bar on the scale of the factor
    X, R = (r.W[4], W_ref[4]) if c["rows_special"] else (r.H[:, 4], H_ref[:, 4])
    scale = float(np.abs(W_ref if c["rows_special"] else H_ref).max())
    dl = float(np.abs(X - R).max()) / scale
    print(f"NADEV {what}: relF W {dw:.3e} H {dh:.3e} all-missing line {dl:.3e} (bar {bar:g}); sweeps {r.sw} / {itw}, {r.sh} / {ith}")
    check_factor(r.W, c["W0"], c["Wm"], nc.MASKED_LINE_W, what)
    check_factor(r.H.T, c["H0"].T, None if c["Hm"] is None else c["Hm"].T, nc.MASKED_LINE_H, what)
    assert dl < bar, (what, dl)
    if slack:
        for which in (0, 1):
            X, X_ref, d = (r.W, W_ref, dw) if which == 0 else (r.H, H_ref, dh)
            if d >= bar:
                ds, flips = nc.stop_slack(ref, c, which, X, X_ref, r.W, setting, bar)
                print(f"NADEV {what}: {'WH'[which]} misses the bar with {d:.3e}; columns {flips} stopped at another sweep than the oracle's, "
                      f"with that allowed {ds:.3e}")
                assert 0 < len(flips) <= MAX_FLIPS, (what, which, flips)
                dw, dh = (ds, dh) if which == 0 else (dw, ds)
    assert dw < bar and dh < bar, (what, dw, dh)
    if counts and mode == "f64":
        assert (r.sw, r.sh) == (itw, ith), (what, r.sw, itw, r.sh, ith)
    elif counts and not slack:  # fp32-operand mode, tight setting
        assert abs(r.sw - itw) <= 2 + itw // 1000 and abs(r.sh - ith) <= 2 + ith // 1000, (what, r.sw, itw, r.sh, ith)
    return dw, dh


# ---- a. every rank --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("door", nc.DOORS)
@pytest.mark.parametrize("mode,prec,bar", MODES)
@pytest.mark.parametrize("k", nc.KS)
def test_every_rank_matches_the_oracle(k, mode, prec, bar, door):
    """Rank k, every variant (unmasked without penalties, masked with all three; at the rank ends also the swapped pairs): SCD at the
    tight and the loose setting, Lee's updates at the tight one: see the module docstring."""
    worst = collections.defaultdict(float)
    for variant in nc.variants_of(k):
        c = nc.make_case(k, variant)
        for sname, setting, method in (("tight", nc.TIGHT, 1), ("loose", nc.LOOSE, 1), ("lee", nc.TIGHT, 2)):
            name = nc.case_name(k, variant, sname)
            what = f"{name} {mode} {door}"
            r = chain(prec, door, c, setting, method=method)
            check_info(r, mode, door, method, c, what)
            dw, dh = check_run(r, c, mode, bar, what, setting, method, slack=(mode, sname) == ("f32", "loose"),
                               counts=name not in nc.ORDER_DEPENDENT)
            fam = nc.solver_of(mode, method, k, False)[0][0]
            worst[fam + " W"], worst[fam + " H"] = max(worst[fam + " W"], dw), max(worst[fam + " H"], dh)
    print(f"NADEV worst k={k} {mode} {door} {nc.gram_of(mode, door, k)[0][0]}: " + ", ".join(f"{key} {v:.3e}" for key, v in sorted(worst.items())))


# ---- b. row lists at every Gram instantiation -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("door", nc.DOORS)
@pytest.mark.parametrize("mode,prec,bar", MODES)
@pytest.mark.parametrize("k", nc.ROWLIST_KS)
def test_row_lists_at_every_gram_instantiation(k, mode, prec, bar, door):
    """One column per row-list length around the four-row groups, the 32-row gather steps, the fold every 256 rows and the switch between
    listing the missing and the present rows (1300 rows; k = 50: tests/test_gpu_parity.py), at ranks that reach every instantiation of
    the three Gram families: every column within 10 x the bar, the factor within the bar, the strict sweep count the oracle's."""
    c = nc.make_rowlist_case(k)
    what = f"rowlist k{k} {mode} {door}"
    r = chain(prec, door, c, nc.ROWLIST_SETTING, which=(1,))
    check_info(r, mode, door, 1, c, what)
    H_ref, ith = nc.oracle_h(ref, c, c["W0"], *nc.ROWLIST_SETTING)
    assert np.isfinite(r.H).all() and (r.H >= 0).all()
    dev = [relF(r.H[:, j], H_ref[:, j]) for j in range(c["m"])]
    j = int(np.argmax(dev))
    print(f"NADEV {what}: relF H {relF(r.H, H_ref):.3e}, worst column {dev[j]:.3e} with {nc.ROWLIST_LENS[j]} missing rows (bar {bar:g}); sweeps {r.sh} / {ith}")
    for j in range(c["m"]):
        assert dev[j] < 10 * bar, (what, nc.ROWLIST_LENS[j], dev[j])
    assert relF(r.H, H_ref) < bar, what
    if mode == "f64":
        assert r.sh == ith, (what, r.sh, ith)


# ---- c. unwritten Gram memory ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("door", nc.DOORS)
@pytest.mark.parametrize("mode,prec,bar", MODES)
@pytest.mark.parametrize("k", nc.RANK_ENDS)
def test_results_do_not_depend_on_unwritten_gram_memory(k, mode, prec, bar, door):
    """The Gram kernels write the upper triangle up to k of each KP x KP block; the rest of a newly allocated buffer is whatever the
    allocation held.  With every double of it a NaN (debug_poison_workspaces) the chain gives the same bits and sweep counts."""
    for variant in ("plain", "masked"):
        c = nc.make_case(k, variant)
        for sname, setting, method in (("tight", nc.TIGHT, 1), ("lee", nc.TIGHT, 2)):
            what = f"{nc.case_name(k, variant, sname)} {mode} {door}"
            clean = chain(prec, door, c, setting, method=method)
            _lib.debug_poison_workspaces(1)
            try:
                r = chain(prec, door, c, setting, method=method)
            finally:
                _lib.debug_poison_workspaces(0)
            for x in (clean, r):
                check_info(x, mode, door, method, c, what)
            assert np.isfinite(r.W).all() and np.isfinite(r.H).all(), what
            assert np.array_equal(r.W, clean.W) and np.array_equal(r.H, clean.H), (what, relF(r.W, clean.W), relF(r.H, clean.H))
            assert (r.sw, r.sh) == (clean.sw, clean.sh), (what, r.sw, clean.sw, r.sh, clean.sh)


# ---- d. limits ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("door", nc.DOORS)
@pytest.mark.parametrize("mode,prec,bar", MODES)
@pytest.mark.parametrize("k", nc.RANK_ENDS)
def test_inner_limits_and_a_negative_tolerance(k, mode, prec, bar, door):
    """A limit of 0 sweeps leaves the factor as it is, to the bit, and counts no sweep; a limit of 1; a negative tolerance (no column ever
    stops: the `0.0 > tol` branch) runs limit x unmasked-columns sweeps."""
    for variant in ("plain", "masked"):
        c = nc.make_case(k, variant)
        for sname, setting in nc.LIMIT_SETTINGS:
            what = f"{nc.case_name(k, variant, sname)} {mode} {door}"
            r = chain(prec, door, c, setting)
            check_info(r, mode, door, 1, c, what)
            check_run(r, c, mode, bar, what, setting)
            if setting[0] == 0:
                assert np.array_equal(r.W, c["W0"]) and np.array_equal(r.H, c["H0"]) and (r.sw, r.sh) == (0, 0), (what, r.sw, r.sh)
            elif sname == "negtol" and mode == "f64":  # (fp32-operand mode: within the tight setting's allowance, in check_run)
                assert (r.sw, r.sh) == (setting[0] * nc.live_columns(c), setting[0] * nc.live_columns_h(c)), (what, r.sw, r.sh)
