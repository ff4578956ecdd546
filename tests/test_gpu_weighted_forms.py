"""Every instantiation behind the per-entry-weights door (nnlm_set_matrix_csc_weighted) against the reference of weighted_cases.py: the
weighted form of sp_gram_kernel and the Gfull branch of sp_gram_fixup_kernel (k_sparse_na.h) and the per-column solvers they feed --
under absent = zero colsolve_strict_kernel in BOTH modes -- at every rank 1 .. 64, in both modes, through both doors (cases and the
restated dispatch: tests/weighted_form_cases.py; that they reach every instantiation and the conditions relied on here:
tests/test_weighted_form_cases_host.py).

A case is the W half-step of nc.make_case's 150 x 165 matrix, then the H half-step on the SAME handle with no set_factors in between, so
the solved W is handed to the next half-step's row copy.  Every run asks the handle which solver and which Gram kernel ran and whether
the handle is weighted before it looks at a number.  W is compared with the reference's W half-step, H with the reference's H half-step
from the DEVICE's W.  Bars, relative Frobenius: 1e-10 in the strict mode, the mode's 1e-4 contract in the fp32-operand mode; masked
entries and fully masked lines equal the input to the bit.  Sweep counts: strict mode exact (under weighted_zero with
wf.rounding_decided_columns() taken out, outside wf.FORMULATION_DEPENDENT); fp32-operand mode at the tight settings within
2 + s_ref // 1000 ((300, 1e-5), where columns stop between sweeps, is counted in the strict mode only); at the loose setting a factor
that misses the bar is held column by column to the bar against the reference's trajectory (scd_sweep_cases.stop_slack), at most
MAX_FLIPS columns per launch.
Each test prints its largest deviations (`pytest -s`, lines "WDEV"); the largest per door, mode and family are in DESIGN.md 4.23."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import na_solver_cases as nc  # noqa: E402
import sparse_cases as spc  # noqa: E402
import weighted_form_cases as wf  # noqa: E402
from helpers import relF  # noqa: E402
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = [("f64", _lib.PREC_F64, 1e-10), ("f32", _lib.PREC_F32, 1e-4)]
MAX_FLIPS = 3  # columns of one launch that may stop at another sweep than the reference's (fp32-operand mode, loose setting): tests/test_gpu_na_forms.py
INFO_KEYS = ("na_solver", "na_solver_kr", "na_gram", "na_gram_nt")
NONE_YET = (-1, -1, -1, -1)

Run = collections.namedtuple("Run", "W sw iw H sh ih")


@pytest.fixture(autouse=True)
def _default_precision(monkeypatch):
    monkeypatch.delenv("NNLM_PRECISION", raising=False)


def info(h, side):
    return tuple(int(h.get_info(f"{key}_{side}")) for key in INFO_KEYS)


def set_door(h, door, S, w):
    """door: a weighted door of wf.DOORS with the weights w, or the unweighted "sparse" (absent = missing) / "zero" doors."""
    if door in wf.DOORS:
        h.set_matrix_csc_weighted(S[0], S[1], S[2], w, S[3], absent_missing=door == "weighted_missing")
    elif door == "sparse":
        h.set_matrix_csc_missing(*S)
    else:
        h.set_matrix_csc(*S)
    assert h.get_info("sparse_weighted") == (1.0 if door in wf.DOORS else 0.0)


def chain(prec, door, P, setting, method=1, which=(0, 1), w=None):
    """The half-steps `which` (W, then H) on one fresh handle, no set_factors in between: Run(W, its sweeps, its info keys, H, ...)."""
    c = P["c"]
    with nnlm_amd.Handle(0, prec) as h:
        assert info(h, "w") == info(h, "h") == NONE_YET
        set_door(h, door, P["S"], P["w"] if w is None else w)
        h.set_factors(c["k"], c["W0"], c["H0"], c["Wm"], c["Hm"])
        W = H = sw = sh = iw = ih = None
        if 0 in which:
            h.half_step(0, c["reg"], setting[0], setting[1], method)
            W, _ = h.get_factors()
            sw, iw = h.take_sweeps(), info(h, "w")
            assert info(h, "h") == NONE_YET
        if 1 in which:
            h.half_step(1, c["reg"], setting[0], setting[1], method)
            W1, H = h.get_factors()
            sh, ih = h.take_sweeps(), info(h, "h")
            assert W is None or np.array_equal(W1, W)
    return Run(W, sw, iw, H, sh, ih)


def check_info(r, mode, door, method, c, what):
    """The info keys against the restated dispatch: before any number is compared."""
    if r.iw is not None:
        assert r.iw == wf.info_of(mode, door, method, c["k"], c["Wm"] is not None), (what, "W", r.iw)
    if r.ih is not None:
        assert r.ih == wf.info_of(mode, door, method, c["k"], c["Hm"] is not None), (what, "H", r.ih)


def check_factor(X, X0, Xm, line, what):
    assert np.isfinite(X).all() and (X >= 0).all(), what
    if Xm is not None:
        assert np.array_equal(X[Xm], X0[Xm]), what
        assert np.array_equal(X[line], X0[line]), what


def check_counts(s, s_ref, counts_ref, free, limit, slack, what):
    lo, hi = wf.count_bounds(s_ref, counts_ref, free, limit)
    assert lo - slack <= s <= hi + slack, (what, s, s_ref, (lo, hi), slack)


def check_run(r, P, mode, bar, what, sname, setting, method=1, slack=False):
    """One chain against the reference: (deviation of W, of H)."""
    c, door = P["c"], P["door"]
    cw, ch = [], []
    if c["variant"] in nc.VARIANTS and sname in ("tight", "loose", "mid", "lee"):
        W_ref, itw = wf.oracle_w_cached(door, c["k"], c["variant"], setting, method)
        cw = None
    else:
        W_ref, itw = wf.oracle_w(P, *setting, method=method, counts=cw)
    H_ref, ith = wf.oracle_h(P, r.W, *setting, method=method, counts=ch)
    dw, dh = relF(r.W, W_ref), relF(r.H, H_ref)
    # the line without stored entries and the line of weight 0: the reference's, to the bar on the scale of the factor
    rows = c["rows_special"]
    scale = float(np.abs(W_ref if rows else H_ref).max())
    dl = max(float(np.abs((r.W[ln] - W_ref[ln]) if rows else (r.H[:, ln] - H_ref[:, ln])).max()) for ln in (wf.EMPTY_LINE, wf.ZERO_LINE)) / scale
    print(f"WDEV {what}: relF W {dw:.3e} H {dh:.3e} empty / weight-0 lines {dl:.3e} (bar {bar:g}); sweeps {r.sw} / {itw}, {r.sh} / {ith}")
    check_factor(r.W, c["W0"], c["Wm"], nc.MASKED_LINE_W, what)
    check_factor(r.H.T, c["H0"].T, None if c["Hm"] is None else c["Hm"].T, nc.MASKED_LINE_H, what)
    assert dl < bar, (what, dl)
    if slack:
        for which in (0, 1):
            X, X_ref, d = (r.W, W_ref, dw) if which == 0 else (r.H, H_ref, dh)
            if d >= bar:
                ds, flips = wf.stop_slack(P, which, X, X_ref, r.W, setting, bar)
                print(f"WDEV {what}: {'WH'[which]} misses the bar with {d:.3e}; columns {flips} stopped at another sweep than the reference's, "
                      f"with that allowed {ds:.3e}")
                assert 0 < len(flips) <= MAX_FLIPS, (what, which, flips)
                dw, dh = (ds, dh) if which == 0 else (dw, ds)
    assert dw < bar and dh < bar, (what, dw, dh)
    if slack or (mode == "f32" and sname == "mid"):   # (fp32 operands: a stop between sweeps at 1e-5 is printed above, not counted)
        return dw, dh
    for side, s, s_ref, cnt in (("w", r.sw, itw, cw), ("h", r.sh, ith, ch)):
        free = wf.rounding_decided_columns(door, c["variant"], side) if method == 1 else ()
        if free and cnt is None:   # (the cached reference keeps no per-column counts: once more, for this variant only)
            cnt = []
            wf.oracle_w(P, *setting, method=method, counts=cnt)
        if wf.case_name(door, c["k"], c["variant"], sname, side) in wf.FORMULATION_DEPENDENT:
            continue
        check_counts(s, s_ref, cnt, free, setting[0], 0 if mode == "f64" else 2 + s_ref // 1000, (what, side))
    return dw, dh


# ---- a. every rank --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,prec,bar", MODES)
@pytest.mark.parametrize("door", wf.DOORS)
@pytest.mark.parametrize("k", wf.KS)
def test_every_rank_matches_the_reference(k, door, mode, prec, bar):
    """Rank k, every variant: SCD at the tight and the loose setting (at the rank ends also (300, 1e-5)), Lee's updates at the tight one."""
    worst = collections.defaultdict(float)
    for variant in nc.variants_of(k):
        P = wf.problem(door, k, variant)
        for sname, setting, method in wf.settings_of(k):
            what = f"{nc.case_name(k, variant, sname)} {mode} {door}"
            r = chain(prec, door, P, setting, method=method)
            check_info(r, mode, door, method, P["c"], what)
            dw, dh = check_run(r, P, mode, bar, what, sname, setting, method, slack=(mode, sname) == ("f32", "loose"))
            fam = wf.solver_of(mode, door, method, k, False)[0][0]
            worst[fam + " W"], worst[fam + " H"] = max(worst[fam + " W"], dw), max(worst[fam + " H"], dh)
    print(f"WDEV worst k={k} {mode} {door} {wf.gram_of(mode, door, k)[0]}: " + ", ".join(f"{key} {v:.3e}" for key, v in sorted(worst.items())))


# ---- b. segments and the fix-up at every KP -------------------------------------------------------------------------------------------------
def check_wide(r, P, mode, bar, what, which):
    c = P["c"]
    cnt = []
    if which == 1:
        X, (X_ref, it), s, lens = r.H, wf.oracle_h(P, c["W0"], *wf.WIDE_SETTING, counts=cnt), r.sh, np.diff(P["S"][0])
    else:
        X, (X_ref, it), s, lens = r.W.T, wf.oracle_w(P, *wf.WIDE_SETTING, counts=cnt), r.sw, np.diff(P["St"][0])
        X_ref = X_ref.T
    assert np.isfinite(X).all() and (X >= 0).all(), what
    dev = [relF(X[:, j], X_ref[:, j]) for j in range(X.shape[1])]
    j = int(np.argmax(dev))
    print(f"WDEV {what}: relF {relF(X, X_ref):.3e}, worst column {dev[j]:.3e} with {int(lens[j])} stored entries (bar {bar:g}); sweeps {s} / {it}")
    for j in range(X.shape[1]):
        assert dev[j] < 10 * bar, (what, int(lens[j]), dev[j])
    assert relF(X, X_ref) < bar, what
    if mode == "f64":
        assert s == it, (what, s, it)


@pytest.mark.parametrize("mode,prec,bar", MODES)
@pytest.mark.parametrize("door", wf.DOORS)
@pytest.mark.parametrize("k", wf.WIDE_KS)
def test_segments_and_the_fixup_in_the_csc(k, door, mode, prec, bar):
    """One column per stored length around the groups of four rows, the 16 rows in flight and the 2048-entry segments (4200 rows): every
    column within 10 x the bar, the factor within the bar, the strict count the reference's.  The columns of more than 2048 entries go
    through sp_gram_fixup_kernel<KP>, with the shared Gram under weighted_zero."""
    P = wf.wide_problem(door, k)
    what = f"wide k{k} {mode} {door}"
    r = chain(prec, door, P, wf.WIDE_SETTING, which=(1,))
    check_info(r, mode, door, 1, P["c"], what)
    check_wide(r, P, mode, bar, what, 1)


@pytest.mark.parametrize("mode,prec,bar", MODES)
@pytest.mark.parametrize("door", wf.DOORS)
@pytest.mark.parametrize("k", wf.WIDE_T_KS)
def test_segments_and_the_fixup_in_the_csr(k, door, mode, prec, bar):
    """The transpose: the W half-step's CSR holds the long lines.  Also under a Gram buffer of wf.WIDE_SLOTS slots (at least three chunks, a
    long line first in one and last in another): the same bits and counts."""
    P = wf.wide_problem(door, k, True)
    what = f"wide^T k{k} {mode} {door}"
    r = chain(prec, door, P, wf.WIDE_SETTING, which=(0,))
    check_info(r, mode, door, 1, P["c"], what)
    check_wide(r, P, mode, bar, what, 0)
    _lib.debug_alloc_limit(wf.wide_alloc_limit(k))
    try:
        with nnlm_amd.Handle(0, prec) as h:
            set_door(h, door, P["S"], P["w"])
            h.set_factors(k, P["c"]["W0"], P["c"]["H0"])
            h.half_step(0, P["c"]["reg"], *wf.WIDE_SETTING, 1)
            Wc, _ = h.get_factors()
            sc, chunks, workers = h.take_sweeps(), int(h.get_info("sp_gram_chunks")), int(h.get_info("sp_gram_workers"))
    finally:
        _lib.debug_alloc_limit(0)
    want = spc.predicted_counts(P["St"][0], k, alloc_limit=wf.wide_alloc_limit(k))
    assert chunks == want["sp_gram_chunks"] >= 3 and workers == want["sp_gram_workers"], (what, chunks, workers, want)
    assert np.array_equal(Wc, r.W) and sc == r.sw, (what, relF(Wc, r.W), sc, r.sw)


# ---- c. unwritten Gram memory ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,prec,bar", MODES)
@pytest.mark.parametrize("door", wf.DOORS)
@pytest.mark.parametrize("k", wf.RANK_ENDS)
def test_results_do_not_depend_on_unwritten_gram_memory(k, door, mode, prec, bar):
    """With every double of a new Gram buffer a NaN (debug_poison_workspaces) the chain gives the same bits and sweep counts."""
    for variant in ("plain", "masked"):
        P = wf.problem(door, k, variant)
        for sname, setting, method in (("tight", wf.TIGHT, 1), ("lee", wf.TIGHT, 2)):
            what = f"{nc.case_name(k, variant, sname)} {mode} {door}"
            clean = chain(prec, door, P, setting, method=method)
            _lib.debug_poison_workspaces(1)
            try:
                r = chain(prec, door, P, setting, method=method)
            finally:
                _lib.debug_poison_workspaces(0)
            for x in (clean, r):
                check_info(x, mode, door, method, P["c"], what)
            assert np.isfinite(r.W).all() and np.isfinite(r.H).all(), what
            assert np.array_equal(r.W, clean.W) and np.array_equal(r.H, clean.H), (what, relF(r.W, clean.W), relF(r.H, clean.H))
            assert (r.sw, r.sh) == (clean.sw, clean.sh), (what, r.sw, clean.sw, r.sh, clean.sh)


# ---- d. limits ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,prec,bar", MODES)
@pytest.mark.parametrize("door", wf.DOORS)
@pytest.mark.parametrize("k", wf.RANK_ENDS)
def test_inner_limits_and_a_negative_tolerance(k, door, mode, prec, bar):
    """A limit of 0 sweeps leaves both factors as they are, to the bit, and counts no sweep; a limit of 1; a negative tolerance (no column
    ever stops) runs limit x unmasked-columns sweeps."""
    for variant in ("plain", "masked"):
        P = wf.problem(door, k, variant)
        c = P["c"]
        for sname, setting in nc.LIMIT_SETTINGS:
            what = f"{nc.case_name(k, variant, sname)} {mode} {door}"
            r = chain(prec, door, P, setting)
            check_info(r, mode, door, 1, c, what)
            check_run(r, P, mode, bar, what, sname, setting)
            if setting[0] == 0:
                assert np.array_equal(r.W, c["W0"]) and np.array_equal(r.H, c["H0"]) and (r.sw, r.sh) == (0, 0), (what, r.sw, r.sh)
            elif mode == "f64" or door == "weighted_zero":   # (the strict solver; colsolve_row_kernel: within the tight allowance, in check_run)
                assert (r.sw, r.sh) == (setting[0] * nc.live_columns(c), setting[0] * nc.live_columns_h(c)), (what, r.sw, r.sh)


# ---- e. every weight 1: the unweighted doors ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,prec,bar", MODES)
@pytest.mark.parametrize("k", wf.RANK_ENDS)
def test_unit_weights_equal_the_unweighted_doors(k, mode, prec, bar):
    """Weights all 1: absent = missing equals set_matrix_csc_missing bit for bit, in factors and in counts (y * 1.0 is exact and the
    summation order is the plain form's); absent = zero equals set_matrix_csc to the bar (there the per-column sums are exactly zero, but
    the shared Gram is scaled and solved by other kernels)."""
    for variant in ("plain", "masked"):
        P = wf.problem("weighted_missing", k, variant)
        ones = np.ones(P["w"].size)
        for sname, setting, method in (("tight", wf.TIGHT, 1), ("loose", wf.LOOSE, 1), ("lee", wf.TIGHT, 2)):
            what = f"{nc.case_name(k, variant, sname)} {mode} unit weights"
            a, b = chain(prec, "weighted_missing", P, setting, method, w=ones), chain(prec, "sparse", P, setting, method)
            check_info(a, mode, "weighted_missing", method, P["c"], what)
            assert a.iw == b.iw and a.ih == b.ih, (what, a.iw, b.iw)
            assert np.array_equal(a.W, b.W) and np.array_equal(a.H, b.H), (what, relF(a.W, b.W), relF(a.H, b.H))
            assert (a.sw, a.sh) == (b.sw, b.sh), (what, a.sw, b.sw, a.sh, b.sh)
            if sname == "loose":
                continue   # (a tolerance-only stop is not comparable across kernels to a bar: tests/test_gpu_scd_forms.py)
            z, u = chain(prec, "weighted_zero", P, setting, method, w=ones), chain(prec, "zero", P, setting, method)
            check_info(z, mode, "weighted_zero", method, P["c"], what)
            assert u.iw == u.ih == NONE_YET, (what, u.iw)   # (the shared-Gram solvers of the dense path)
            dw, dh = relF(z.W, u.W), relF(z.H, u.H)
            print(f"WDEV {what}: weighted_zero against set_matrix_csc W {dw:.3e} H {dh:.3e} (bar {bar:g}); sweeps {z.sw} / {u.sw}, {z.sh} / {u.sh}")
            assert dw < bar and dh < bar, (what, dw, dh)
