"""Every instantiation of the dense square-loss SCD sweep against the oracle and against each other: sweep_scd_q_kernel and
sweep_scd_qw_kernel (k_sweep_q.h, strict fp64: plain and persistent form), sweep_scd_f_kernel (k_sweep_f.h, fp32 operands on the matrix
pipe) and sweep_row_kernel (k_sweep_r.h, fp32 operands, row form) at every rank 1 .. 64, with and without masks and penalties, with four
and eight wavefronts per workgroup (cases and the restated launch policy: tests/scd_sweep_cases.py; that they reach all 144
instantiations and every group count of the persistent form: tests/test_scd_sweep_cases_host.py).

A case is the W half-step of a 150 x 160 matrix on a handle that counts 1, 3, 5 or 10 compute units (nnlm_debug_set_cus), so the same
150 columns go through every family.  Every run asks the handle which form ran ("sweep_form_*", "sweep_groups_*", "cus" of
nnlm_get_info) before it looks at a number.  Bars: 1e-10 relative Frobenius against ref.update in the strict mode, the mode's 1e-4
contract in the fp32-operand mode; masked entries and fully masked columns equal the input to the bit; strict sweep counts equal the
oracle's (at the loose tolerance where the oracle's own count does not depend on the order of summation: all cases, see the host file).

The H half-step that follows on the same handle is the check on what the W sweep's epilogue leaves behind: half_step() (nnlm_mi355x.hip)
folds the Gram partial sums of the previous sweep's workgroups (gram_fold_kernel / factor16_fold_kernel, taken when sg_which names the
factor the previous half-step solved) instead of running a Gram pass, and the fp32-operand mode also takes max|x| and the split copy's
scale from it -- so H is compared with the oracle's chain ref.update(H0, W_oracle.T, A, ...) at the same bars.

Between forms on the same problem: plain against persistent, and four against eight wavefronts per workgroup in both fp32-operand
kernels, are the same operations per column in the same order: bit-identical factors and equal sweep counts.  The row form against the
matrix-pipe form: 2e-5 and sweep counts within 0.02 s + 2 (the bars of tests/test_gpu_wrap.py).  Each test prints its largest deviations
(`pytest -s`, lines "SCDDEV"); the largest per family are in DESIGN.md section 4.4."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scd_sweep_cases as sc  # noqa: E402
from helpers import relF  # noqa: E402
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib  # noqa: E402
from oracle import ref  # noqa: E402

pytestmark = pytest.mark.gpu

PRECS = [("f64", _lib.PREC_F64, 1e-10), ("f32", _lib.PREC_F32, 1e-4)]
CROSS = 2e-5  # row form against matrix-pipe form

Run = collections.namedtuple("Run", "W sw fw H sh fh")


@pytest.fixture(autouse=True)
def _default_precision(monkeypatch):
    monkeypatch.delenv("NNLM_PRECISION", raising=False)


def chain(prec, cus, c, w_setting, h_setting=None):
    """W half-step, then H half-step on the same handle, on a device that "has" `cus` compute units: Run(W, its sweeps, (form, groups),
    H, its sweeps, (form, groups))."""
    _lib.debug_set_cus(cus)  # (test hook of the C ABI: handles created from now on plan their launches for `cus` compute units)
    try:
        h = nnlm_amd.Handle(0, prec)
    finally:
        _lib.debug_set_cus(0)
    with h:
        assert int(h.get_info("cus")) == cus and int(h.get_info("sweep_form_w")) == -1
        h.set_matrix(c["A"])
        h.set_factors(c["k"], c["W0"], c["H0"], c["Wm"], c["Hm"])
        h.half_step(0, c["reg"], w_setting[0], w_setting[1], 1)
        W, _ = h.get_factors()
        sw = h.take_sweeps()
        fw = (int(h.get_info("sweep_form_w")), int(h.get_info("sweep_groups_w")))
        h.half_step(1, c["reg"], *(h_setting or w_setting), 1)
        _, H = h.get_factors()
        sh = h.take_sweeps()
        fh = (int(h.get_info("sweep_form_h")), int(h.get_info("sweep_groups_h")))
    return Run(W, sw, fw, H, sh, fh)


def want_form(pname, k, ncols, cus, inner):
    f = sc.policy(pname, k, ncols, cus, inner)
    return f, (sc.FORM_CODE[f.family], f.groups)


MAX_FLIPS = 3  # columns of one launch that may stop at another sweep than the oracle's (fp32-operand mode, loose setting): see check_run


def check_run(r, c, oracle, bar, what, slack=None):
    """One chain against the oracle's: (deviation of W, of H, flipped columns of W, of H).
    slack = the (loose) setting, fp32-operand mode only: where a factor misses the bar, scd_sweep_cases.stop_slack() holds every column
    that misses it to the bar against the oracle's own trajectory (the oracle's column after exactly t sweeps) and names those columns:
    they stopped at another sweep than the oracle's, which is tolerance-only in this mode.  Measured on the MI355X: 11 of the 148 loose
    cases have one or two such columns, the same ones in every form; more than MAX_FLIPS of 150 columns in one
    launch would be a stopping rule gone wrong, not rounding."""
    W_ref, _, H_ref, _ = oracle
    dw, dh = relF(r.W, W_ref), relF(r.H, H_ref)
    print(f"SCDDEV {what}: relF W {dw:.3e} H {dh:.3e} (bar {bar:g})")
    for X in (r.W, r.H):
        assert np.isfinite(X).all() and (X >= 0).all(), what
    if c["Wm"] is not None:
        assert np.array_equal(r.W[c["Wm"]], c["W0"][c["Wm"]]), what  # masked entries: the input, bit for bit
        assert np.array_equal(r.H[c["Hm"]], c["H0"][c["Hm"]]), what
        cols = sc.masked_columns(c["n"])
        assert np.array_equal(r.W[cols], c["W0"][cols]), what         # fully masked columns: untouched
    flips = [[], []]
    if slack is not None:
        for which in (0, 1):
            X, X_ref, d, W_fixed = (r.W, W_ref, dw, None) if which == 0 else (r.H, H_ref, dh, W_ref)
            if which == 1 and flips[0]:  # a row of W that stopped a sweep off moves all of H: the oracle's H half-step from THIS W
                W_fixed = r.W
                X_ref = sc.oracle_h(ref, c, r.W, *slack)[0]
                d = relF(r.H, X_ref)
            if d >= bar:
                ds, flips[which] = sc.stop_slack(ref, c, which, X, X_ref, W_fixed, slack, bar)
                print(f"SCDDEV {what}: {'WH'[which]} misses the bar with {d:.3e}; columns {flips[which]} stopped at another sweep than the oracle's, "
                      f"with that allowed {ds:.3e}")
                assert 0 < len(flips[which]) <= MAX_FLIPS, (what, which, flips[which])
                d = ds
            dw, dh = (d, dh) if which == 0 else (dw, d)
    assert dw < bar and dh < bar, (what, dw, dh)
    return dw, dh, flips[0], flips[1]


def without(X, rows):
    return np.delete(X, rows, axis=0) if rows else X


# ---- a. every instantiation against the oracle, and the forms against each other ------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,bar", PRECS)
@pytest.mark.parametrize("k", sc.KS)
def test_every_form_matches_the_oracle_and_the_other_forms(k, pname, prec, bar):
    """Rank k, every variant (unmasked without penalties, masked with all three; at the rank ends of every rank padding also the swapped
    pairs), the tight and the loose setting, every family of the mode: see the module docstring."""
    worst = collections.defaultdict(float)
    for variant in sc.variants_of(k):
        c = sc.make_case(k, variant)
        for sname, setting in sc.SETTINGS:
            name = sc.case_name(k, variant, sname)
            oracle = sc.oracle_chain(ref, k, variant, setting)
            runs, off = {}, {}  # (off: columns that stopped a sweep off the oracle's, fp32-operand mode at the loose setting only)
            for cus in sc.cus_of(pname, k):
                f, code = want_form(pname, k, sc.N, cus, setting[0])
                r = chain(prec, cus, c, setting)
                assert r.fw == code and r.fh == want_form(pname, k, sc.M, cus, setting[0])[1], (name, cus, r.fw, r.fh, f)
                runs[(f.family, f.groups)] = r
                dw, dh, fw_, fh_ = check_run(r, c, oracle, bar, f"{name} {pname} {f.family}{f.groups}",
                                             slack=setting if (pname, sname) == ("f32", "loose") else None)
                off[(f.family, f.groups)] = (fw_, fh_)
                worst[f.family + " W"], worst[f.family + " H"] = max(worst[f.family + " W"], dw), max(worst[f.family + " H"], dh)
                if pname == "f64" and name not in sc.LOOSE_ORDER_DEPENDENT:
                    assert (r.sw, r.sh) == (oracle[1], oracle[3]), (name, cus, r.sw, r.sh, oracle[1], oracle[3])
            if pname == "f64":
                pairs = [(("q", 4), ("qw", 5), True)]
            else:
                pairs = [(("f", 4), ("f", 8), True)]
                if k <= sc.SWEEPR_KMAX:
                    pairs += [(("r", 4), ("r", 8), True), (("r", 4), ("f", 4), False), (("r", 8), ("f", 8), False)]
            for fa, fb, same in pairs:
                ra, rb = runs[fa], runs[fb]
                offw, offh = sorted(set(off[fa][0] + off[fb][0])), sorted(set(off[fa][1] + off[fb][1]))
                d = relF(without(ra.W, offw), without(rb.W, offw))
                key = f"{fa[0]}{fa[1]}:{fb[0]}{fb[1]}"
                worst[key] = max(worst[key], d)
                if same:  # the same operations per column in the same order
                    assert np.array_equal(ra.W, rb.W) and ra.sw == rb.sw, (name, key, d, ra.sw, rb.sw)
                    # (H: the Gram partial sums are per workgroup -- the same sum in another order: close, not identical)
                    dh = relF(without(ra.H.T, offh), without(rb.H.T, offh))
                    assert dh < (1e-10 if pname == "f64" else CROSS), (name, key, dh)
                else:
                    assert d < CROSS, (name, key, d)
                    assert abs(ra.sw - rb.sw) <= 0.02 * rb.sw + 2, (name, key, ra.sw, rb.sw)
    print(f"SCDDEV worst k={k} {pname}: " + ", ".join(f"{key} {v:.3e}" for key, v in sorted(worst.items())))


# ---- b. the persistent form at every group count the policy can choose ----------------------------------------------------------------------
@pytest.mark.parametrize("cus,n,G", sc.G_SHAPES)
@pytest.mark.parametrize("k", sc.KS_FEW)
def test_persistent_form_at_every_group_count(k, cus, n, G):
    """Strict mode, masked, NB = 1, 6, 11, 15 at G = 5, 6, 7, 9: against the oracle, and bit-identical to the plain form (a device with
    enough compute units for one wavefront per SIMD)."""
    c = sc.make_case(k, "masked", n)
    for sname, setting in sc.SETTINGS:
        oracle = sc.oracle_chain(ref, k, "masked", setting, None, False, n)
        r = chain(_lib.PREC_F64, cus, c, setting)
        assert r.fw == (1, G), (r.fw, G)
        p = chain(_lib.PREC_F64, 8, c, setting)
        assert p.fw == (0, 4) and p.fh == (0, 4)
        check_run(r, c, oracle, 1e-10, f"k{k}-n{n}-{sname} f64 qw{G}")
        check_run(p, c, oracle, 1e-10, f"k{k}-n{n}-{sname} f64 q4")
        assert np.array_equal(r.W, p.W) and r.sw == p.sw == oracle[1], (sname, r.sw, p.sw, oracle[1])
        assert r.sh == p.sh == oracle[3], (sname, r.sh, p.sh, oracle[3])


# ---- c. inner limits below the persistent form's threshold ----------------------------------------------------------------------------------
@pytest.mark.parametrize("inner", sc.INNER_LIMITS)
@pytest.mark.parametrize("k", sc.KS_FEW)
def test_inner_limits_below_four_take_the_plain_form(k, inner):
    """Strict mode, ten column groups on four SIMDs with a limit of 0, 1 or 3 sweeps: the plain form beyond one wavefront per SIMD.
    0 = no sweep: W is the input to the bit, the epilogue still leaves the Gram sums the H half-step (tight setting, persistent form) uses."""
    c = sc.make_case(k, "masked")
    w_setting = (inner, sc.TIGHT[1])
    oracle = sc.oracle_chain(ref, k, "masked", w_setting, sc.TIGHT)
    r = chain(_lib.PREC_F64, 1, c, w_setting, sc.TIGHT)
    assert r.fw == (0, 4) and r.fh == (1, 5), (r.fw, r.fh)
    check_run(r, c, oracle, 1e-10, f"k{k}-inner{inner} f64 q4")
    assert (r.sw, r.sh) == (oracle[1], oracle[3]), (r.sw, r.sh, oracle[1], oracle[3])
    if inner == 0:
        assert np.array_equal(r.W, c["W0"]) and r.sw == 0
