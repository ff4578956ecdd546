"""Launch forms of the SCD sweep.  Strict fp64 mode: the persistent ("wrap-around") form (k_sweep_q.h, sweep_scd_qw_kernel) -- between one and two wavefronts of 16
columns per SIMD the launch gives every CU G = 5, 6, 7 or 9 column groups (the cheapest; a tie keeps the smaller G, so 8 and 10 are never
taken: tests/test_scd_sweep_cases_host.py), which its four wavefronts share by McNaughton's rule -- a group
cut by a piece boundary is started by one wavefront and finished by another, its state handed over through LDS.  Same arithmetic per
column as the plain form, so the results must be BIT-IDENTICAL to it: the device is made to look small (nnlm_debug_set_cus, read by
nnlm_create) so that a few hundred columns take the persistent form, and the same problem is run on the plain form for comparison;
both are also held against the oracle.  The benchmark's W half-step (20000 columns on 256 CUs: G = 5) takes this form at full size
(tests/test_gpu_fullsize.py).
fp32-operand mode: what runs here today.  A device "with" 1 - 3 CUs takes the fp32-chain kernel (k_sweep_f.h, sweep_scd_f_kernel;
nnlm_get_info form 2) with workgroups of four wavefronts (one per SIMD) up to one wavefront per SIMD of the device and of eight (two per
SIMD) beyond; the real device takes the row form (k_sweep_r.h, sweep_row_kernel; form 3) at these sizes for k <= 50 and the fp32-chain
kernel with four wavefronts at k = 64.  So the F32 branch of the first test compares the matrix-pipe form with the row form (other
starting-gradient arithmetic: 2e-5), not two widths of one kernel.  The two widths of either kernel do the same operations per column in
the same order; that they are bit-identical is asserted by tests/test_gpu_scd_forms.py, at every rank.
Ranks run here: strict plain and persistent k = 7, 33, 50, 64 (NB = 2, 9, 13, 16; masks at NB = 2 and 16), the policy test k = 8; fp32
chain on a small device k = 5, 7, 16, 17, 32, 33, 48, 49, 50, 51, 64; row form k = 5 .. 50 of the third test's list."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import relF  # noqa: E402
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib  # noqa: E402
from oracle import ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(monkeypatch, cus, prec, A, k, W0, H0, Wm, Hm, reg, inner, tol, iters):
    """(W, H, sweeps) after `iters` outer iterations; iters = 'W' / 'H': ONE half-step from the given factors."""
    _lib.debug_set_cus(cus)  # (test hook of the C ABI: handles created from now on plan their launches for `cus` compute units)
    try:
        h = nnlm_amd.Handle(0, prec)
    finally:
        _lib.debug_set_cus(0)
    with h:
        h.set_matrix(A)
        h.set_factors(k, W0, H0, Wm, Hm)
        if iters in ("W", "H"):
            h.half_step(0 if iters == "W" else 1, reg, inner, tol, 1)
        else:
            h.iterate(iters, reg, reg, inner, tol, 1)
        W, H = h.get_factors()
        sw = h.take_sweeps()
    return W, H, sw


@pytest.mark.parametrize("pname,prec,otol", [("f64", _lib.PREC_F64, 1e-9), ("f32", _lib.PREC_F32, 1e-4)])
@pytest.mark.parametrize("cus,n,m", [(2, 150, 224), (3, 260, 330), (1, 70, 112),  # G = 5 .. 7 each way (150 -> 5, 224 -> 7, 260 -> 6, 330 -> 7, 70 -> 5, 112 -> 7), ragged ends
                                     (1, 144, 160),   # round 5: 9 groups on one CU -> G = 9; 10 groups -> G = 5 in two rounds of workgroups
                                     (2, 400, 300)])  # 25 groups on two CUs -> G = 7, four workgroups = two rounds; 19 groups -> G = 5, four workgroups (G = 10 in one round costs the same: the tie keeps 5)
@pytest.mark.parametrize("k,masks,inner,itol", [(50, False, 50, 1e-9), (7, True, 9, 1e-9), (64, True, 6, 1e-2), (33, False, 50, 1e-3)])
def test_persistent_sweep_is_bit_identical_to_the_plain_form(monkeypatch, pname, prec, otol, cus, n, m, k, masks, inner, itol):
    rng = np.random.default_rng(1000 * k + n + cus)
    kk = min(k, n, m)
    Wp, Hp = rng.random((n, kk + 2)) ** 2 + 0.05, rng.random((kk + 2, m)) ** 2 + 0.05
    A = Wp @ Hp / (kk + 2) * 4 + 0.02 * rng.random((n, m)) + 0.01
    sc = 2.0 / np.sqrt(kk + 2)
    W0, H0 = Wp[:, :kk] * sc * (0.7 + 0.6 * rng.random((n, kk))), Hp[:kk, :] * sc * (0.7 + 0.6 * rng.random((kk, m)))
    Wm = Hm = None
    if masks:
        Wm, Hm = rng.random((n, kk)) < 0.1, rng.random((kk, m)) < 0.1
        Wm[3, :] = True  # a column of the W half-step with every coordinate masked: skipped (src/update_with_missing.cpp:33)
        W0[Wm] = 0.0
        H0[Hm] = 0.0
    reg = [0.01, 0.0, 0.005]
    # one half-step from the same factors, each orientation: the same operations per column in the same order -- bit for bit
    for which in ("W", "H"):
        Ww, Hw, sww = _run(monkeypatch, cus, prec, A, kk, W0, H0, Wm, Hm, reg, inner, itol, which)
        Wp_, Hp_, swp = _run(monkeypatch, 0, prec, A, kk, W0, H0, Wm, Hm, reg, inner, itol, which)
        if pname == "f64":
            assert np.array_equal(Ww, Wp_) and np.array_equal(Hw, Hp_), (which, relF(Ww, Wp_), relF(Hw, Hp_))
            assert sww == swp
        else:
            # fp32-operand mode since the end of round 6: at these sizes the real device takes the row form of the sweep (k_sweep_r.h), the
            # device "with" 1-3 CUs the matrix-pipe form (k_sweep_f.h) -- other starting-gradient arithmetic, the same recurrence: close
            assert relF(Ww, Wp_) < 2e-5 and relF(Hw, Hp_) < 2e-5, (which, relF(Ww, Wp_), relF(Hw, Hp_))
            assert abs(sww - swp) <= 0.02 * swp + 2, (sww, swp)
    # two iterations: the Gram partial sums a sweep leaves behind are per workgroup, 16 G columns here and 64 there, so the next
    # half-step's Gram is the same sum in another order (1e-16): close, not identical; both against the oracle
    Ww, Hw, sww = _run(monkeypatch, cus, prec, A, kk, W0, H0, Wm, Hm, reg, inner, itol, 2)
    Wp_, Hp_, swp = _run(monkeypatch, 0, prec, A, kk, W0, H0, Wm, Hm, reg, inner, itol, 2)
    close = 1e-10 if pname == "f64" else 5e-5  # (fp32-operand mode: two sweep forms, see above)
    assert relF(Ww, Wp_) < close and relF(Hw, Hp_) < close, (relF(Ww, Wp_), relF(Hw, Hp_))
    o = ref.c_nnmf(A, kk, W0, H0, Wm, Hm, reg, reg, 2, -1.0, 0, 0, False, inner, itol, 1, 2)
    assert relF(Ww, o["W"]) < otol and relF(Hw, o["H"]) < otol
    if pname == "f64" and itol < 1e-6:  # (sweep counts at a loose inner tolerance ride on rounding)
        assert sww == int(round(float(np.sum(o["average_epoch"])) * (n + m)))


def test_launch_policy_picks_the_cheapest_form(monkeypatch):
    """nnlm_get_info reports the form the last SCD sweep took: plain up to one wavefront per SIMD, the persistent form with the group
    count per workgroup that costs least beyond (costs in quarter sweeps: plain ceil(groups / SIMDs) * 4, persistent rounds * G)."""
    rng = np.random.default_rng(5)
    k = 8
    cases = [(_lib.PREC_F64, cus, n, want) for cus, n, want in
             [(2, 128, (0, 4)), (2, 150, (1, 5)), (1, 144, (1, 9)), (1, 128, (0, 4)), (2, 400, (1, 7)), (2, 304, (1, 5)), (2, 280, (1, 9))]]
    # fp32-operand mode: form 2 = the fp32-chain kernel, "groups" = wavefronts per workgroup (4 up to one wavefront per SIMD, 8 beyond)
    cases += [(_lib.PREC_F32, 2, 128, (2, 4)), (_lib.PREC_F32, 2, 150, (2, 8)), (_lib.PREC_F32, 1, 64, (2, 4)), (_lib.PREC_F32, 1, 400, (2, 8))]
    for prec, cus, n, want in cases:
        A = rng.random((n, 40))
        _lib.debug_set_cus(cus)
        try:
            h = nnlm_amd.Handle(0, prec)
        finally:
            _lib.debug_set_cus(0)
        with h:
            assert int(h.get_info("cus")) == cus and int(h.get_info("sweep_form_w")) == -1
            h.set_matrix(A)
            h.set_factors(k, rng.random((n, k)), rng.random((k, 40)))
            h.half_step(0, [0, 0, 0], 10, 1e-9, 1)
            h.sync()
            assert (int(h.get_info("sweep_form_w")), int(h.get_info("sweep_groups_w"))) == want, (cus, n)


@pytest.mark.parametrize("n,k", [(100, 5), (100, 16), (100, 48), (4096, 50), (4100, 50), (8192, 50), (8200, 50), (4100, 17), (8192, 33),
                                 (4100, 51), (1000, 32), (3000, 49)])
def test_fp32_sweep_takes_the_row_form_while_it_is_one_round_of_wavefronts(n, k):
    """fp32-operand mode, dense SCD: up to 16 columns per CU the sweep runs as sweep_row_kernel with four-wavefront workgroups (form 3,
    groups 4), up to 32 per CU with eight, beyond -- and for ranks above 50 -- as sweep_scd_f_kernel (form 2).  One W half-step with masks
    and all three penalties against the oracle, and against the same half-step with the matrix-pipe form forced (a device that "has" one CU)."""
    rng = np.random.default_rng(100 * k + n % 97)
    m = 64
    Wp, Hp = rng.random((n, k + 2)) ** 2 + 0.05, rng.random((k + 2, m)) ** 2 + 0.05
    A = Wp @ Hp / (k + 2) * 4 + 0.02 * rng.random((n, m)) + 0.01
    sc = 2.0 / np.sqrt(k + 2)
    W0, H0 = Wp[:, :k] * sc * (0.7 + 0.6 * rng.random((n, k))), Hp[:k, :] * sc * (0.7 + 0.6 * rng.random((k, m)))
    Wm = rng.random((n, k)) < 0.05
    W0 = np.where(Wm, 0.3 * W0, W0)
    reg = [0.01, 0.004, 0.005]

    def run(cus):
        _lib.debug_set_cus(cus)
        try:
            h = nnlm_amd.Handle(0, _lib.PREC_F32)
        finally:
            _lib.debug_set_cus(0)
        with h:
            h.set_matrix(A)
            h.set_factors(k, W0, H0, Wm, None)
            h.half_step(0, reg, 30, 1e-7, 1)
            W, _ = h.get_factors()
            return W, h.take_sweeps(), (int(h.get_info("sweep_form_w")), int(h.get_info("sweep_groups_w"))), int(h.get_info("cus"))

    W3, s3, f3, cus = run(0)
    if cus == 256:
        want = (2, 4) if k > 50 else ((3, 4) if n <= 4096 else ((3, 8) if n <= 8192 else (2, 4)))
        assert f3 == want, (n, k, f3)
    W2, s2, f2, _ = run(1)
    assert f2[0] == 2
    Wt, sweeps = ref.update(W0.T.copy(), H0, np.ascontiguousarray(A.T), Wm.T.copy(), reg, 30, 1e-7, 1)
    assert relF(W3, Wt.T) < 1e-4 and relF(W2, Wt.T) < 1e-4, (relF(W3, Wt.T), relF(W2, Wt.T))
    assert relF(W3, W2) < 2e-5, relF(W3, W2)
    assert np.array_equal(W3[Wm], W0[Wm])  # masked entries: the input, to the bit
    assert abs(s3 - s2) <= 0.02 * s2 + 2, (s3, s2, sweeps)  # (sweep counts: tolerance-only in this mode)


@pytest.mark.parametrize("prec,form", [(_lib.PREC_F64, 1), (_lib.PREC_F32, 2)])
def test_sweep_time_scales_with_the_work_beyond_two_wavefronts_per_simd(prec, form):
    """(fp32-operand mode: 20000 columns are one round of 157 eight-wavefront workgroups, 40000 two rounds of the 256 CUs.)
    VERDICT r4 item 6: the persistent form for any group count.  40000 columns (2500 groups of 16 on 1024 SIMDs: G = 5 in two rounds of 250 workgroups -- G = 10 in one round
    costs the same and the tie keeps 5 --, 125 sweeps of work per wavefront) must not cost more than 1.25 x per unit of work what 20000 columns cost (1250 groups: G = 5, 63 sweeps) -- the
    plain form took three whole rounds of wavefronts for 2.44 rounds of work there."""
    rng = np.random.default_rng(11)
    k, m = 50, 256
    per_col = {}
    for n in (20000, 40000):
        A = rng.random((n, m))
        with nnlm_amd.Handle(0, prec) as h:
            h.set_matrix(A)
            h.set_factors(k, 0.01 * rng.random((n, k)), 0.01 * rng.random((k, m)))
            for _ in range(3):
                h.half_step(0, [0, 0, 0], 50, -1.0, 1)  # (inner.rel.tol < 0: always 50 sweeps)
            h.sync()
            h.profile_reset()
            h.profile_enable(True)
            for _ in range(5):
                h.half_step(0, [0, 0, 0], 50, -1.0, 1)
            h.sync()
            ms, cnt = h.profile_get("sweep_w")
            h.profile_enable(False)
            assert cnt == 5 and int(h.get_info("sweep_form_w")) == form
            per_col[n] = ms / cnt / n
            print(f"sweep_w at {n} columns: {ms / cnt:.4f} ms, G = {int(h.get_info('sweep_groups_w'))}")
    assert per_col[40000] <= 1.25 * per_col[20000], per_col


@pytest.mark.parametrize("pname,prec,tol", [("f64", _lib.PREC_F64, 1e-9), ("f32", _lib.PREC_F32, 1e-4)])
def test_forty_thousand_columns_on_the_real_device_match_the_oracle(pname, prec, tol):
    """The launch forms the real CU count produces beyond two wavefronts per SIMD, against the oracle: 40000 columns (2500 groups: the
    persistent form in two rounds of workgroups) and 29000 (1813 groups: the plain form in two rounds of wavefronts), one W half-step of
    50 sweeps each, both arithmetic modes; sweep counts exact in the strict mode."""
    rng = np.random.default_rng(23)
    k, m = 50, 192
    for n, want_form in ((40000, 1), (29000, 0)):
        Wp, Hp = rng.random((n, k + 2)) ** 2 + 0.05, rng.random((k + 2, m)) ** 2 + 0.05
        A = Wp @ Hp / (k + 2) * 4 + 0.02 * rng.random((n, m)) + 0.01
        sc = 2.0 / np.sqrt(k + 2)
        W0, H0 = Wp[:, :k] * sc * (0.7 + 0.6 * rng.random((n, k))), Hp[:k, :] * sc * (0.7 + 0.6 * rng.random((k, m)))
        reg = [0.01, 0.0, 0.005]
        with nnlm_amd.Handle(0, prec) as h:
            h.set_matrix(A)
            h.set_factors(k, W0, H0)
            h.half_step(0, reg, 50, 1e-9, 1)
            W, _ = h.get_factors()
            sw = h.take_sweeps()
            if int(h.get_info("cus")) == 256:
                assert int(h.get_info("sweep_form_w")) == (want_form if pname == "f64" else 2), (n, h.get_info("sweep_groups_w"))
        # the W half-step is update(Wt, H, A^T) (src/nnmf.cpp:131): Wt k x n solved, H the fixed factor, contraction over the m columns of A
        Wt, sweeps = ref.update(W0.T.copy(), H0, np.ascontiguousarray(A.T), None, reg, 50, 1e-9, 1)
        assert relF(W, Wt.T) < tol, (n, relF(W, Wt.T))
        if pname == "f64":
            assert sw == sweeps, (n, sw, sweeps)
