"""xprod16_tn_kernel (fp32-operand mode) in its two block widths -- 8 wavefronts = 128-column tiles, 10 wavefronts = 160-column tiles --
and with the factor image trimmed to 13 pieces at k = 49 .. 52 (a zeroed LDS row stands in for the rows that are not loaded).

The cross product is read through debug_partial(which) and compared with Y @ B in numpy at the fp32-operand bound of
tests/test_gpu_parity.py (PRECS: 2e-5); the form is forced with nnlm_debug_set_xprod_waves and asserted through get_info.  700 x 300 pads
to 768 x 384 columns: the last 160-column tile has 8 live wavefronts on the W side and 4 on the H side."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import relF  # noqa: E402
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib  # noqa: E402
from oracle import ref  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 2e-5        # PRECS of tests/test_gpu_parity.py, fp32-operand mode
TOL_FORMS = 2e-7  # a changed slab count / block width: the bound the virtual-rank test puts on it (tol * 1e-2)
F32 = _lib.PREC_F32


@pytest.fixture(autouse=True)
def _default_precision(monkeypatch):
    monkeypatch.delenv("NNLM_PRECISION", raising=False)


def handle(waves):
    _lib.debug_set_xprod_waves(waves)
    try:
        return nnlm_amd.Handle(0, F32)
    finally:
        _lib.debug_set_xprod_waves(0)


def partial(waves, A, W0, H0, which, expect):
    k = W0.shape[1]
    with handle(waves) as h:
        h.set_matrix(A)
        h.set_factors(k, W0, H0)
        G, Cp = h.debug_partial(which)
        side = "h" if which == 1 else "w"
        got = int(h.get_info("xprod_waves_" + side))
        splits = int(h.get_info("xprod_splits_" + side))
    assert got == expect or (expect is None and got in (8, 10)), (waves, k, which, got)
    assert splits >= 1
    return (Cp, got) if expect is None else Cp


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(160)
    n, m = 700, 300
    A = rng.random((n, m))
    W = rng.random((n, 64))
    H = rng.random((64, m))
    return A, W, H


def products(A, W0, H0, which):
    Y = W0.T if which == 1 else H0
    B = A if which == 1 else A.T
    return Y @ B


@pytest.mark.parametrize("which", [0, 1])
def test_stale_image_rows_then_every_rank(data, which):
    """k = 64 first (every row of the factor image written with data), then k = 5 in the same process: an image row that was never
    zeroed would hold the old data.  Then the ranks around every piece / tile boundary, 10 wavefronts; 53 and 64 must fall back to 8."""
    A, W, H = data
    for k, expect in [(64, 8), (5, 10), (1, 10), (3, 10), (4, 10), (16, 10), (17, 10), (48, 10), (49, 10), (52, 10), (53, 8)]:
        W0, H0 = np.ascontiguousarray(W[:, :k]), np.ascontiguousarray(H[:k, :])
        C = partial(10, A, W0, H0, which, expect)
        err = relF(C, products(A, W0, H0, which))
        print(f"which={which} k={k} waves={expect} relF={err:.3e}")
        assert err < TOL, (k, err)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("k", [3, 11, 50, 64])
def test_eight_and_ten_wavefronts_agree(data, which, k):
    A, W, H = data
    W0, H0 = np.ascontiguousarray(W[:, :k]), np.ascontiguousarray(H[:k, :])
    C8 = partial(8, A, W0, H0, which, 8)
    C10 = partial(10, A, W0, H0, which, 10 if k <= 52 else 8)
    ref_c = products(A, W0, H0, which)
    e8, e10, d = relF(C8, ref_c), relF(C10, ref_c), relF(C10, C8)
    print(f"which={which} k={k} relF8={e8:.3e} relF10={e10:.3e} 8-vs-10={d:.3e}")
    assert e8 < TOL and e10 < TOL
    assert d < TOL_FORMS
    # the plan's own choice is one of the two
    C0, w0 = partial(0, A, W0, H0, which, None)
    assert np.array_equal(C0, C8 if w0 == 8 else C10)


def test_split_contraction_both_widths():
    """1100 rows pad to 20 stages: the plan cuts the H half-step's contraction into two slabs of 10, summed by the consumer."""
    rng = np.random.default_rng(20)
    n, m, k = 1100, 300, 50
    A = rng.random((n, m))
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    out = {}
    for waves in (8, 10):
        with handle(waves) as h:
            h.set_matrix(A)
            h.set_factors(k, W0, H0)
            _, out[waves] = h.debug_partial(1)
            plan = _lib.xprod_plan(384, 20, k, int(h.get_info("cus")), waves)  # (two slabs on a whole device)
            assert int(h.get_info("xprod_waves_h")) == waves and int(h.get_info("xprod_splits_h")) == plan["splits"]
    ref_c = W0.T @ A
    assert relF(out[8], ref_c) < TOL and relF(out[10], ref_c) < TOL
    assert relF(out[10], out[8]) < TOL_FORMS


@pytest.mark.parametrize("waves", [8, 10])
def test_short_contractions(waves):
    """40 x 40 pads to a contraction of 4 stages (H side) and 2 stages (W side): fewer stages than the ring has buffers in flight, fewer
    than 8 per slab.  Two virtual ranks halve the W side's contraction: ONE stage each."""
    rng = np.random.default_rng(41)
    n = m = 40
    k = 7
    A = rng.random((n, m))
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    for which in (0, 1):
        C = partial(waves, A, W0, H0, which, waves)
        assert relF(C, products(A, W0, H0, which)) < TOL
    Y, B = H0, A.T
    Cs = 0.0
    for rk in range(2):
        with handle(waves) as h:
            h.set_matrix(A)
            h.set_factors(k, W0, H0)
            h.comm_init(None, rk, 2, form="reduce")
            _, Cp = h.debug_partial(0)
            assert int(h.get_info("xprod_waves_w")) == waves
        b, e = _lib.shard_range(n, m, F32, 0, rk, 2)
        if rk == 0:
            assert e - b <= 64  # one stage
        if e > b:
            assert relF(Cp, Y[:, b:e] @ B[b:e, :]) < TOL
        Cs = Cs + Cp
    assert relF(Cs, Y @ B) < TOL


@pytest.mark.parametrize("k", [11, 50])
@pytest.mark.parametrize("waves", [8, 10])
def test_three_iterations_match_the_oracle(monkeypatch, data, waves, k):
    """Three whole nnmf iterations in fp32-operand mode with the form forced, against the oracle at the whole-iteration bounds of
    tests/test_gpu_parity.py (fp32-operand mode: 1e-4 on the factors, 10 x that on the traces).  Trace every second iteration: the W
    half-step of iteration 1 is the fused cross product / error kernel (128 columns), those of iterations 0 and 2 the plain kernel in
    the forced width, on the same slabs.  Once through the one-shot driver (NNLM_PRECISION=f32), once through the resident loop on a
    handle, whose launches are asserted."""
    monkeypatch.setenv("NNLM_PRECISION", "f32")
    A, W, H = data
    W0, H0 = 0.01 * np.ascontiguousarray(W[:, :k]), 0.01 * np.ascontiguousarray(H[:k, :])
    z = [0.0, 0.0, 0.0]
    tol = 1e-4
    args = (A, k, W0, H0, None, None, z, z, 3, -1.0, 1, 0, False, 50, 1e-9, 1, 2)
    o = ref.c_nnmf(*args)
    assert o["n_iteration"] == 3

    def check(r, Wn, Hn):
        assert r["n_iteration"] == 3
        assert relF(Wn, o["W"]) < tol and relF(Hn, o["H"]) < tol
        for key in ("mse_error", "mkl_error", "target_error"):
            assert r[key].shape == o[key].shape
            assert np.allclose(r[key], o[key], rtol=10 * tol, atol=1e-12), key

    _lib.debug_set_xprod_waves(waves)
    try:
        r = nnlm_amd.c_nnmf(*args)
    finally:
        _lib.debug_set_xprod_waves(0)
    check(r, r["W"], r["H"])
    with handle(waves) as h:
        h.set_matrix(A)
        h.set_factors(k, W0, H0)
        t = h.run(z, z, 3, -1.0, 0, False, 50, 1e-9, 1, 2)
        Wn, Hn = h.get_factors()
        assert int(h.get_info("xprod_waves_h")) == waves and int(h.get_info("xprod_waves_w")) == waves
        assert int(h.get_info("xprod_splits_err")) >= 1  # the fused kernel ran
    check(t, Wn, Hn)


@pytest.mark.parametrize("waves", [8, 10])
def test_plain_and_fused_w_launches_with_different_slab_counts_share_the_slabs(monkeypatch, waves):
    """The plain W launch is planned on the handle's CU count, the fused one on the device's: with the handle told of 4 compute units,
    300 x 1100 (18 stages, 4 tiles) runs the plain launch with one slab and the fused launch with more, alternating on one buffer that
    factors_alloc sized for the larger of the two plans."""
    rng = np.random.default_rng(77)
    n, m, k = 300, 1100, 11
    A = rng.random((n, m))
    W0, H0 = 0.01 * rng.random((n, k)), 0.01 * rng.random((k, m))
    z = [0.0, 0.0, 0.0]
    tol = 1e-4
    o = ref.c_nnmf(A, k, W0, H0, None, None, z, z, 3, -1.0, 1, 0, False, 50, 1e-9, 1, 2)
    _lib.debug_set_cus(4)
    try:
        h = handle(waves)
    finally:
        _lib.debug_set_cus(0)
    with h:
        h.set_matrix(A)
        h.set_factors(k, W0, H0)
        t = h.run(z, z, 3, -1.0, 0, False, 50, 1e-9, 1, 2)
        Wn, Hn = h.get_factors()
        plain, fused = int(h.get_info("xprod_splits_w")), int(h.get_info("xprod_splits_err"))
        assert int(h.get_info("xprod_waves_w")) == waves
        assert plain == _lib.xprod_plan(512, 18, k, 4, waves)["splits"] == 1
        print(f"waves={waves} slabs: plain {plain}, fused {fused}")
        assert fused >= plain  # (2 on a 256-CU device)
    assert relF(Wn, o["W"]) < tol and relF(Hn, o["H"]) < tol
    for key in ("mse_error", "mkl_error", "target_error"):
        assert np.allclose(t[key], o[key], rtol=10 * tol, atol=1e-12), key
