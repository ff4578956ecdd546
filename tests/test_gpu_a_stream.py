"""Cache policy of the stream of A in the three A-streaming cross products (xprod16_tn_kernel, xprod16_err_kernel, xprod_tn_kernel<double>):
the requests for A of the contraction stages >= nt_from_stage are non-temporal (nnlm_debug_set_a_stream; glds16_s_nt in k_xprod.h).

A cache policy cannot change a value, so every assertion here is BIT IDENTITY against the default-policy run (hook = INT_MAX).  What that
guards is the edit: the second copy of each request loop, the operands of the new instruction, and the branch on the GLOBAL stage index
where a slab begins.  A case is three outer iterations with trace = 1 -- the fused kernel runs in iterations 1 and 2, the plain kernels
in iteration 0 and on the H side -- once per hook value, each on a fresh handle."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import err_cases as ec  # noqa: E402
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = _lib.A_STREAM_NONE  # INT_MAX: today's behaviour
F32, F64 = _lib.PREC_F32, _lib.PREC_F64
Z = [0.0, 0.0, 0.0]
TRACES = ("mse_error", "mkl_error", "target_error", "average_epoch")


@pytest.fixture(autouse=True)
def _default_precision(monkeypatch):
    monkeypatch.delenv("NNLM_PRECISION", raising=False)


def handle(prec, nt_from, waves=0):
    _lib.debug_set_a_stream(nt_from)
    _lib.debug_set_xprod_waves(waves)
    try:
        return nnlm_amd.Handle(0, prec)
    finally:
        _lib.debug_set_xprod_waves(0)
        _lib.debug_set_a_stream(-1)


def run3(prec, nt_from, A, W0, H0, waves=0):
    """(W, H, traces, a_stream_nt_from, xprod_splits_err) of three iterations, trace = 1, SCD."""
    with handle(prec, nt_from, waves) as h:
        h.set_matrix(A)
        h.set_factors(W0.shape[1], W0, H0)
        t = h.run(Z, Z, 3, -1.0, 0, False, 50, 1e-9, 1, 1)
        W, H = h.get_factors()
        used, fused = int(h.get_info("a_stream_nt_from")), int(h.get_info("xprod_splits_err"))
    assert t["n_iteration"] == 3
    return W, H, t, used, fused


def same_bits(got, want, what):
    for a, b, name in ((got[0], want[0], "W"), (got[1], want[1], "H")):
        assert np.array_equal(a, b), (what, name)
    for key in TRACES:
        assert got[2][key].shape == want[2][key].shape and np.array_equal(got[2][key], want[2][key]), (what, key)


def check_values(prec, A, W0, H0, values, waves=0, fused=True):
    base = run3(prec, NONE, A, W0, H0, waves)
    assert base[3] == NONE
    assert np.isfinite(base[0]).all() and np.isfinite(base[1]).all() and np.isfinite(base[2]["mse_error"]).all()
    assert (base[4] >= 1) == fused  # (the fused kernel exists in the fp32-operand mode only)
    for v in values:
        got = run3(prec, v, A, W0, H0, waves)
        assert got[3] == v, (v, got[3])
        assert (got[4] >= 1) == fused
        same_bits(got, base, f"nt_from_stage={v}")
    return base


def factors(rng, n, m, k):
    return 0.01 * rng.random((n, k)), 0.01 * rng.random((k, m))


@pytest.fixture(scope="module")
def ragged():
    """700 x 300 pads to 768 x 384: the last 160-column tile has dead wavefronts on both sides (tests/test_gpu_xprod_blocks.py)."""
    return np.random.default_rng(355).random((700, 300))


@pytest.mark.parametrize("k", [3, 33, 50, 64])  # NKQ = 1; NKQ = 3 untrimmed; 13 factor pieces; NKQ = 4 untrimmed
def test_every_rank_form(ragged, k):
    A = ragged
    W0, H0 = factors(np.random.default_rng(k), 700, 300, k)
    check_values(F32, A, W0, H0, (0, 1, 2))


@pytest.mark.parametrize("waves", [8, 10])
def test_both_block_widths(ragged, waves):
    A = ragged
    W0, H0 = factors(np.random.default_rng(50 + waves), 700, 300, 50)
    with handle(F32, 0, waves) as h:  # (the width that runs is the one asked for)
        h.set_matrix(A)
        h.set_factors(50, W0, H0)
        h.iterate(1, Z, Z, 50, 1e-9, 1)
        assert int(h.get_info("xprod_waves_h")) == waves and int(h.get_info("xprod_waves_w")) == waves
        assert int(h.get_info("a_stream_nt_from")) == 0
    check_values(F32, A, W0, H0, (0, 1, 2), waves=waves)


def test_missing_entries(ragged):
    """10 % NaN: the HAS_MISS instantiation of the fused kernel."""
    A = ragged
    rng = np.random.default_rng(10)
    A = A.copy()
    A[rng.random(A.shape) < 0.1] = np.nan
    W0, H0 = factors(rng, 700, 300, 50)
    check_values(F32, A, W0, H0, (0, 1, 2))


@pytest.mark.parametrize("k", [50, 64])  # strict kernel: 48 + 2 tail rows; four whole tiles
def test_strict_mode(ragged, k):
    A = ragged
    W0, H0 = factors(np.random.default_rng(64 + k), 700, 300, k)
    check_values(F64, A, W0, H0, (0, 1, 2), fused=False)


def test_slab_boundaries():
    """64 x m with m large enough for the fused kernel's plan to cut the contraction into slabs: block (x, 1) begins at the GLOBAL stage
    stages_per_split, so nt_from_stage at that stage and beside it puts the switch at the end of slab 0, at the first stage of slab 1
    and one stage into it.  The same three values around the plain W launch's boundary, where its plan differs."""
    k = 50
    with nnlm_amd.Handle(0, F32) as h:
        cus = int(h.get_info("cus"))

    def plans(n, m):
        npad, mpad = ec.pads(n, m)
        return _lib.xprod_plan(npad, mpad // 64, k, cus, 8), _lib.xprod_plan(npad, mpad // 64, k, cus, 0)

    shapes = [(n, m) for n, m in ((64, 1100), (64, 2100), (64, 4200), (64, 8300)) if plans(n, m)[0]["splits"] > 1]
    assert shapes, "no candidate shape is planned with more than one slab"
    n, m = shapes[0]
    fused, plain = plans(n, m)
    values = {0, 1, 2}
    for p in (fused, plain):
        if p["splits"] > 1:
            values |= {p["stages_per_split"] - 1, p["stages_per_split"], p["stages_per_split"] + 1}
    rng = np.random.default_rng(1100)
    A = rng.random((n, m))
    W0, H0 = factors(rng, n, m, k)
    with handle(F32, fused["stages_per_split"]) as h:  # (the plan asked about is the one that runs)
        h.set_matrix(A)
        h.set_factors(k, W0, H0)
        h.run(Z, Z, 3, -1.0, 0, False, 50, 1e-9, 1, 1)
        assert int(h.get_info("xprod_splits_err")) == fused["splits"]
    print(f"A_STREAM {n}x{m}: fused slabs {fused['splits']} x {fused['stages_per_split']} stages, values {sorted(values)}")
    check_values(F32, A, W0, H0, sorted(values))


def test_library_choice_is_the_reported_constant(ragged):
    """A default handle (hook -1) reports the library's own choice and gives the bits of a handle that was told that value.  At this size a
    pass over A fits the Infinity Cache many times over, and the library's choice for such a pass is the default policy."""
    A = ragged
    W0, H0 = factors(np.random.default_rng(7), 700, 300, 50)
    auto = run3(F32, -1, A, W0, H0)
    assert auto[3] == NONE and auto[4] >= 1
    told = run3(F32, auto[3], A, W0, H0)
    assert told[3] == auto[3]
    same_bits(auto, told, "library's choice")
    with nnlm_amd.Handle(0, F32) as h:
        assert int(h.get_info("a_stream_nt_from")) == -1  # (no cross product yet)
