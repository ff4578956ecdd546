"""Batched factorisation (nnlm_set_factors_batch / nnlm_run_batch / nnlm_c_nnmf_batch, api.nnmf_batch) on the MI355X: every member
against the fp64 oracle run with that member's init, against the same member run alone, independent of its neighbours, with its own
stopping rule; the refusals; one pass over A per trace iteration.  Run with `pytest -m gpu`.

Bounds: strict fp64 mode 1e-10 with equal iteration and sweep counts; fp32-operand mode 1e-4 (the solo path's own bound)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import relF  # noqa: E402
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402
from oracle import ref  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = [("f64", _lib.PREC_F64, 1e-10), ("f32", _lib.PREC_F32, 1e-4)]
ERR_ARG, ERR_UNSUPPORTED = 1, 5
Z3 = [0.0, 0.0, 0.0]


@pytest.fixture(autouse=True)
def _default_precision(monkeypatch):
    monkeypatch.delenv("NNLM_PRECISION", raising=False)


def problem(n, m, ks, seed):
    """A full-rank matrix with a rank-6 component (well conditioned up to rank 64: a rank-6 matrix plus little noise makes the SCD
    chain at high rank amplify rounding differences of ANY two implementations, the solo path against the oracle included)."""
    rng = np.random.default_rng(seed)
    r = 6
    A = rng.random((n, m)) + 0.5 * rng.random((n, r)) @ rng.random((r, m))
    inits = [(rng.random((n, k)), rng.random((k, m))) for k in ks]
    return A, inits


def oracle(A, k, W, H, alpha, beta, max_iter, rel_tol, method, trace, inner=50, itol=1e-9):
    return ref.c_nnmf(A, k, W, H, None, None, alpha, beta, max_iter, rel_tol, 1, 0, True, inner, itol, method, trace)


def batch(prec, A, ks, inits, alpha, beta, max_iter, rel_tol, method, trace, inner=50, itol=1e-9, cus=0, prof=False):
    if cus:
        _lib.debug_set_cus(cus)
    try:
        h = nnlm_amd.Handle(0, prec)
    finally:
        _lib.debug_set_cus(0)
    with h:
        h.set_matrix(A)
        h.set_factors_batch(ks, [w for w, _ in inits], [x for _, x in inits])
        if prof:
            h.profile_enable(True)
        t = h.run_batch(alpha, beta, max_iter, rel_tol, 0, True, inner, itol, method, trace)
        f = h.get_factors_batch()
        info = {key: h.get_info(key) for key in ("sweep_form_w", "sweep_form_h")}
        if prof:
            info["prof"] = {nm: h.profile_get(nm) for nm in ("xprod_h", "xprod_w", "batch_errors", "errors", "sweep_w", "gram")}
    for o, (W, H) in zip(t, f):
        o["W"], o["H"] = W, H
    return t, info


def solo(prec, A, k, W, H, alpha, beta, max_iter, rel_tol, method, trace, inner=50, itol=1e-9, cus=0):
    if cus:
        _lib.debug_set_cus(cus)
    try:
        h = nnlm_amd.Handle(0, prec)
    finally:
        _lib.debug_set_cus(0)
    with h:
        h.set_matrix(A)
        h.set_factors(k, W, H)
        t = h.run(alpha, beta, max_iter, rel_tol, 0, True, inner, itol, method, trace)
        t["W"], t["H"] = h.get_factors()
    return t


def check_member(o, r, tol, strict, traces=True, solo_run=None):
    """o = batch member, r = reference run.  fp32-operand mode with solo_run: the bound is the solo fp32 path's own distance to r
    (at least tol) -- the member must be no further from the oracle than the same member run alone."""
    if solo_run is not None and not strict:
        tol = max(tol, 1.01 * relF(solo_run["W"], r["W"]), 1.01 * relF(solo_run["H"], r["H"]))
    assert relF(o["W"], r["W"]) < tol and relF(o["H"], r["H"]) < tol, (relF(o["W"], r["W"]), relF(o["H"], r["H"]), tol)
    assert o["n_iteration"] == r["n_iteration"] and len(o["mse_error"]) == len(r["mse_error"])
    if strict:
        assert np.array_equal(o["average_epoch"], r["average_epoch"]), (o["average_epoch"], r["average_epoch"])
        if traces:
            for key in ("mse_error", "target_error", "mkl_error"):
                assert relF(o[key], r[key]) < tol, (key, relF(o[key], r[key]))


@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("ks", [[5], [1, 4, 7], [1, 4, 7, 16, 3, 2, 8, 6]])
def test_member_equals_oracle_and_solo_run(pname, prec, tol, method, ks):
    A, inits = problem(150, 110, ks, 11 * len(ks) + method)
    t, _ = batch(prec, A, ks, inits, Z3, Z3, 12, -1.0, method, 3)
    for b, k in enumerate(ks):
        o = oracle(A, k, *inits[b], Z3, Z3, 12, -1.0, method, 3)
        s = solo(prec, A, k, *inits[b], Z3, Z3, 12, -1.0, method, 3)
        check_member(t[b], o, tol, pname == "f64", solo_run=s)
        check_member(t[b], s, tol if pname == "f64" else 1e-5, pname == "f64")


@pytest.mark.parametrize("pname,prec,tol", MODES)
def test_penalties_in_all_three_positions(pname, prec, tol):
    """L2, angle and L1 on both factors: a cross-member Gram block reaching a solver (the angle term touches every entry of G) would
    move every member away from the oracle."""
    ks = [3, 5, 2, 6]
    alpha, beta = [0.1, 0.05, 0.02], [0.2, 0.1, 0.03]
    A, inits = problem(140, 100, ks, 5)
    for method in (1, 2):
        t, _ = batch(prec, A, ks, inits, alpha, beta, 10, -1.0, method, 2)
        for b, k in enumerate(ks):
            s = solo(prec, A, k, *inits[b], alpha, beta, 10, -1.0, method, 2)
            check_member(t[b], oracle(A, k, *inits[b], alpha, beta, 10, -1.0, method, 2), tol, pname == "f64", solo_run=s)
            check_member(t[b], s, tol if pname == "f64" else 1e-5, pname == "f64")


@pytest.mark.parametrize("pname,prec,tol", MODES)
def test_independence_of_members(pname, prec, tol):
    """Permuting the members or adding one leaves every other member's result unchanged: factors, traces and sweep counts bit for bit
    (strict) / factors within 1e-6 (fp32)."""
    ks = [4, 7, 1, 9]
    A, inits = problem(160, 120, ks + [12], 8)
    base, _ = batch(prec, A, ks, inits[:4], Z3, Z3, 10, -1.0, 1, 2)
    perm = [2, 0, 3, 1]
    tp, _ = batch(prec, A, [ks[p] for p in perm], [inits[p] for p in perm], Z3, Z3, 10, -1.0, 1, 2)
    ta, _ = batch(prec, A, ks + [12], inits, Z3, Z3, 10, -1.0, 1, 2)
    for b in range(4):
        for other in (tp[perm.index(b)], ta[b]):
            for key in ("W", "H"):
                if pname == "f64":
                    assert np.array_equal(other[key], base[b][key]), (b, key, relF(other[key], base[b][key]))
                else:
                    assert relF(other[key], base[b][key]) < 1e-6, (b, key, relF(other[key], base[b][key]))
            assert other["n_iteration"] == base[b]["n_iteration"]
            if pname == "f64":
                assert np.array_equal(other["average_epoch"], base[b]["average_epoch"])
                for key in ("mse_error", "mkl_error", "target_error"):
                    assert np.array_equal(other[key], base[b][key]), (b, key)


@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("trace", [1, 3])
def test_each_member_stops_on_its_own_rule(pname, prec, tol, trace):
    ks = [2, 6, 3, 10, 1]
    A, inits = problem(130, 90, ks, 21)
    inits = [(w * s, x * s) for (w, x), s in zip(inits, [1.0, 0.02, 3.0, 0.3, 0.01])]
    t, _ = batch(prec, A, ks, inits, Z3, Z3, 300, 1e-4, 1, trace)
    its = set()
    for b, k in enumerate(ks):
        s = solo(prec, A, k, *inits[b], Z3, Z3, 300, 1e-4, 1, trace)
        assert t[b]["n_iteration"] == s["n_iteration"] and len(t[b]["target_error"]) == len(s["target_error"])
        assert t[b]["warning"] == s["warning"]
        # (the solo run stopped there: equal factors show that the frozen member did not move afterwards)
        check_member(t[b], s, tol, pname == "f64")
        if pname == "f64":
            check_member(t[b], oracle(A, k, *inits[b], Z3, Z3, 300, 1e-4, 1, trace), tol, True)
        its.add(t[b]["n_iteration"])
    assert len(its) >= 2, its


def test_warning_per_member():
    ks = [2, 5]
    A, inits = problem(100, 80, ks, 3)
    t, _ = batch(_lib.PREC_F64, A, ks, inits, Z3, Z3, 4, 1e-12, 1, 1)
    for b, k in enumerate(ks):
        o = oracle(A, k, *inits[b], Z3, Z3, 4, 1e-12, 1, 1)
        assert t[b]["warning"] == bool(o["warning"]) is True


@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("ks", [[1], [64], [16, 16, 16, 16], [30, 1, 33], [16, 1], [1, 16], [8, 9]])
def test_edges(pname, prec, tol, ks):
    """rank 1, a rank sum of exactly 64, and the K-padding boundaries 16 | 17."""
    A, inits = problem(180, 140, ks, sum(ks))
    t, _ = batch(prec, A, ks, inits, Z3, [0.01, 0, 0], 6, -1.0, 1, 2)
    for b, k in enumerate(ks):
        s = solo(prec, A, k, *inits[b], Z3, [0.01, 0, 0], 6, -1.0, 1, 2)
        check_member(t[b], oracle(A, k, *inits[b], Z3, [0.01, 0, 0], 6, -1.0, 1, 2), tol, pname == "f64", solo_run=s)
        check_member(t[b], s, tol if pname == "f64" else 1e-5, pname == "f64")


@pytest.mark.parametrize("cus", [0, 1])
def test_fp32_sweep_forms(cus):
    """fp32-operand mode: the row form of the sweep (few columns: k_sweep_r.h) and, on a device that "has" one CU, the matrix-pipe form
    (k_sweep_f.h) -- both on member row blocks."""
    ks = [3, 12, 5]
    A, inits = problem(300, 200, ks, 9)
    t, info = batch(_lib.PREC_F32, A, ks, inits, [0.01, 0.002, 0.003], Z3, 6, -1.0, 1, 2, cus=cus)
    assert int(info["sweep_form_w"]) == (3 if cus == 0 else 2) and int(info["sweep_form_h"]) == (3 if cus == 0 else 2), info
    for b, k in enumerate(ks):
        s = solo(_lib.PREC_F32, A, k, *inits[b], [0.01, 0.002, 0.003], Z3, 6, -1.0, 1, 2, cus=cus)  # (the same sweep form)
        check_member(t[b], oracle(A, k, *inits[b], [0.01, 0.002, 0.003], Z3, 6, -1.0, 1, 2), 1e-4, False, solo_run=s)
        check_member(t[b], s, 1e-5, False)


@pytest.mark.parametrize("pname,prec,tol", MODES)
def test_one_pass_over_A_per_trace_iteration(pname, prec, tol):
    ks = [8] * 8
    A, inits = problem(200, 150, ks, 4)
    t, info = batch(prec, A, ks, inits, Z3, Z3, 6, -1.0, 1, 2, prof=True)
    p = info["prof"]
    ntr = len(t[0]["mse_error"])
    assert ntr == 4  # iterations 0, 2, 4 and the last (src/nnmf.cpp:164)
    assert p["batch_errors"][1] == ntr and p["errors"][1] == 0, p
    assert p["xprod_h"][1] == 6 and p["xprod_w"][1] == 6, p
    assert p["sweep_w"][1] == 6 * 8 and p["gram"][1] == 2 * 6 * 8, p


def test_one_shot_entry_and_api(monkeypatch):
    """nnlm_c_nnmf_batch through api.nnmf_batch: member b = nnmf() with the generator in the state member b found it; best = argmin."""
    rng = np.random.default_rng(2)
    A = rng.random((90, 6)) @ rng.random((6, 70)) + 0.05 * rng.random((90, 70))
    res, best = api.nnmf_batch(A, [2, 4], nrun=2, rng=np.random.default_rng(17), max_iter=40, rel_tol=1e-6, alpha=[0.01, 0, 0])
    assert len(res) == 4
    g = np.random.default_rng(17)
    for b, k in enumerate([2, 2, 4, 4]):
        solo_res = api.nnmf(A, k, rng=g, max_iter=40, rel_tol=1e-6, alpha=[0.01, 0, 0])
        assert relF(res[b]["W"], solo_res["W"]) < 1e-10 and relF(res[b]["H"], solo_res["H"]) < 1e-10
        assert res[b]["n_iteration"] == solo_res["n_iteration"]
        assert np.array_equal(res[b]["average_epochs"], solo_res["average_epochs"])
        assert relF(res[b]["target_loss"], solo_res["target_loss"]) < 1e-10
    assert best == int(np.argmin([r["target_loss"][-1] for r in res]))
    # the library's default init (W_init = H_init = NULL) is the solo entry's, member by member
    out = _lib.c_nnmf_batch(A, [3], None, None, Z3, Z3, 5, -1.0, 1, 0, True, 50, 1e-9, 1, 1)
    o1 = _lib.c_nnmf(A, 3, None, None, None, None, Z3, Z3, 5, -1.0, 1, 0, True, 50, 1e-9, 1, 1)
    assert relF(out[0]["W"], o1["W"]) < 1e-10 and out[0]["n_iteration"] == o1["n_iteration"]


def test_refusals():
    rng = np.random.default_rng(0)
    A = rng.random((60, 50))
    W, H = [rng.random((60, 2)), rng.random((60, 3))], [rng.random((2, 50)), rng.random((3, 50))]

    def code(fn):
        with pytest.raises(_lib.NnlmError) as e:
            fn()
        return e.value.code

    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
        h.set_matrix(A)
        h.set_factors_batch([2, 3], W, H)
        for method in (3, 4):  # KL loss
            assert code(lambda: h.run_batch(Z3, Z3, 3, -1.0, 0, True, 1, 1e-9, method, 1)) == ERR_UNSUPPORTED
        assert code(lambda: h.set_factors_batch([33, 32])) == ERR_UNSUPPORTED  # rank sum 65
        h.set_factors_batch([33, 31])  # 64 is accepted
        lib = _lib.load()
        for ks in ([0], [2, 0]):  # bad rank list at the C ABI itself
            arr = np.array(ks, dtype=np.uint32)
            assert lib.nnlm_set_factors_batch(h._h, len(ks), arr.ctypes.data_as(C.POINTER(C.c_uint)), None, None) == ERR_ARG
        arr = np.ones(65, dtype=np.uint32)
        assert lib.nnlm_set_factors_batch(h._h, 65, arr.ctypes.data_as(C.POINTER(C.c_uint)), None, None) == ERR_ARG
        assert lib.nnlm_set_factors_batch(h._h, 0, arr.ctypes.data_as(C.POINTER(C.c_uint)), None, None) == ERR_ARG
        h.set_factors(2, W[0], H[0])  # a solo set ends the batch
        assert code(lambda: h.run_batch(Z3, Z3, 3, -1.0, 0, True, 50, 1e-9, 1, 1)) == ERR_ARG
    An = A.copy()
    An[5, 7] = np.nan
    Ai = A.copy()
    Ai[0, 0] = -np.inf
    for bad in (An, Ai):  # NA / Inf in A
        with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
            h.set_matrix(bad)
            assert code(lambda: h.set_factors_batch([2, 3], W, H)) == ERR_UNSUPPORTED
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:  # sparse A
        cols, rows = np.nonzero(A.T)
        ptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=50))])
        h.set_matrix_csc(ptr, rows, A[rows, cols], A.shape)
        assert code(lambda: h.set_factors_batch([2, 3], W, H)) == ERR_UNSUPPORTED
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:  # a communicator (virtual rank)
        h.set_matrix(A)
        h.comm_init(None, 0, 2)
        assert code(lambda: h.set_factors_batch([2, 3], W, H)) == ERR_UNSUPPORTED
    # one-shot entry: KL and the rank sum; masks and known profiles have no place in the C call and are refused by api.nnmf_batch
    assert code(lambda: _lib.c_nnmf_batch(A, [2, 3], W, H, Z3, Z3, 3, -1.0, 1, 0, True, 1, 1e-9, 3, 1)) == ERR_UNSUPPORTED
    assert code(lambda: _lib.c_nnmf_batch(A, [40, 25], None, None, Z3, Z3, 3, -1.0, 1, 0, True, 1, 1e-9, 1, 1)) == ERR_UNSUPPORTED
    assert code(lambda: _lib.c_nnmf_batch(A, [2, 3], W[::-1], H, Z3, Z3, 3, -1.0, 1, 0, True, 1, 1e-9, 1, 1)) == ERR_ARG
    assert code(lambda: api.nnmf_batch(A, [2, 3], mask={"H": np.zeros((2, 50), dtype=bool)})) == ERR_UNSUPPORTED
    assert code(lambda: api.nnmf_batch(A, [2, 3], init=[{"W0": np.ones((60, 1))}, {}])) == ERR_UNSUPPORTED
