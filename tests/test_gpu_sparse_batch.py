"""Batched factorisation on a sparse A (nnlm_set_matrix_csc_batch + the batch entries, nnlm_c_nnmf_csc_batch,
api.nnmf_batch(sparse_batch=True)) on the MI355X: every member against the fp64 oracle on the densified matrix and against the same
member run alone on the sparse path, independent of its neighbours, with its own stopping rule; the edges of the stack and of the
pattern; one SpMM per half-step and one walk over the non-zeros per trace iteration; the door.  Run with `pytest -m gpu`.

Bounds (those of test_gpu_batch.py and test_gpu_sparse.py): strict fp64 mode 1e-10 with equal iteration and sweep counts; fp32-operand
mode 1e-4 against the oracle, widened to 1.01 x the solo fp32 run's own distance; fp32 batch against fp32 solo 1e-5, against another
fp32 batch 1e-6."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import relF  # noqa: E402
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402
from oracle import ref  # noqa: E402
import sparse_cases as sc  # noqa: E402
import sparse_batch_cases as sbc  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = [("f64", _lib.PREC_F64, 1e-10), ("f32", _lib.PREC_F32, 1e-4)]
ERR_ARG, ERR_UNSUPPORTED = 1, 5
Z3 = [0.0, 0.0, 0.0]
PROF = ("spmm_h", "spmm_w", "sp_batch_errors", "sp_errors", "batch_errors", "errors", "xprod_h", "xprod_w", "sweep_w", "gram")


@pytest.fixture(autouse=True)
def _default_precision(monkeypatch):
    monkeypatch.delenv("NNLM_PRECISION", raising=False)


def handle(prec, cus=0):
    if cus:
        _lib.debug_set_cus(cus)
    try:
        return nnlm_amd.Handle(0, prec)
    finally:
        _lib.debug_set_cus(0)


def oracle(A, k, W, H, alpha, beta, max_iter, rel_tol, method, trace, inner=50):
    return ref.c_nnmf(A, k, W, H, None, None, alpha, beta, max_iter, rel_tol, 1, 0, True, inner, 1e-9, method, trace)


def batch(prec, S, ks, inits, alpha, beta, max_iter, rel_tol, method, trace, inner=50, cus=0, prof=False):
    with handle(prec, cus) as h:
        h.set_matrix_csc_batch(*S)
        h.set_factors_batch(ks, [w for w, _ in inits], [x for _, x in inits])
        if prof:
            h.profile_enable(True)
        t = h.run_batch(alpha, beta, max_iter, rel_tol, 0, True, inner, 1e-9, method, trace)
        f = h.get_factors_batch()
        info = {"waves": int(h.get_info("sp_batch_waves"))}
        if prof:
            info["prof"] = {nm: h.profile_get(nm) for nm in PROF}
    for o, (W, H) in zip(t, f):
        o["W"], o["H"] = W, H
    return t, info


def solo(prec, S, k, W, H, alpha, beta, max_iter, rel_tol, method, trace, inner=50, cus=0, door=False):
    with handle(prec, cus) as h:
        h.set_matrix_csc_batch(*S) if door else h.set_matrix_csc(*S)
        h.set_factors(k, W, H)
        t = h.run(alpha, beta, max_iter, rel_tol, 0, True, inner, 1e-9, method, trace)
        t["W"], t["H"] = h.get_factors()
    return t


def dist(a, b):
    """relF, absolute where the reference is (close to) zero (sparse_cases.err: a factor of a matrix of zeros)."""
    return sc.err(a, b)


def check_member(o, r, tol, strict, traces=True, solo_run=None):
    """check_member of test_gpu_batch.py.  o = batch member, r = reference run; fp32-operand mode with solo_run: the bound is the solo
    fp32 path's own distance to r (at least tol).
    mkl_error: the error block of a sparse A leaves out the zeros' -eps ln(wh + eps), at most 3.7e-15 per entry of the mean (the contract
    of nnlm_set_matrix_csc; test_gpu_sparse.py bounds the same comparison by 1e-10 |ref| + 4e-15).  Where the trace itself is that
    small -- A = 0: the oracle's mkl is 1.6e-28; a 33 x 1 matrix: 1.5e-5, of which 1.8e-15 is 1.2e-10 -- the relative bound means
    nothing, and that absolute term decides, as it does there."""
    if solo_run is not None and not strict:
        tol = max(tol, 1.01 * dist(solo_run["W"], r["W"]), 1.01 * dist(solo_run["H"], r["H"]))
    print("member: W %.3e H %.3e (bound %.3g)" % (dist(o["W"], r["W"]), dist(o["H"], r["H"]), tol))
    assert dist(o["W"], r["W"]) < tol and dist(o["H"], r["H"]) < tol, (dist(o["W"], r["W"]), dist(o["H"], r["H"]), tol)
    assert o["n_iteration"] == r["n_iteration"] and len(o["mse_error"]) == len(r["mse_error"])
    if strict:
        assert np.array_equal(o["average_epoch"], r["average_epoch"]), (o["average_epoch"], r["average_epoch"])
        if traces:
            for key in ("mse_error", "target_error", "mkl_error"):
                gap = float(np.max(np.abs(np.asarray(o[key]) - np.asarray(r[key])), initial=0.0))
                print("  %s %.3e (largest gap %.3e)" % (key, relF(o[key], r[key]), gap))
                assert relF(o[key], r[key]) < tol or (key == "mkl_error" and gap <= 4e-15), (key, relF(o[key], r[key]), gap)


def check_batch(pname, prec, tol, S, ks, inits, alpha, beta, max_iter, rel_tol, method, trace, inner=50, cus=0):
    """Every member against the oracle on the densified matrix and against c_nnmf_csc's path run alone from the same init."""
    A = sc.densify(S, "zero")
    t, info = batch(prec, S, ks, inits, alpha, beta, max_iter, rel_tol, method, trace, inner, cus=cus)
    for b, k in enumerate(ks):
        o = oracle(A, k, *inits[b], alpha, beta, max_iter, rel_tol, method, trace, inner)
        s = solo(prec, S, k, *inits[b], alpha, beta, max_iter, rel_tol, method, trace, inner, cus=cus)
        check_member(t[b], o, tol, pname == "f64", solo_run=s)
        check_member(t[b], s, tol if pname == "f64" else 1e-5, pname == "f64")
    return t, info


# ---- 1. member = oracle = solo sparse run ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("density", [0.01, 0.2, 1.0])
@pytest.mark.parametrize("ks", [[5], [1, 4, 7], [1, 4, 7, 16, 3, 2, 8, 6]])
def test_member_equals_oracle_and_solo_sparse_run(pname, prec, tol, method, density, ks):
    S, inits = sbc.thinned(150, 110, density, ks, 11 * len(ks) + method + int(100 * density))
    alpha, beta = sbc.l1_where_lines_are_empty(S, Z3, Z3)
    check_batch(pname, prec, tol, S, ks, inits, alpha, beta, 12, -1.0, method, 3)


# ---- 2. edges of the stack ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("ks", [[1], [64], [16, 16, 16, 16], [30, 1, 33], [16, 1], [1, 16], [8, 9]])
def test_edges_of_the_stack(pname, prec, tol, method, ks):
    """Member blocks that start on, end on and straddle 16-row boundaries; the SpMM's three lane widths (KP = 16, 32, 64)."""
    S, inits = sbc.thinned(180, 140, 0.2, ks, sum(ks) + method)
    check_batch(pname, prec, tol, S, ks, inits, Z3, [0.01, 0, 0], 6, -1.0, method, 2)


# ---- 3. edges of the pattern -------------------------------------------------------------------------------------------------------------
EDGES = sbc.pattern_edges()


@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("case", range(len(EDGES)), ids=[e[0] for e in EDGES])
def test_edges_of_the_pattern(pname, prec, tol, method, case):
    name, S, ks = EDGES[case]
    n, m = S[3]
    rng = np.random.default_rng(7 + case)
    inits = [(rng.random((n, k)), rng.random((k, m))) for k in ks]
    alpha, beta = sbc.l1_where_lines_are_empty(S, [0.01, 0, 0], [0.01, 0, 0])
    t, info = check_batch(pname, prec, tol, S, ks, inits, alpha, beta, 5, -1.0, method, 2, inner=5)
    assert info["waves"] == sbc.spb_waves(S[1].size)
    for o in t:
        assert np.all(np.isfinite(o["mse_error"])) and np.all(np.isfinite(o["mkl_error"]))


FAMILY = sbc.family_cases()
BOUNDARY = sbc.boundary_batch_cases()


def run_case(pname, prec, tol, c, method, cus=0):
    """(both methods on every case: the case's own choice of method is not used)"""
    return check_batch(pname, prec, tol, c["S"], c["ks"], c["inits"], c["alpha"], c["beta"], c["max_iter"], -1.0, method, c["trace"],
                       inner=c["inner"], cus=cus)


@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("case", range(len(FAMILY)), ids=[c["name"] for c in FAMILY])
def test_pattern_families(pname, prec, tol, method, case):
    run_case(pname, prec, tol, FAMILY[case], method)


@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("case", range(len(BOUNDARY)), ids=[c["name"] for c in BOUNDARY])
def test_boundary_family_as_batches(pname, prec, tol, method, case):
    """Columns, heads and empty runs exactly on the SpMM's worker boundaries at the stacked rank (test_sparse_batch_host.py shows
    which events each case hits)."""
    run_case(pname, prec, tol, BOUNDARY[case], method)


@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [1, 2])
def test_other_worker_counts(pname, prec, tol, method):
    """nnlm_debug_set_cus reaches the split of the error kernel: 1 and 3 compute units cap it at 16 and 48 wavefronts."""
    rng = np.random.default_rng(31)
    P = sc._powerlaw(400, 400, rng, by_rows=False)  # (more than 48 x 256 non-zeros: the three counts differ)
    S = sc.csc_from_pattern(P, sbc.values(400, 400, rng))
    ks = [3, 6, 2]
    inits = [(rng.random((400, k)), rng.random((k, 400))) for k in ks]
    alpha, beta = sbc.l1_where_lines_are_empty(S, Z3, Z3)
    waves = []
    for cus in (0, 1, 3):
        _, info = check_batch(pname, prec, tol, S, ks, inits, alpha, beta, 4, -1.0, method, 2, inner=5, cus=cus)
        waves.append(info["waves"])
    nnz = S[1].size
    assert waves == [sbc.spb_waves(nnz), 16, 48] and len(set(waves)) == 3, (nnz, waves)


# ---- 4. independence ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [1, 2])
def test_independence_of_members(pname, prec, tol, method):
    """Permuting the members, or adding one that leaves the stacked padded rank at 32, leaves every member bit-identical (strict);
    adding one that makes it 48 changes the SpMM's worker split: 1e-10.  fp32: 1e-6 throughout."""
    ks = [4, 7, 1, 9]
    S, inits = sbc.thinned(160, 120, 0.2, ks + [5, 12], 8)
    strict = pname == "f64"
    base, _ = batch(prec, S, ks, inits[:4], Z3, Z3, 10, -1.0, method, 2)
    perm = [2, 0, 3, 1]
    tp, _ = batch(prec, S, [ks[p] for p in perm], [inits[p] for p in perm], Z3, Z3, 10, -1.0, method, 2)
    t5, _ = batch(prec, S, ks + [5], inits[:5], Z3, Z3, 10, -1.0, method, 2)
    t12, _ = batch(prec, S, ks + [12], inits[:4] + [inits[5]], Z3, Z3, 10, -1.0, method, 2)
    for b in range(4):
        for other, same_bits in ((tp[perm.index(b)], True), (t5[b], True), (t12[b], False)):
            exact = strict and same_bits
            for key in ("W", "H"):
                if exact:
                    assert np.array_equal(other[key], base[b][key]), (b, key, relF(other[key], base[b][key]))
                else:
                    assert relF(other[key], base[b][key]) < (1e-10 if strict else 1e-6), (b, key, relF(other[key], base[b][key]))
            assert other["n_iteration"] == base[b]["n_iteration"]
            if strict:
                assert np.array_equal(other["average_epoch"], base[b]["average_epoch"])
                for key in ("mse_error", "mkl_error", "target_error"):
                    if exact:
                        assert np.array_equal(other[key], base[b][key]), (b, key)
                    else:
                        assert relF(other[key], base[b][key]) < 1e-10, (b, key)


# ---- 5. penalties ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [1, 2])
def test_penalties_in_all_three_positions(pname, prec, tol, method):
    ks = [3, 5, 2, 6]
    S, inits = sbc.thinned(140, 100, 0.2, ks, 5)
    check_batch(pname, prec, tol, S, ks, inits, [0.1, 0.05, 0.02], [0.2, 0.1, 0.03], 10, -1.0, method, 2)


# ---- 6. each member stops on its own rule ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("trace", [1, 3])
def test_each_member_stops_on_its_own_rule(pname, prec, tol, method, trace):
    """(The stacked padded rank of this batch is 32, a solo member's 16: the SpMM splits the non-zeros over other workers, so batch and
    solo agree to the strict bound here; test_frozen_members_do_not_move_bit_for_bit has the batch whose bits are the solo run's.)"""
    ks = [2, 6, 3, 10, 1]
    S, inits = sbc.thinned(130, 90, 0.3, ks, 21)
    A = sc.densify(S, "zero")
    inits = [(w * s, x * s) for (w, x), s in zip(inits, [1.0, 0.02, 3.0, 0.3, 0.01])]
    # (the oracle's iterations, method 1: trace 1 -> 5, 9, 6, 12, 3; trace 3 -> 10, 12, 10, 12, 7; method 2: 5, 8, 6, 12, 3 and the same)
    max_iter, rel_tol = 12, 1e-3
    t, _ = batch(prec, S, ks, inits, Z3, Z3, max_iter, rel_tol, method, trace)
    its = []
    for b, k in enumerate(ks):
        s = solo(prec, S, k, *inits[b], Z3, Z3, max_iter, rel_tol, method, trace)
        assert t[b]["n_iteration"] == s["n_iteration"] and len(t[b]["target_error"]) == len(s["target_error"])
        assert t[b]["warning"] == s["warning"]
        # (the solo run stopped there: equal factors show that the frozen member did not move afterwards)
        check_member(t[b], s, tol if pname == "f64" else 1e-5, pname == "f64")
        if pname == "f64":
            check_member(t[b], oracle(A, k, *inits[b], Z3, Z3, max_iter, rel_tol, method, trace), tol, True)
        its.append(t[b]["n_iteration"])
    print("iterations", its)
    assert len(set(its)) >= 2 and max(its) == max_iter and min(its) < max_iter, its


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("trace", [1, 3])
def test_frozen_members_do_not_move_bit_for_bit(method, trace):
    """Strict mode, a batch whose stacked padded rank (16) is a solo member's: the SpMM splits the non-zeros alike, the member's Gram and
    sweep are launched as the solo run launches them, so every member must end with the BITS of its solo run -- in particular the
    members that stopped early and sat frozen while the others went on.  Also: the same batch cut off at the first member's stopping
    iteration gives that member the same bits as the long run."""
    ks = [2, 6, 3]
    S, inits = sbc.thinned(130, 90, 0.3, ks, 21)
    inits = [(w * s, x * s) for (w, x), s in zip(inits, [1.0, 0.02, 3.0])]
    long_run, _ = batch(_lib.PREC_F64, S, ks, inits, Z3, Z3, 12, 1e-3, method, trace)
    its = [o["n_iteration"] for o in long_run]
    print("iterations", its)
    first = int(np.argmin(its))
    assert its[first] < max(its), its
    for b, k in enumerate(ks):
        s = solo(_lib.PREC_F64, S, k, *inits[b], Z3, Z3, 12, 1e-3, method, trace)
        assert s["n_iteration"] == its[b] and s["warning"] == long_run[b]["warning"]
        for key in ("W", "H"):
            assert np.array_equal(long_run[b][key], s[key]), (b, key, relF(long_run[b][key], s[key]))
        assert np.array_equal(long_run[b]["average_epoch"], s["average_epoch"])
    short_run, _ = batch(_lib.PREC_F64, S, ks, inits, Z3, Z3, its[first], 1e-3, method, trace)
    for key in ("W", "H"):
        assert np.array_equal(short_run[first][key], long_run[first][key])


# ---- 7. error block against a near-exact fit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", MODES)
def test_error_block_of_a_near_exact_fit(pname, prec, tol):
    """A = W0 H0 on its stored pattern: the zeros' share <W^T W, H H^T> - S2 at its worst cancellation, and its clamp at 0.  Bounds of
    test_gpu_sparse.py's solo test."""
    n, m, ks = 300, 131, [6, 3, 9]
    rng = np.random.default_rng(3)
    facs = [(rng.random((n, k)) * (rng.random((n, k)) < 0.15), rng.random((k, m)) * (rng.random((k, m)) < 0.15)) for k in ks]
    A = facs[0][0] @ facs[0][1]  # (member 0 fits exactly; the others are ordinary members on the same matrix)
    if prec == _lib.PREC_F32:
        A = A.astype(np.float32).astype(np.float64)  # (what the fp32 mode stores)
    S = sc.csc_from_pattern(A != 0, A)
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix_csc_batch(*S)
        h.set_factors_batch(ks, [w for w, _ in facs], [x for _, x in facs])
        t = h.run_batch(Z3, Z3, 0, -1.0, 0, False, 1, 1e-9, 1, 2)  # (no iteration: the closing entry of the trace alone, src/nnmf.cpp:164)
    for b, (W, H) in enumerate(facs):
        e = api.mse_mkl(A, W @ H)
        mse, kl = t[b]["mse_error"][-1], t[b]["mkl_error"][-1]
        print("member %d: mse %.3e (ref %.3e) mkl %.6e (ref %.6e)" % (b, mse, e["MSE"], kl, e["MKL"]))
        assert len(t[b]["mse_error"]) == 1
        assert abs(mse - e["MSE"]) <= 1e-12 * np.mean(A * A) + 1e-10 * e["MSE"], (b, mse, e["MSE"])
        assert abs(kl - e["MKL"]) <= 1e-10 * abs(e["MKL"]) + 4e-15, (b, kl, e["MKL"])
    assert t[0]["mse_error"][-1] >= 0.0


# ---- 8. one pass per phase ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_one_pass_per_phase(pname, prec, tol, method, B):
    ks = [8] * B
    S, inits = sbc.thinned(200, 150, 0.2, ks, 4)
    T = 6
    t, info = batch(prec, S, ks, inits, Z3, Z3, T, -1.0, method, 2, prof=True)
    p = info["prof"]
    ntr = len(t[0]["mse_error"])
    assert ntr == 4  # iterations 0, 2, 4 and the closing entry (src/nnmf.cpp:164)
    assert p["spmm_h"][1] == T and p["spmm_w"][1] == T, p
    assert p["sp_batch_errors"][1] == ntr, p
    assert p["sp_errors"][1] == 0 and p["batch_errors"][1] == 0 and p["errors"][1] == 0 and p["xprod_h"][1] == 0 and p["xprod_w"][1] == 0, p
    assert p["sweep_w"][1] == T * B and p["gram"][1] == 2 * T * B, p


# ---- 9. the door -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", MODES)
def test_the_door_is_the_ordinary_sparse_handle(pname, prec, tol):
    S, inits = sbc.thinned(120, 90, 0.2, [7], 12)
    W0, H0 = inits[0]
    a = solo(prec, S, 7, W0, H0, [0.01, 0, 0.001], Z3, 8, -1.0, 1, 2, door=True)
    b = solo(prec, S, 7, W0, H0, [0.01, 0, 0.001], Z3, 8, -1.0, 1, 2, door=False)
    for key in ("W", "H", "mse_error", "mkl_error", "target_error", "average_epoch"):
        assert np.array_equal(a[key], b[key]), key
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix_csc_batch(*S)
        assert h.get_info("sparse_batch") == 1 and h.get_info("matrix_nnz") == S[1].size
        h.set_factors(7, a["W"], a["H"])
        idx, score = h.top_n(5, by="column", exclude=True)
        P = sc.pattern_of(S)
        full = np.where(P, -np.inf, a["W"] @ a["H"])
        for j in range(0, 90, 17):
            assert not P[idx[j][idx[j] >= 0], j].any()
            assert relF(score[j][0], full[:, j].max()) < (1e-10 if pname == "f64" else 1e-4)
        mse, mkl, _ = h.errors()
        assert np.isfinite(mse) and np.isfinite(mkl)
        h.set_matrix_csc(*S)
        assert h.get_info("sparse_batch") == 0
        h.set_matrix_csc_kl(*S)
        assert h.get_info("sparse_batch") == 0
        h.set_matrix_csc_missing(*S)
        assert h.get_info("sparse_batch") == 0
        h.set_matrix(sc.densify(S, "zero"))
        assert h.get_info("sparse_batch") == 0


def test_refusals_under_the_door():
    rng = np.random.default_rng(0)
    S = sc.rand_csc(60, 50, 0.3, rng)
    W, H = [rng.random((60, 2)), rng.random((60, 3))], [rng.random((2, 50)), rng.random((3, 50))]

    def code(fn):
        with pytest.raises(_lib.NnlmError) as e:
            fn()
        return e.value.code

    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
        h.set_matrix_csc_batch(*S)
        h.set_factors_batch([2, 3], W, H)
        for method in (3, 4):  # KL loss
            assert code(lambda: h.run_batch(Z3, Z3, 3, -1.0, 0, True, 1, 1e-9, method, 1)) == ERR_UNSUPPORTED
        big = [rng.random((60, 33)), rng.random((60, 32))], [rng.random((33, 50)), rng.random((32, 50))]
        assert code(lambda: h.set_factors_batch([33, 32], *big)) == ERR_UNSUPPORTED  # a rank sum of 65
        assert code(lambda: h.set_factors_batch([2, 0], W, H)) == ERR_ARG
        assert code(lambda: h.set_factors_batch([], [], [])) == ERR_ARG
        assert code(lambda: h.comm_init(None, 0, 2)) == ERR_UNSUPPORTED  # (a sparse handle takes no communicator)
        h.set_factors_batch([2, 3], W, H)
        h.run_batch(Z3, Z3, 2, -1.0, 0, True, 5, 1e-9, 1, 1)
        # re-loading through the other sparse entries closes the door again
        for load in (h.set_matrix_csc, h.set_matrix_csc_kl, h.set_matrix_csc_missing):
            load(*S)
            assert code(lambda: h.set_factors_batch([2, 3], W, H)) == ERR_UNSUPPORTED
        h.set_matrix_csc_batch(*S)
        h.set_factors_batch([2, 3], W, H)
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:  # a communicator (virtual rank) first: the sparse loader itself refuses
        h.comm_init(None, 0, 2)
        assert code(lambda: h.set_matrix_csc_batch(*S)) == ERR_UNSUPPORTED
        h.set_matrix(sc.densify(S, "zero"))
        assert code(lambda: h.set_factors_batch([2, 3], W, H)) == ERR_UNSUPPORTED
    # one-shot entry: KL and the rank sum
    assert code(lambda: _lib.c_nnmf_csc_batch(*S, [2, 3], W, H, Z3, Z3, 3, -1.0, 1, 0, True, 1, 1e-9, 3, 1)) == ERR_UNSUPPORTED
    assert code(lambda: _lib.c_nnmf_csc_batch(*S, [40, 25], None, None, Z3, Z3, 3, -1.0, 1, 0, True, 1, 1e-9, 1, 1)) == ERR_UNSUPPORTED
    assert code(lambda: _lib.c_nnmf_csc_batch(*S, [2, 3], W[::-1], H, Z3, Z3, 3, -1.0, 1, 0, True, 1, 1e-9, 1, 1)) == ERR_ARG


# ---- 10. one-shot entry and the API ------------------------------------------------------------------------------------------------------
def test_one_shot_entry_and_api():
    """nnlm_c_nnmf_csc_batch through api.nnmf_batch(sparse_batch=True): member b = nnmf() on the same sparse A with the generator in the
    state member b found it; best = argmin of the final target errors."""
    rng = np.random.default_rng(2)
    V = rng.random((90, 6)) @ rng.random((6, 70)) + 0.05 * rng.random((90, 70))
    S = sc.csc_from_pattern(rng.random((90, 70)) < 0.4, V)
    A = sc.Csc(S)
    opts = dict(max_iter=40, rel_tol=1e-6, alpha=[0.01, 0, 0])
    res, best = api.nnmf_batch(A, [2, 3], nrun=2, rng=np.random.default_rng(17), sparse_batch=True, **opts)
    assert len(res) == 4
    g = np.random.default_rng(17)
    for b, k in enumerate([2, 2, 3, 3]):
        solo_res = api.nnmf(A, k, rng=g, **opts)
        assert relF(res[b]["W"], solo_res["W"]) < 1e-10 and relF(res[b]["H"], solo_res["H"]) < 1e-10
        assert res[b]["n_iteration"] == solo_res["n_iteration"]
        assert np.array_equal(res[b]["average_epochs"], solo_res["average_epochs"])
        assert relF(res[b]["target_loss"], solo_res["target_loss"]) < 1e-10
    assert best == int(np.argmin([r["target_loss"][-1] for r in res]))
    # the default refuses as before
    with pytest.raises(_lib.NnlmError) as e:
        api.nnmf_batch(A, [2, 3], nrun=2, rng=np.random.default_rng(17), **opts)
    assert e.value.code == ERR_UNSUPPORTED
    # the library's default init (W_init = H_init = NULL) is drawn in nnlm_c_nnmf_batch's order: member by member, W before H
    out = _lib.c_nnmf_csc_batch(*S, [3, 2], None, None, Z3, Z3, 5, -1.0, 1, 0, True, 50, 1e-9, 1, 1)
    dense = _lib.c_nnmf_batch(sc.densify(S, "zero"), [3, 2], None, None, Z3, Z3, 5, -1.0, 1, 0, True, 50, 1e-9, 1, 1)
    o1 = _lib.c_nnmf_csc(*S, 3, None, None, None, None, Z3, Z3, 5, -1.0, 1, 0, True, 50, 1e-9, 1, 1)
    assert relF(out[0]["W"], o1["W"]) < 1e-10 and out[0]["n_iteration"] == o1["n_iteration"]
    for b in range(2):
        assert relF(out[b]["W"], dense[b]["W"]) < 1e-10 and relF(out[b]["H"], dense[b]["H"]) < 1e-10
