"""Batched KL factorisation on a sparse count matrix (nnlm_set_matrix_csc_kl_batch + the batch entries with methods 3 and 4,
nnlm_c_nnmf_csc_kl_batch, api.nnmf_batch(loss="mkl", sparse_batch="kl")) on the MI355X.  Run with `pytest -m gpu`.

The property under test: nothing in a member's half-step depends on its neighbours, its position in the stack or the group size of
sp_kl_batch_kernel, so member b is BIT-IDENTICAL to the solo fit of rank k_b on an nnlm_set_matrix_csc_kl handle from the same start
(np.array_equal on W and H, equal n_iteration and average_epoch); only the traces differ, by the error block's summation order.

Bounds (those of test_gpu_sparse_batch.py and test_gpu_sparse_kl.py): strict mode 1e-10 against the oracle with equal iteration and sweep
counts; fp32-operand mode 1e-4, widened to 1.01 x the solo fp32 run's own distance to the oracle; traces: mse within tol mse + 1e-12
mean(A^2), mkl and target within tol |ref| + 4e-15 (tol = 1e-10 strict, 1e-4 fp32).  Cases: tests/sparse_kl_batch_cases.py; the ones
compared with the oracle are shown well posed by tests/test_sparse_kl_batch_host.py.  Every test fails without the feature: the symbols
do not exist."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402
from oracle import ref  # noqa: E402
import sparse_cases as sc  # noqa: E402
import sparse_kl_cases as kc  # noqa: E402
import sparse_kl_batch_cases as kb  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = [("f64", _lib.PREC_F64, 1e-10), ("f32", _lib.PREC_F32, 1e-4)]
ERR_ARG, ERR_UNSUPPORTED = 1, 5
Z3 = [0.0, 0.0, 0.0]
SEEDS = max(1, 12 * int(os.environ.get("NNLM_FUZZ_SEEDS", "16")) // 16)
PROF = ("spkl_batch_h", "spkl_batch_w", "spkl_copy", "spkl_solve_h", "spkl_solve_w", "spmm_h", "spmm_w", "sp_batch_errors", "gram", "sweep_w")
TRACES = ("mse_error", "mkl_error", "target_error", "average_epoch")


@pytest.fixture(autouse=True)
def _default_precision(monkeypatch):
    monkeypatch.delenv("NNLM_PRECISION", raising=False)


def batch(prec, S, ks, inits, alpha, beta, max_iter, rel_tol, method, trace, inner=1, inner_tol=1e-9, loader="set_matrix_csc_kl_batch",
          prof=False):
    with nnlm_amd.Handle(0, prec) as h:
        getattr(h, loader)(*S)
        h.set_factors_batch(ks, [w for w, _ in inits], [x for _, x in inits])
        if prof:
            h.profile_enable(True)
        t = h.run_batch(alpha, beta, max_iter, rel_tol, 0, False, inner, inner_tol, method, trace)
        f = h.get_factors_batch()
        info = {key: int(h.get_info("sparse_kl_batch_" + key)) for key in ("form_w", "form_h", "group")}
        if prof:
            info["prof"] = {nm: h.profile_get(nm) for nm in PROF}
    for o, (W, H) in zip(t, f):
        o["W"], o["H"] = W, H
    return t, info


def solo(prec, S, k, W, H, alpha, beta, max_iter, rel_tol, method, trace, inner=1, inner_tol=1e-9, loader="set_matrix_csc_kl"):
    with nnlm_amd.Handle(0, prec) as h:
        getattr(h, loader)(*S)
        h.set_factors(k, W, H)
        t = h.run(alpha, beta, max_iter, rel_tol, 0, False, inner, inner_tol, method, trace)
        t["W"], t["H"] = h.get_factors()
    return t


def check_traces(r, o, A, tol, what):
    """check_traces of test_gpu_sparse_kl.py."""
    for key in TRACES:
        assert np.shape(r[key]) == np.shape(o[key]), (what, key)
    dm = np.abs(np.asarray(r["mse_error"]) - np.asarray(o["mse_error"]))
    bm = tol * np.asarray(o["mse_error"]) + 1e-12 * np.mean(A * A)
    assert np.all(dm <= bm), (what, "mse", float(np.max(dm / bm)))
    for key in ("mkl_error", "target_error"):
        d = np.abs(np.asarray(r[key]) - np.asarray(o[key]))
        b = tol * np.abs(np.asarray(o[key])) + 4e-15
        print(what, key, float(np.max(d / b, initial=0.0)), "of bound")
        assert np.all(d <= b), (what, key, float(np.max(d / b)))


def same_bits(o, s, A, tol, what):
    """Member o of a batch against the solo run s: the factors' bits, the iteration and sweep counts; the traces within the bounds."""
    for key in ("W", "H"):
        assert np.array_equal(o[key], s[key]), (what, key, sc.err(o[key], s[key]), int(np.sum(o[key] != s[key])))
    assert o["n_iteration"] == s["n_iteration"] and o["warning"] == s["warning"], (what, o["n_iteration"], s["n_iteration"])
    assert np.array_equal(o["average_epoch"], s["average_epoch"]), (what, o["average_epoch"], s["average_epoch"])
    check_traces(o, s, A, tol, what)


def batch_equals_solo(prec, tol, S, ks, inits, alpha, beta, max_iter, rel_tol, method, trace, inner=1, inner_tol=1e-9):
    A = sc.densify(S, "zero")
    t, info = batch(prec, S, ks, inits, alpha, beta, max_iter, rel_tol, method, trace, inner, inner_tol)
    solos = []
    for b, k in enumerate(ks):
        s = solo(prec, S, k, *inits[b], alpha, beta, max_iter, rel_tol, method, trace, inner, inner_tol)
        same_bits(t[b], s, A, tol, "member %d (rank %d)" % (b, k))
        assert np.all(np.isfinite(t[b]["W"])) and np.all(np.isfinite(t[b]["H"]))
        solos.append(s)
    assert info["group"] in kb.GROUPS
    return t, solos, info


# ---- 1. member = solo, bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [3, 4])
@pytest.mark.parametrize("density", [0.01, 0.2, 1.0])
@pytest.mark.parametrize("ks", [[5], [1, 4, 7], [1, 4, 7, 16, 3, 2, 8, 6]])
def test_member_equals_solo_bit_for_bit(pname, prec, tol, method, density, ks):
    c = kb.count_batch(150, 110, ks, density, 11 * len(ks) + method + int(100 * density))
    batch_equals_solo(prec, tol, c["S"], ks, c["inits"], Z3, Z3, 12, -1.0, method, 3, inner=1 if method == 3 else 2)


# ---- 2. member = oracle on the densified matrix --------------------------------------------------------------------------------------------
ORACLE = kb.oracle_cases()


@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("i", range(len(ORACLE)), ids=["%s m%d i%d" % (c["name"], me, inn) for c, me, inn in ORACLE])
def test_member_equals_oracle(pname, prec, tol, i):
    c, method, inner = ORACLE[i]
    A = sc.densify(c["S"], "zero")
    ra, rb = kb.ORACLE_REG
    t, solos, _ = batch_equals_solo(prec, tol, c["S"], c["ks"], c["inits"], ra, rb, kb.ORACLE_ITERS, -1.0, method, 1, inner)
    for b, k in enumerate(c["ks"]):
        o = kb.oracle_run(ref, A, k, c["inits"][b], method, inner)
        bound = tol if pname == "f64" else max(tol, 1.01 * sc.err(solos[b]["W"], o["W"]), 1.01 * sc.err(solos[b]["H"], o["H"]))
        ew, eh = sc.err(t[b]["W"], o["W"]), sc.err(t[b]["H"], o["H"])
        print(c["name"], pname, method, b, "W %.3e H %.3e (bound %.3g)" % (ew, eh, bound))
        assert ew <= bound and eh <= bound, (b, ew, eh, bound)
        assert t[b]["n_iteration"] == o["n_iteration"] == kb.ORACLE_ITERS
        check_traces(t[b], o, A, tol, "member %d vs oracle" % b)
        if pname == "f64":
            assert np.array_equal(t[b]["average_epoch"], o["average_epoch"])


# ---- 3. edges of the stack and of the group ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [3, 4])
@pytest.mark.parametrize("ks", [[1], [64], [16, 16, 16, 16], [30, 1, 33], [16, 1], [1, 16], [8, 9]])
def test_edges_of_the_stack(pname, prec, tol, method, ks):
    c = kb.count_batch(180, 140, ks, 0.2, sum(ks) + method)
    batch_equals_solo(prec, tol, c["S"], ks, c["inits"], Z3, [0.01, 0, 0], 5, -1.0, method, 2, inner=1 if method == 3 else 2)


def group_size():
    c = kc.count_case(40, 30, 3, 0.3, 5)
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
        h.set_matrix_csc_kl_batch(*c["S"])
        g = int(h.get_info("sparse_kl_batch_group"))
    assert g in kb.GROUPS
    return g


@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [3, 4])
def test_member_counts_around_the_group(pname, prec, tol, method):
    """G - 1, G, G + 1 and 2 G + 1 members (a short last group, a full one, one member left over), with ranks that differ inside a group."""
    G = group_size()
    for B in sorted({max(G - 1, 1), G, G + 1, 2 * G + 1}):
        ks = [1 + (3 * b) % 7 for b in range(B)]
        c = kb.count_batch(150, 110, ks, 0.2, 40 + B)
        batch_equals_solo(prec, tol, c["S"], ks, c["inits"], Z3, Z3, 4, -1.0, method, 2, inner=1 if method == 3 else 2)


@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [3, 4])
def test_a_group_holding_ranks_1_and_33(pname, prec, tol, method):
    """Two members are one group at every group size above 1: for 32 of the 33 coordinate steps the rank-1 member is predicated off."""
    ks = [1, 33]
    c = kb.count_batch(150, 110, ks, 0.2, 77)
    batch_equals_solo(prec, tol, c["S"], ks, c["inits"], Z3, Z3, 4, -1.0, method, 2, inner=1 if method == 3 else 3)


@pytest.mark.parametrize("pname,prec,tol", MODES)
def test_members_of_a_group_leave_the_sweep_loop_at_different_sweeps(pname, prec, tol):
    """Lee, up to five inner sweeps, an inner tolerance (0.1) that the lines of a member meet after three to five sweeps: the members a
    wavefront interleaves leave the sweep loop at different sweeps.  Every member's average_epoch is its solo run's."""
    ks = [4, 4, 4, 4]
    c = kb.count_batch(150, 110, ks, 0.3, 7)
    inits = [(w * s, x * s) for (w, x), s in zip(c["inits"], [1.0, 0.3, 3.0, 0.05])]
    t, solos, info = batch_equals_solo(prec, tol, c["S"], ks, inits, Z3, Z3, 3, -1.0, 4, 1, inner=5, inner_tol=0.1)
    ep = [tuple(o["average_epoch"]) for o in t]
    print("average_epoch", ep)
    assert all(1.0 < e < 5.0 for o in ep for e in o)  # (neither every line at the cap nor at one sweep)
    assert len(set(ep[:2])) == 2 and len(set(ep[2:])) == 2  # (equal ranks keep their order: members 0, 1 share a group at G >= 2)


# ---- 4. line lengths -----------------------------------------------------------------------------------------------------------------------
LINES = kb.line_cases()


@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [3, 4])
@pytest.mark.parametrize("i", range(len(LINES)), ids=[c["name"].replace(" ", "_") for c in LINES])
def test_line_lengths(pname, prec, tol, method, i):
    """Lines of 0, 1, 63, 64, 65, 255, 256 and 257 stored entries in both orientations (the batched short kernel and the per-member long
    launches in one half-step), a line holding half of all entries, the pattern families; every penalty position."""
    c = LINES[i]
    reg = kc.REGS["all"]
    _, _, info = batch_equals_solo(prec, tol, c["S"], c["ks"], c["inits"], reg, reg[::-1], 3, -1.0, method, 1, inner=1 if method == 3 else 2)
    assert (info["form_w"], info["form_h"]) == kc.line_forms(c["S"]), (info, kc.line_forms(c["S"]))


# ---- 5. each member stops on its own rule --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [3, 4])
@pytest.mark.parametrize("trace", [1, 3])
def test_each_member_stops_on_its_own_rule(pname, prec, tol, method, trace):
    """(the oracle's iterations at rel_tol 0.01: SCD 4, 7, 20, 7, 12 (trace 1) and 7, 13, 20, 13, 16 (trace 3); Lee 3, 6, 3, 10, 2 and 7, 19,
    10, 20, 4.)  A member that stopped sits frozen while the others go on: its factors are its solo run's bits, which stopped there."""
    ks = [2, 6, 3, 10, 1]
    c = kb.count_batch(150, 110, ks, 0.3, 21)
    inits = [(w * s, x * s) for (w, x), s in zip(c["inits"], [1.0, 0.02, 3.0, 0.3, 0.01])]
    t, solos, _ = batch_equals_solo(prec, tol, c["S"], ks, inits, Z3, Z3, 20, 0.01, method, trace)
    its = [o["n_iteration"] for o in t]
    print("iterations", its)
    assert its == [s["n_iteration"] for s in solos]
    assert len(set(its)) >= 3 and min(its) < max(its), its
    # the same batch cut off where its first member stopped: that member has the long run's bits (it did not move afterwards)
    first = int(np.argmin(its))
    short, _ = batch(prec, c["S"], ks, inits, Z3, Z3, its[first], 0.01, method, trace)
    for key in ("W", "H"):
        assert np.array_equal(short[first][key], t[first][key]), key


# ---- 6. independence and determinism ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [3, 4])
def test_independence_and_determinism(pname, prec, tol, method):
    """Permuting the members, adding one (stacked padded rank 32 -> 32 and 32 -> 48) and running twice: every member keeps its bits."""
    ks = [4, 7, 1, 9]
    c = kb.count_batch(160, 120, ks + [5, 12], 0.2, 8)
    inits = c["inits"]
    A = sc.densify(c["S"], "zero")
    args = (Z3, [0, 0, 0.01], 8, -1.0, method, 2, 1 if method == 3 else 2)
    base, _ = batch(prec, c["S"], ks, inits[:4], *args)
    again, _ = batch(prec, c["S"], ks, inits[:4], *args)
    perm = [2, 0, 3, 1]
    tp, _ = batch(prec, c["S"], [ks[p] for p in perm], [inits[p] for p in perm], *args)
    t5, _ = batch(prec, c["S"], ks + [5], inits[:5], *args)
    t12, _ = batch(prec, c["S"], ks + [12], inits[:4] + [inits[5]], *args)
    for b in range(4):
        for key in ("W", "H") + TRACES:
            assert np.array_equal(again[b][key], base[b][key]), (b, key)  # two runs: the same bits, traces included
        for other, what in ((tp[perm.index(b)], "permuted"), (t5[b], "one more, KP 32"), (t12[b], "one more, KP 48")):
            same_bits(other, base[b], A, tol, "%s member %d" % (what, b))


# ---- 7. the door -----------------------------------------------------------------------------------------------------------------------------
def code_of(fn, *a):
    with pytest.raises(_lib.NnlmError) as ei:
        fn(*a)
    return ei.value.code, str(ei.value)


@pytest.mark.parametrize("pname,prec,tol", MODES)
def test_refusals_that_stay(pname, prec, tol):
    c = kb.count_batch(120, 90, [2, 3], 0.3, 3)
    S, ks, inits = c["S"], c["ks"], c["inits"]
    Ws, Hs = [w for w, _ in inits], [x for _, x in inits]
    ptr, idx, val, shp = S
    A = sc.densify(S, "zero")
    run = (Z3, Z3, 2, -1.0, 0, False, 1, 1e-9)
    with nnlm_amd.Handle(0, prec) as h:
        # an nnlm_set_matrix_csc_kl handle: refused with its present message
        h.set_matrix_csc_kl(*S)
        assert h.get_info("sparse_kl_batch") == 0
        code, msg = code_of(h.set_factors_batch, ks, Ws, Hs)
        assert code == ERR_UNSUPPORTED and "nnlm_set_matrix_csc_kl" in msg and "nnlm_set_matrix_csc_kl_batch" not in msg
        # methods 3 and 4 on every other batch handle
        hold = (np.array([0, 1] + [1] * (shp[1] - 1), dtype=np.int64), np.array([0], dtype=np.int32))
        for load in (lambda: h.set_matrix(A), lambda: h.set_matrix_csc_batch(*S), lambda: h.set_matrix_csc_missing_batch(*S),
                     lambda: h.set_matrix_holdout(A, *hold)):
            load()
            h.set_factors_batch(ks, Ws, Hs)
            for method in (3, 4):
                code, msg = code_of(h.run_batch, *run, method, 1)
                assert code == ERR_UNSUPPORTED and "square loss (methods 1, 2) only" in msg, msg
            h.run_batch(*run, 1, 1)
        # the new handle: the checks of nnlm_set_matrix_csc_kl, the communicator, the rank sum
        for bad in (-1.0, np.nan, np.inf):
            v = val.copy()
            v[3] = bad
            code, msg = code_of(h.set_matrix_csc_kl_batch, ptr, idx, v, shp)
            assert code == ERR_ARG and "entry 3" in msg and "nnlm_set_matrix_csc_kl_batch" in msg
        swapped = idx.copy()
        j = int(np.argmax(np.diff(ptr)))
        swapped[ptr[j]], swapped[ptr[j] + 1] = idx[ptr[j] + 1], idx[ptr[j]]
        assert code_of(h.set_matrix_csc_kl_batch, ptr, swapped, val, shp)[0] == ERR_ARG
        h.set_matrix_csc_kl_batch(*S)
        assert h.get_info("sparse_kl_batch") == 1 and h.get_info("sparse_kl") == 1 and h.get_info("sparse_batch") == 1
        assert h.get_info("sparse_kl_batch_form_w") == -1 and h.get_info("sparse_kl_batch_form_h") == -1
        assert code_of(h.comm_init, None, 0, 2)[0] == ERR_UNSUPPORTED
        rng = np.random.default_rng(0)
        big = [rng.random((shp[0], 33)), rng.random((shp[0], 32))], [rng.random((33, shp[1])), rng.random((32, shp[1]))]
        assert code_of(h.set_factors_batch, [33, 32], *big)[0] == ERR_UNSUPPORTED
        assert code_of(h.set_factors_batch, [2, 0], Ws, Hs)[0] == ERR_ARG
        h.set_factors_batch(ks, Ws, Hs)
        assert code_of(h.run_batch, *run, 5, 1)[0] == ERR_ARG
        for method in (1, 2, 3, 4):
            h.run_batch(*run, method, 1)
        for load in (h.set_matrix_csc, h.set_matrix_csc_kl, h.set_matrix_csc_missing):  # re-loading through another entry closes the door
            load(*S)
            assert h.get_info("sparse_kl_batch") == 0 and code_of(h.set_factors_batch, ks, Ws, Hs)[0] == ERR_UNSUPPORTED
    # the other one-shot batch entries keep refusing KL; the new one takes it and refuses what the batch refuses
    tail = (Z3, Z3, 2, -1.0, 1, 0, False, 1, 1e-9)
    for method in (3, 4):
        assert code_of(_lib.c_nnmf_batch, A, ks, Ws, Hs, *tail, method, 1)[0] == ERR_UNSUPPORTED
        assert code_of(_lib.c_nnmf_csc_batch, *S, ks, Ws, Hs, *tail, method, 1)[0] == ERR_UNSUPPORTED
        assert code_of(_lib.c_nnmf_csc_missing_batch, *S, ks, Ws, Hs, *tail, method, 1)[0] == ERR_UNSUPPORTED
        assert code_of(_lib.c_nnmf_holdout_batch, A, *hold, ks, Ws, Hs, *tail, method, 1)[0] == ERR_UNSUPPORTED
    assert code_of(_lib.c_nnmf_csc_kl_batch, *S, [40, 25], None, None, *tail, 3, 1)[0] == ERR_UNSUPPORTED
    assert code_of(_lib.c_nnmf_csc_kl_batch, *S, ks, Ws[::-1], Hs, *tail, 3, 1)[0] == ERR_ARG
    assert code_of(_lib.c_nnmf_csc_kl_batch, *S, ks, Ws, Hs, *tail, 5, 1)[0] == ERR_ARG


@pytest.mark.parametrize("pname,prec,tol", MODES)
def test_the_new_handle_is_the_old_ones(pname, prec, tol, monkeypatch):
    """Solo calls: the nnlm_set_matrix_csc_kl handle's bits (all four methods).  Batched methods 1 and 2: the nnlm_set_matrix_csc_batch
    handle's bits.  The one-shot entry: the resident run's bits."""
    c = kb.count_batch(150, 110, [3, 6, 2], 0.2, 5)
    S, ks, inits = c["S"], c["ks"], c["inits"]
    for method in (1, 2, 3, 4):
        inner = 5 if method < 3 else 1
        a = solo(prec, S, 6, *inits[1], [0.01, 0, 0.001], Z3, 5, -1.0, method, 2, inner, loader="set_matrix_csc_kl_batch")
        b = solo(prec, S, 6, *inits[1], [0.01, 0, 0.001], Z3, 5, -1.0, method, 2, inner, loader="set_matrix_csc_kl")
        for key in ("W", "H") + TRACES:
            assert np.array_equal(a[key], b[key]), (method, key)
    for method in (1, 2):
        a, _ = batch(prec, S, ks, inits, Z3, [0.01, 0, 0], 5, -1.0, method, 2, 5, loader="set_matrix_csc_kl_batch")
        b, _ = batch(prec, S, ks, inits, Z3, [0.01, 0, 0], 5, -1.0, method, 2, 5, loader="set_matrix_csc_batch")
        for x, y in zip(a, b):
            for key in ("W", "H") + TRACES:
                assert np.array_equal(x[key], y[key]), (method, key)
    if pname == "f32":
        monkeypatch.setenv("NNLM_PRECISION", "f32")
    for method in (3, 4):
        a, _ = batch(prec, S, ks, inits, Z3, [0.01, 0, 0], 5, -1.0, method, 2)
        o = _lib.c_nnmf_csc_kl_batch(*S, ks, [w for w, _ in inits], [x for _, x in inits], Z3, [0.01, 0, 0], 5, -1.0, 1, 0, False, 1, 1e-9,
                                     method, 2)
        for x, y in zip(a, o):
            for key in ("W", "H") + TRACES:
                assert np.array_equal(x[key], y[key]), (method, key)
            assert x["n_iteration"] == y["n_iteration"] == 5


# ---- 8. one launch for all members -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [3, 4])
def test_one_launch_for_all_members(pname, prec, tol, method):
    """The profile counts scopes, not kernels: one spkl_batch_* scope per half-step whatever B is, no solo solver scope, no SpMM, no Gram
    and no per-member sweep beside it, and the same number of row copies for every B.  That the scope holds ONE sp_kl_batch_kernel launch
    is the host code's (batch_half_step_sparse_kl launches it once, outside its member loop); the form bits say that it ran and that no
    per-member long launch did."""
    copies = set()
    for B in (1, 3, 8):
        ks = [8] * B
        c = kb.count_batch(200, 150, ks, 0.2, 4)
        assert kc.line_forms(c["S"]) == (1, 1)  # every line short
        T = 6
        t, info = batch(prec, c["S"], ks, c["inits"], Z3, Z3, T, -1.0, method, 2, prof=True)
        p = info["prof"]
        assert p["spkl_batch_h"][1] == T and p["spkl_batch_w"][1] == T, p  # (a scope per half-step, ONE launch in it: forms == 1)
        assert (info["form_w"], info["form_h"]) == (1, 1)
        assert p["spmm_h"][1] == 0 and p["spmm_w"][1] == 0 and p["spkl_solve_h"][1] == 0 and p["spkl_solve_w"][1] == 0, p
        assert p["gram"][1] == 0 and p["sweep_w"][1] == 0, p
        assert p["sp_batch_errors"][1] == len(t[0]["mse_error"]) == 4, p
        copies.add(p["spkl_copy"][1])
    assert copies == {2 * 6}, copies


# ---- 9. Python -------------------------------------------------------------------------------------------------------------------------------
def test_api_nnmf_batch():
    c = kb.count_batch(90, 70, [2, 2, 3, 3], 0.4, 9)
    A = sc.Csc(c["S"])
    opts = dict(loss="mkl", max_iter=15, rel_tol=1e-3)
    init = [{"W": w, "H": x} for w, x in c["inits"]]
    for method in ("scd", "lee"):
        res, best = api.nnmf_batch(A, [2, 3], nrun=2, sparse_batch="kl", init=init, method=method, rng=np.random.default_rng(17), **opts)
        assert len(res) == 4
        for b, k in enumerate([2, 2, 3, 3]):
            s = api.nnmf(A, k, sparse_kl=True, init=init[b], method=method, **opts)
            assert np.array_equal(res[b]["W"], s["W"]) and np.array_equal(res[b]["H"], s["H"]), (method, b)
            assert res[b]["n_iteration"] == s["n_iteration"] and np.array_equal(res[b]["average_epochs"], s["average_epochs"])
            assert res[b]["options"]["loss"] == "mkl"
        assert best == int(np.argmin([r["target_loss"][-1] for r in res]))
    # inits drawn from the generator, member by member, as nnmf() draws them
    res, best = api.nnmf_batch(A, [2, 3], nrun=2, sparse_batch="kl", rng=np.random.default_rng(17), **opts)
    g = np.random.default_rng(17)
    for b, k in enumerate([2, 2, 3, 3]):
        s = api.nnmf(A, k, sparse_kl=True, rng=g, **opts)
        assert np.array_equal(res[b]["W"], s["W"]) and np.array_equal(res[b]["H"], s["H"]), b
    assert best == int(np.argmin([r["target_loss"][-1] for r in res]))
    # square loss through this door is sparse_batch = True
    r1, _ = api.nnmf_batch(A, [2, 3], sparse_batch="kl", rng=np.random.default_rng(3), max_iter=5, rel_tol=-1.0)
    r2, _ = api.nnmf_batch(A, [2, 3], sparse_batch=True, rng=np.random.default_rng(3), max_iter=5, rel_tol=-1.0)
    assert all(np.array_equal(x["W"], y["W"]) and np.array_equal(x["H"], y["H"]) for x, y in zip(r1, r2))


# ---- 10. randomised parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("seed", range(SEEDS))
def test_randomised_parity(pname, prec, tol, seed):
    seed = kb.fuzz_seed(seed)
    c = kb.fuzz_case(seed)
    A = sc.densify(c["S"], "zero")
    reg = (c["alpha"], c["beta"])
    t, solos, info = batch_equals_solo(prec, tol, c["S"], c["ks"], c["inits"], *reg, c["max_iter"], -1.0, c["method"], 1, c["inner"])
    assert (info["form_w"], info["form_h"]) == kc.line_forms(c["S"])
    for b in kb.FUZZ_WELL_POSED.get(seed, []):  # (the members tests/test_sparse_kl_batch_host.py shows well posed)
        o = kb.oracle_run(ref, A, c["ks"][b], c["inits"][b], c["method"], c["inner"], c["max_iter"], reg)
        bound = tol if pname == "f64" else max(tol, 1.01 * sc.err(solos[b]["W"], o["W"]), 1.01 * sc.err(solos[b]["H"], o["H"]))
        ew, eh = sc.err(t[b]["W"], o["W"]), sc.err(t[b]["H"], o["H"])
        print(c["name"], pname, b, "W %.3e H %.3e (bound %.3g)" % (ew, eh, bound))
        assert ew <= bound and eh <= bound, (seed, b, ew, eh, bound)
        if pname == "f64":
            assert np.array_equal(t[b]["average_epoch"], o["average_epoch"])
