"""Rank selection on held-out entries on the MI355X: nnlm_set_matrix_holdout, the batch half-step with missing
entries, nnlm_holdout_errors, nnlm_c_nnmf_holdout_batch and api.nnmf_cv.  Run with `pytest -m gpu`.

Bounds are those of tests/test_gpu_batch.py: against the fp64 oracle on the NaN matrix, strict mode 1e-10 with equal iteration and sweep
counts, fp32-operand mode 1e-4 (or the solo fp32 run's own distance to the oracle); batch against the solo missing-value run of the same
mode 1e-10 / 1e-5.  Held-out sums against numpy: 1e-12 relative (strict), rtol 1e-3 (fp32: test_gpu_fuzz_sparse.py's bound for its
error sums).  Every input generator asserts that each row and column keeps max k_b + 1 observed entries (cv_cases.assert_trainable)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cv_cases as cv  # noqa: E402
from helpers import relF  # noqa: E402
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402
from oracle import ref  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = [("f64", _lib.PREC_F64, 1e-10), ("f32", _lib.PREC_F32, 1e-4)]
ERR_ARG, ERR_UNSUPPORTED = 1, 5
Z3 = [0.0, 0.0, 0.0]
TRACE_KEYS = ("mse_error", "mkl_error", "target_error", "average_epoch")


@pytest.fixture(autouse=True)
def _default_precision(monkeypatch):
    monkeypatch.delenv("NNLM_PRECISION", raising=False)


def problem(n, m, ks, frac, seed):
    """test_gpu_batch.problem's matrix (full rank with a rank-6 component), a hold-out pattern of the given fraction, member inits."""
    rng = np.random.default_rng(seed)
    A = rng.random((n, m)) + 0.5 * rng.random((n, 6)) @ rng.random((6, m))
    ptr, idx = api._holdout_pattern(frac, n, m, rng)
    cv.assert_trainable(A, ptr, idx, max(ks))
    inits = [(rng.random((n, k)), rng.random((k, m))) for k in ks]
    return A, ptr, idx, inits


def oracle(An, k, W, H, alpha, beta, max_iter, rel_tol, method, trace):
    return ref.c_nnmf(An, k, W, H, None, None, alpha, beta, max_iter, rel_tol, 1, 0, True, 50, 1e-9, method, trace)


def batch(prec, A, ptr, idx, ks, inits, alpha, beta, max_iter, rel_tol, method, trace, prof=False):
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix_holdout(A, ptr, idx)
        h.set_factors_batch(ks, [w for w, _ in inits], [x for _, x in inits])
        if prof:
            h.profile_enable(True)
        t = h.run_batch(alpha, beta, max_iter, rel_tol, 0, True, 50, 1e-9, method, trace)
        f = h.get_factors_batch()
        hm, hk = h.holdout_errors()
        p = {nm: h.profile_get(nm) for nm in ("xprod_h", "xprod_w", "batch_errors", "errors")} if prof else None
    for b, (o, (W, H)) in enumerate(zip(t, f)):
        o["W"], o["H"], o["holdout_mse"], o["holdout_mkl"] = W, H, hm[b], hk[b]
    return t, p


def solo_na(prec, An, k, W, H, alpha, beta, max_iter, rel_tol, method, trace):
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix(An)
        h.set_factors(k, W, H)
        t = h.run(alpha, beta, max_iter, rel_tol, 0, True, 50, 1e-9, method, trace)
        t["W"], t["H"] = h.get_factors()
    return t


def check_member(o, r, tol, strict, solo_run=None):
    """test_gpu_batch.check_member: o = batch member, r = reference run; fp32 with solo_run: the solo fp32 path's own distance to r."""
    if solo_run is not None and not strict:
        tol = max(tol, 1.01 * relF(solo_run["W"], r["W"]), 1.01 * relF(solo_run["H"], r["H"]))
    print("   member k=%d  W %.2e  H %.2e  (bound %.1e)" % (o["W"].shape[1], relF(o["W"], r["W"]), relF(o["H"], r["H"]), tol))
    assert relF(o["W"], r["W"]) < tol and relF(o["H"], r["H"]) < tol, (relF(o["W"], r["W"]), relF(o["H"], r["H"]), tol)
    assert o["n_iteration"] == r["n_iteration"] and len(o["mse_error"]) == len(r["mse_error"])
    if strict:
        assert np.array_equal(o["average_epoch"], r["average_epoch"]), (o["average_epoch"], r["average_epoch"])
        for key in ("mse_error", "target_error", "mkl_error"):
            assert relF(o[key], r[key]) < tol, (key, relF(o[key], r[key]))


def check_holdout_sums(o, A, ptr, idx, strict):
    want = cv.numpy_holdout_errors(A, ptr, idx, o["W"], o["H"])
    for got, w in zip((o["holdout_mse"], o["holdout_mkl"]), want):
        assert abs(got - w) <= (1e-12 if strict else 1e-3) * abs(w), (got, w)


def check_all(prec, pname, tol, A, ptr, idx, ks, inits, alpha, beta, max_iter, method, trace):
    strict = pname == "f64"
    An = cv.with_nan(A, ptr, idx)
    t, _ = batch(prec, A, ptr, idx, ks, inits, alpha, beta, max_iter, -1.0, method, trace)
    for b, k in enumerate(ks):
        o = oracle(An, k, *inits[b], alpha, beta, max_iter, -1.0, method, trace)
        s = solo_na(prec, An, k, *inits[b], alpha, beta, max_iter, -1.0, method, trace)
        check_member(t[b], o, tol, strict, solo_run=s)
        check_member(t[b], s, tol if strict else 1e-5, strict)
        check_holdout_sums(t[b], A, ptr, idx, strict)


@pytest.mark.parametrize("pname,prec,tol", MODES)
def test_handle_state_equals_the_nan_upload(pname, prec, tol):
    """matrix_info and a solo run equal set_matrix(A with NaN at the pattern) -- bit for bit in strict mode; solo held-out sums = numpy."""
    A, ptr, idx, inits = problem(150, 110, [5], 0.2, 3)
    An = cv.with_nan(A, ptr, idx)
    for method in (1, 2, 3, 4):
        inner = 50 if method < 3 else 1
        with nnlm_amd.Handle(0, prec) as h, nnlm_amd.Handle(0, prec) as g:
            h.set_matrix_holdout(A, ptr, idx)
            g.set_matrix(An)
            assert h.matrix_info() == g.matrix_info() and h.matrix_info()["any_missing"]
            assert h.get_info("matrix_holdout") == idx.size and g.get_info("matrix_holdout") == -1
            res = []
            for x in (h, g):
                x.set_factors(5, *inits[0])
                t = x.run([0.01, 0, 0], Z3, 8, -1.0, 0, True, inner, 1e-9, method, 2)
                t["W"], t["H"] = x.get_factors()
                res.append(t)
            for key in TRACE_KEYS + ("W", "H"):
                if pname == "f64":
                    assert np.array_equal(res[0][key], res[1][key]), (method, key)
                else:
                    assert relF(res[0][key], res[1][key]) < 1e-6, (method, key)
            hm, hk = h.holdout_errors()
            assert hm.shape == (1,)
            check_holdout_sums(dict(W=res[0]["W"], H=res[0]["H"], holdout_mse=hm[0], holdout_mkl=hk[0]), A, ptr, idx, pname == "f64")
    assert not np.isnan(A).any()  # (the caller's matrix is not written)


@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("ks,frac", [([5], 0.05), ([1, 4, 12], 0.3), ([1, 4, 7, 16, 3, 2, 8, 23], 0.05), ([1], 0.3)])
def test_member_equals_oracle_and_solo_na_run(pname, prec, tol, method, ks, frac):
    """B = 1, 3 and 8; rank sums 17 and 64; rank 1; 5 % and 30 % held out."""
    A, ptr, idx, inits = problem(170, 120, ks, frac, 11 * len(ks) + method)
    check_all(prec, pname, tol, A, ptr, idx, ks, inits, Z3, Z3, 10, method, 3)


@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("pos", [0, 1, 2])
def test_penalties_in_each_position(pname, prec, tol, pos):
    ks = [3, 5, 2, 6]
    alpha, beta = [0.0] * 3, [0.0] * 3
    alpha[pos], beta[pos] = [0.1, 0.05, 0.02][pos], [0.2, 0.1, 0.03][pos]
    if pos == 1:  # (the angle penalty needs L2 >= angle, as the reference's arguments do)
        alpha[0], beta[0] = 0.1, 0.2
    A, ptr, idx, inits = problem(140, 100, ks, 0.3, 5 + pos)
    for method in (1, 2):
        check_all(prec, pname, tol, A, ptr, idx, ks, inits, alpha, beta, 8, method, 2)


def test_independence_of_members():
    """Strict mode: permuting the members or adding one changes no member's bits -- factors, traces, sweep counts, held-out sums."""
    ks = [4, 7, 1, 9]
    A, ptr, idx, inits = problem(160, 120, ks + [12], 0.2, 8)
    run = lambda kk, ii: batch(_lib.PREC_F64, A, ptr, idx, kk, ii, Z3, Z3, 8, -1.0, 1, 2)[0]  # noqa: E731
    base = run(ks, inits[:4])
    perm = [2, 0, 3, 1]
    tp = run([ks[p] for p in perm], [inits[p] for p in perm])
    ta = run(ks + [12], inits)
    for b in range(4):
        for other in (tp[perm.index(b)], ta[b]):
            for key in ("W", "H") + TRACE_KEYS + ("holdout_mse", "holdout_mkl"):
                assert np.array_equal(other[key], base[b][key]), (b, key)
            assert other["n_iteration"] == base[b]["n_iteration"]


@pytest.mark.parametrize("trace", [1, 3])
def test_each_member_stops_on_its_own_rule(trace):
    """Strict mode, rel_tol = 1e-4: n_iteration and trace lengths are the solo run's; equal factors show a frozen member did not move."""
    ks = [2, 6, 3, 10, 1]
    A, ptr, idx, inits = problem(130, 90, ks, 0.1, 21)
    inits = [(w * s, x * s) for (w, x), s in zip(inits, [1.0, 0.02, 3.0, 0.3, 0.01])]
    An = cv.with_nan(A, ptr, idx)
    t, _ = batch(_lib.PREC_F64, A, ptr, idx, ks, inits, Z3, Z3, 300, 1e-4, 1, trace)
    its = set()
    for b, k in enumerate(ks):
        s = solo_na(_lib.PREC_F64, An, k, *inits[b], Z3, Z3, 300, 1e-4, 1, trace)
        assert t[b]["n_iteration"] == s["n_iteration"] and len(t[b]["target_error"]) == len(s["target_error"])
        assert t[b]["warning"] == s["warning"]
        check_member(t[b], s, 1e-10, True)
        its.add(t[b]["n_iteration"])
    assert len(its) >= 2, its


@pytest.mark.parametrize("pname,prec,tol", MODES)
def test_empty_holdout_is_the_plain_batch(pname, prec, tol):
    ks = [3, 6, 2]
    A, _, _, inits = problem(120, 90, ks, 0.1, 2)
    ptr, idx = np.zeros(91, dtype=np.int64), np.zeros(0, dtype=np.int32)
    t, _ = batch(prec, A, ptr, idx, ks, inits, Z3, Z3, 6, -1.0, 1, 2)
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix(A)
        h.set_factors_batch(ks, [w for w, _ in inits], [x for _, x in inits])
        p = h.run_batch(Z3, Z3, 6, -1.0, 0, True, 50, 1e-9, 1, 2)
        f = h.get_factors_batch()
    for b in range(3):
        assert np.array_equal(t[b]["W"], f[b][0]) and np.array_equal(t[b]["H"], f[b][1])
        for key in TRACE_KEYS:
            assert np.array_equal(t[b][key], p[b][key])
        assert np.isnan(t[b]["holdout_mse"]) and np.isnan(t[b]["holdout_mkl"])


def test_refusals():
    A, ptr, idx, inits = problem(60, 50, [2, 3], 0.1, 0)
    W, H = [w for w, _ in inits], [x for _, x in inits]

    def code(fn):
        with pytest.raises(_lib.NnlmError) as e:
            fn()
        return e.value.code

    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
        h.set_matrix_holdout(A, ptr, idx)
        h.set_factors_batch([2, 3], W, H)
        for method in (3, 4):
            assert code(lambda: h.run_batch(Z3, Z3, 3, -1.0, 0, True, 1, 1e-9, method, 1)) == ERR_UNSUPPORTED
        assert code(lambda: h.comm_init(None, 0, 2)) == ERR_UNSUPPORTED
        assert code(lambda: h.set_factors_batch([33, 32])) == ERR_UNSUPPORTED
    for bad in (np.nan, -np.inf):
        Ab = A.copy()
        Ab[5, 7] = bad
        with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
            with pytest.raises(_lib.NnlmError, match=r"A\[5, 7\]") as e:
                h.set_matrix_holdout(Ab, ptr, idx)
            assert e.value.code == ERR_ARG
    c0 = int(np.argmax(np.diff(ptr) >= 2))  # a column with two held-out entries
    swapped, dup, out = idx.copy(), idx.copy(), idx.copy()
    swapped[ptr[c0]], swapped[ptr[c0] + 1] = idx[ptr[c0] + 1], idx[ptr[c0]]
    dup[ptr[c0] + 1] = dup[ptr[c0]]
    out[0] = 60
    badptr = ptr.copy()
    badptr[3] = badptr[2] - 1 if badptr[2] > 0 else badptr[4] + 1
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
        for p, i in ((ptr, swapped), (ptr, dup), (ptr, out), (badptr, idx)):
            assert code(lambda: h.set_matrix_holdout(A, p, i)) == ERR_ARG
        h.set_matrix(A)
        h.set_factors(2, W[0], H[0])
        assert code(lambda: h.holdout_errors()) == ERR_ARG  # a plain handle
    An = cv.with_nan(A, ptr, idx)
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:  # missing entries that came in through set_matrix stay refused
        h.set_matrix(An)
        assert code(lambda: h.set_factors_batch([2, 3], W, H)) == ERR_UNSUPPORTED
    assert code(lambda: _lib.c_nnmf_holdout_batch(A, ptr, idx, [2, 3], W, H, Z3, Z3, 3, -1.0, 1, 0, True, 1, 1e-9, 3, 1)) == ERR_UNSUPPORTED


@pytest.mark.parametrize("pname,prec,tol", MODES)
def test_end_to_end_rank_choice(monkeypatch, pname, prec, tol):
    """api.nnmf_cv on the planted-rank input: best is the planted rank, the held-out errors are the oracle's; two batches = one."""
    monkeypatch.setenv("NNLM_PRECISION", pname)
    strict = pname == "f64"
    ks = list(range(1, 13))
    A, inits = cv.planted(ks)
    init = [{"W": w, "H": x} for w, x in inits]
    opts = dict(max_iter=cv.ITERS, rel_tol=-1.0, trace=cv.TRACE, show_warning=False)
    r6 = api.nnmf_cv(A, range(1, 7), holdout=cv.FRACTION, rng=np.random.default_rng(cv.SEED), init=init[:6], **opts)
    ptr, idx = r6["holdout"]["indptr"], r6["holdout"]["indices"]
    want = api._holdout_pattern(cv.FRACTION, cv.N, cv.M, np.random.default_rng(cv.SEED))
    assert np.array_equal(ptr, want[0]) and np.array_equal(idx, want[1])
    cv.assert_trainable(A, ptr, idx, 12)
    assert r6["k"] == list(range(1, 7)) and r6["k"][r6["best"]] == cv.RANK, (r6["best"], r6["holdout_mse"])
    An = cv.with_nan(A, ptr, idx)
    for b, k in enumerate(r6["k"]):
        o = oracle(An, k, *inits[b], Z3, Z3, cv.ITERS, -1.0, 1, cv.TRACE)
        om = cv.numpy_holdout_errors(A, ptr, idx, o["W"], o["H"])[0]
        bound = tol
        if not strict:
            s = solo_na(prec, An, k, *inits[b], Z3, Z3, cv.ITERS, -1.0, 1, cv.TRACE)
            bound = max(tol, 1.01 * relF(s["W"], o["W"]), 1.01 * relF(s["H"], o["H"]))
        print("   k=%d held-out mse %.6e oracle %.6e rel %.2e (bound %.1e)" % (k, r6["holdout_mse"][b], om, abs(r6["holdout_mse"][b] - om) / om, bound))
        assert abs(r6["holdout_mse"][b] - om) <= bound * om, (k, r6["holdout_mse"][b], om)
        assert r6["fits"][b]["holdout_mse"] == r6["holdout_mse"][b] and r6["fits"][b]["W"].shape == (cv.N, k)
    # sum k = 78: two batches on one handle; the members the two calls share agree at the strict bound
    r12 = api.nnmf_cv(A, range(1, 13), holdout=r6["holdout"], init=init, **opts)
    assert r12["k"] == ks and len(r12["fits"]) == 12
    for b in range(6):
        lim = 1e-10 if strict else 1e-5
        assert relF(r12["fits"][b]["W"], r6["fits"][b]["W"]) < lim and relF(r12["fits"][b]["H"], r6["fits"][b]["H"]) < lim
        assert abs(r12["holdout_mse"][b] - r6["holdout_mse"][b]) <= lim * r6["holdout_mse"][b]
    # the one-shot C entry gives the first batch's members
    out = _lib.c_nnmf_holdout_batch(A, ptr, idx, ks[:6], [w for w, _ in inits[:6]], [x for _, x in inits[:6]], Z3, Z3, cv.ITERS, -1.0, 1, 0,
                                    False, 50, 1e-9, 1, cv.TRACE)
    for b in range(6):
        lim = 1e-10 if strict else 1e-5
        assert relF(out[b]["W"], r6["fits"][b]["W"]) < lim and abs(out[b]["holdout_mse"] - r6["holdout_mse"][b]) <= lim * r6["holdout_mse"][b]


@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("B", [1, 8])
def test_one_pass_over_A_whatever_B_is(pname, prec, tol, B):
    ks = [4] * B
    A, ptr, idx, inits = problem(200, 150, ks, 0.1, 4)
    t, p = batch(prec, A, ptr, idx, ks, inits, Z3, Z3, 6, -1.0, 1, 2, prof=True)
    ntr = len(t[0]["mse_error"])
    assert ntr == 4
    assert p["batch_errors"][1] == ntr and p["errors"][1] == 0, p
    assert p["xprod_h"][1] == 6 and p["xprod_w"][1] == 6, p


@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("seed", range(max(1, int(os.environ.get("NNLM_FUZZ_SEEDS", "150")) // 25)))
def test_random_slice(pname, prec, tol, seed):
    """Shapes 40-400, random batches, 2-40 % held out (subject to the training-entry assertion), both methods, random penalties."""
    rng = np.random.default_rng(1000 + seed)
    n, m = (int(v) for v in rng.integers(40, 401, size=2))
    frac = float(rng.uniform(0.02, 0.4))
    # ranks the hold-out fraction leaves room for: k + 1 observed entries in the sparsest row and column, with a margin
    kcap = max(1, min(16, int(0.4 * (1 - frac) * min(n, m)) - 1))
    B = int(rng.integers(1, 7))
    ks = [int(v) for v in rng.integers(1, kcap + 1, size=B)]
    while sum(ks) > 64:
        ks.pop()
    method = int(rng.integers(1, 3))
    alpha = [float(rng.choice([0.0, 0.05])), 0.0, float(rng.choice([0.0, 0.01]))]
    beta = [float(rng.choice([0.0, 0.05])), 0.0, float(rng.choice([0.0, 0.01]))]
    A, ptr, idx, inits = problem(n, m, ks, frac, 2000 + seed)
    print("case", n, m, "frac %.2f" % frac, ks, "method", method, alpha, beta)
    check_all(prec, pname, tol, A, ptr, idx, ks, inits, alpha, beta, int(rng.integers(3, 9)), method, int(rng.integers(1, 4)))
