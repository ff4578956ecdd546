"""Per-entry weights on a sparse A, host side (no GPU): the reference helper pinned to the oracle at weights 1, the three new C entries
(declared, listed, exported), the refusals of `weights` in nnmf() / nnlm(), the alignment rules of the two forms of `weights`, the
weighted error summary of nnlm() and predict_nnmf()'s hand-over."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nnlm_amd import _lib, api  # noqa: E402
from oracle import nnlm_oracle  # noqa: E402
import weighted_cases as wc  # noqa: E402
from weighted_cases import Csc  # noqa: E402

NEW = ("nnlm_set_matrix_csc_weighted", "nnlm_c_nnmf_csc_weighted", "nnlm_c_nnlm_csc_weighted")
REG = [0.02, 0.01, 0.03]


def relmax(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(float(np.max(np.abs(b))), 1e-300))


def nan_dense(S):
    indptr, idx, val, (n, m) = S
    A = np.full((n, m), np.nan)
    A[idx, np.repeat(np.arange(m), np.diff(indptr))] = val
    return A


# ---- the helper equals the oracle when every weight is 1 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("absent", ["zero", "missing"])
@pytest.mark.parametrize("method", [1, 2])
def test_helper_half_steps_equal_the_oracle_at_weights_one(absent, method):
    n, m, k = 40, 23, 4
    rng = np.random.default_rng(1 + method)
    S = wc.rand_csc(n, m, 0.3, rng)
    A, C, obs = wc.dense_parts(S, np.ones(S[2].size), absent)
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    Wm, Hm = rng.random((n, k)) < 0.15, rng.random((k, m)) < 0.15
    missing = absent == "missing"
    Ao = nan_dense(S) if missing else A
    upd = nnlm_oracle.update_with_missing if missing else nnlm_oracle.update
    Wt_o, H_o = W0.T.copy(), H0.copy()
    it1 = upd(Wt_o, H_o, np.ascontiguousarray(Ao.T), Wm.T.astype(np.int64), REG, 5, 1e-9, method)
    it2 = upd(H_o, Wt_o, Ao, Hm.astype(np.int64), REG, 5, 1e-9, method)
    Wt_h, s1 = wc.half_step(W0.T, H0, A.T, C.T, obs.T, Wm.T, REG, 5, 1e-9, method, missing)
    H_h, s2 = wc.half_step(H0, Wt_h, A, C, obs, Hm, REG, 5, 1e-9, method, missing)
    assert relmax(Wt_h, Wt_o) <= 1e-12 and relmax(H_h, H_o) <= 1e-12, (relmax(Wt_h, Wt_o), relmax(H_h, H_o))
    assert (s1, s2) == (it1, it2)


@pytest.mark.parametrize("absent", ["zero", "missing"])
def test_helper_full_run_equals_the_oracle_at_weights_one(absent):
    n, m, k = 30, 20, 3
    rng = np.random.default_rng(3)
    S = wc.rand_csc(n, m, 0.4, rng)
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    alpha, beta = [0.01, 0.0, 0.001], [0.0, 0.002, 0.01]
    Ao = nan_dense(S) if absent == "missing" else np.nan_to_num(nan_dense(S))
    o = nnlm_oracle.c_nnmf(Ao, k, W0, H0, None, None, alpha, beta, 9, 1e-300, 1, 0, False, 5, 1e-9, 1, 2)
    g = wc.c_nnmf(S, np.ones(S[2].size), absent, k, W0, H0, None, None, alpha, beta, 9, 1e-300, 5, 1e-9, 1, 2)
    assert g["n_iteration"] == o["n_iteration"] == 9 and len(g["mse_error"]) == len(o["mse_error"])
    for key in ("W", "H", "mse_error", "mkl_error", "target_error"):
        assert relmax(g[key], o[key]) <= 1e-12, (key, relmax(g[key], o[key]))
    assert np.array_equal(g["average_epoch"], o["average_epoch"])


def test_helper_weights_change_the_fit():
    """(the pin above would also hold for a helper that ignored its weights)"""
    n, m, k = 30, 20, 3
    rng = np.random.default_rng(4)
    S = wc.rand_csc(n, m, 0.4, rng)
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    w = 1.0 + 40.0 * rng.random(S[2].size)
    for absent in ("zero", "missing"):
        A, C, obs = wc.dense_parts(S, w, absent)
        H1, _ = wc.half_step(H0, W0.T, A, C, obs, None, [0, 0, 0], 200, 1e-12, 1, absent == "missing")
        # the weighted normal equations of one column, solved directly where the solution is interior
        j = int(np.argmax(np.all(H1 > 1e-8, axis=0)))
        G = (W0.T * C[:, j]) @ W0 + 1e-16 * np.eye(k)
        b = W0.T @ (C[:, j] * A[:, j])
        if np.all(H1[:, j] > 1e-8):
            assert np.allclose(H1[:, j], np.linalg.solve(G, b), rtol=1e-6, atol=1e-9)
        A1, C1, obs1 = wc.dense_parts(S, np.ones(w.size), absent)
        H2, _ = wc.half_step(H0, W0.T, A1, C1, obs1, None, [0, 0, 0], 200, 1e-12, 1, absent == "missing")
        assert relmax(H1, H2) > 1e-3


# ---- the C entries ------------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "nnlm_mi355x.h")).read()
    for sym in NEW:
        assert re.search(r"\bint " + sym + r"\s*\(", header), sym
        assert sym in _lib.EXPORTS
        assert hasattr(_lib.load(), sym)
    assert "sparse_weighted" in header
    for name in ("c_nnmf_csc_weighted", "c_nnlm_csc_weighted"):
        assert callable(getattr(_lib, name))
    assert hasattr(_lib.Handle, "set_matrix_csc_weighted")


# ---- refusals of `weights` -----------------------------------------------------------------------------------------------------------------
class FakeDeviceTensor:
    """What _lib.is_device_array takes for a tensor in device memory."""
    shape, dtype = (6, 5), "float64"

    class device:
        type, index = "cuda", 0

    def data_ptr(self):
        return 0

    def stride(self):
        return (5, 1)


class FakeSparseDeviceTensor(FakeDeviceTensor):
    layout = "torch.sparse_csc"


def small(rng=None, n=12, m=9, density=0.4):
    rng = rng or np.random.default_rng(5)
    return wc.rand_csc(n, m, density, rng)


def test_nnmf_refuses_weights_by_name():
    S = small()
    w = np.ones(S[2].size)
    with pytest.raises(api.NnlmStop, match="weights need a sparse A"):
        api.nnmf(np.ones((12, 9)), 2, weights=np.ones((12, 9)))
    for T in (FakeDeviceTensor(), FakeSparseDeviceTensor()):
        with pytest.raises(api.NnlmStop, match="weights cannot be combined with a A in device memory"):
            api.nnmf(T, 2, weights=w)
    with pytest.raises(api.NnlmStop, match="loss = 'mse' only"):
        api.nnmf(Csc(S), 2, loss="mkl", weights=w)
    with pytest.raises(api.NnlmStop, match="loss = 'mse' only"):
        api.nnmf(Csc(S), 2, sparse_kl=True, weights=w)
    for init in ("nndsvd", "nndsvda"):
        with pytest.raises(api.NnlmStop, match="weights cannot be combined with init"):
            api.nnmf(Csc(S), 2, init=init, weights=w)


def test_nnlm_refuses_weights_by_name():
    S = small()
    x = np.random.default_rng(6).random((12, 3))
    w = np.ones(S[2].size)
    with pytest.raises(api.NnlmStop, match="weights need a sparse y"):
        api.nnlm(x, np.ones((12, 9)), weights=np.ones((12, 9)))
    with pytest.raises(api.NnlmStop, match="device memory"):
        api.nnlm(x, FakeDeviceTensor(), weights=w)
    with pytest.raises(api.NnlmStop, match="loss = 'mse' only"):
        api.nnlm(x, Csc(S), loss="mkl", weights=w)
    with pytest.raises(api.NnlmStop, match="loss = 'mse' only"):
        api.nnlm(x, Csc(S), sparse_kl=True, weights=w)


def test_batch_and_cv_take_no_weights():
    import inspect
    for fn in (api.nnmf_batch, api.nnmf_cv):
        assert "weights" not in inspect.signature(fn).parameters
    S = small()
    with pytest.raises((api.NnlmStop, TypeError)):
        api.nnmf_batch(Csc(S), [2, 3], sparse_batch=True, weights=np.ones(S[2].size))


# ---- alignment of `weights` with the stored entries -----------------------------------------------------------------------------------------
def test_weights_as_a_sparse_matrix_must_have_the_pattern_of_A():
    S = small()
    indptr, idx, val, shp = S
    c = api.as_csc(Csc(S))
    w = 1.0 + np.arange(val.size, dtype=float)
    assert np.array_equal(api._weights_arg(Csc((indptr, idx, w, shp)), Csc(S), c, "nnmf"), w)
    # one entry of column 4 moved to another row: column 4 is the first that differs
    j = 4
    assert indptr[j + 1] > indptr[j]
    col = idx[indptr[j]:indptr[j + 1]]
    free = np.setdiff1d(np.arange(shp[0]), col)[0]
    idx2 = idx.copy()
    seg = np.sort(np.concatenate([col[1:], [free]])).astype(np.int32)
    idx2[indptr[j]:indptr[j + 1]] = seg
    with pytest.raises(api.NnlmStop, match=r"first in column 4\b"):
        api._weights_arg(Csc((indptr, idx2, w, shp)), Csc(S), c, "nnmf")
    # one stored entry fewer in column 2
    keep = np.ones(val.size, dtype=bool)
    keep[indptr[2]] = False
    ptr3 = indptr.copy()
    ptr3[3:] -= 1
    with pytest.raises(api.NnlmStop, match=r"first in column 2\b"):
        api._weights_arg(Csc((ptr3, idx[keep], w[keep], shp)), Csc(S), c, "nnmf")
    with pytest.raises(api.NnlmStop, match="weights is 9 x 12"):
        api._weights_arg(Csc(S).T, Csc(S), c, "nnmf")
    # unsorted weights of the same pattern are made canonical like A
    order = np.arange(val.size)
    a, b = indptr[j], indptr[j + 1]
    order[a:b] = order[a:b][::-1]
    got = api._weights_arg(Csc((indptr, idx[order], w[order], shp)), Csc(S), c, "nnmf")
    assert np.array_equal(got, w)


def test_weights_as_an_array_need_a_canonical_A():
    S = small()
    indptr, idx, val, shp = S
    c = api.as_csc(Csc(S))
    w = np.linspace(0.0, 3.0, val.size)
    assert np.array_equal(api._weights_arg(w, Csc(S), c, "nnmf"), w)
    with pytest.raises(api.NnlmStop, match="one weight per stored entry"):
        api._weights_arg(w[:-1], Csc(S), c, "nnmf")
    with pytest.raises(api.NnlmStop, match="one weight per stored entry"):
        api._weights_arg(np.ones((2, val.size)), Csc(S), c, "nnmf")
    # A with the rows of one column stored in descending order: as_csc re-orders
    j = 4
    order = np.arange(val.size)
    order[indptr[j]:indptr[j + 1]] = order[indptr[j]:indptr[j + 1]][::-1]
    U = Csc((indptr, idx[order], val[order], shp))
    with pytest.raises(api.NnlmStop, match="not canonical"):
        api._weights_arg(w, U, api.as_csc(U), "nnmf")
    # A with a duplicate entry: as_csc merges (and the canonical matrix then stores one entry fewer)
    ptr2 = indptr.copy()
    ptr2[j + 1:] += 1
    at = indptr[j]
    D = Csc((ptr2, np.insert(idx, at, idx[at]), np.insert(val, at, 0.5), shp))
    cd = api.as_csc(D)
    assert cd.data.size == val.size
    with pytest.raises(api.NnlmStop, match="not canonical"):
        api._weights_arg(w, D, cd, "nnmf")
    for bad in (-1.0, np.nan, np.inf):
        wb = w.copy()
        wb[3] = bad
        with pytest.raises(api.NnlmStop, match="finite and >= 0"):
            api._weights_arg(wb, Csc(S), c, "nnmf")


# ---- nnlm()'s weighted summary, predict_nnmf()'s hand-over ---------------------------------------------------------------------------------
@pytest.mark.parametrize("absent", ["zero", "missing"])
def test_nnlm_summary_uses_the_weighted_sums(absent):
    rng = np.random.default_rng(7)
    n, q, p = 25, 7, 3
    S = wc.rand_csc(n, q, 0.4, rng)
    w = rng.choice([0.0, 0.25, 1.0, 3.5], S[2].size)
    x, coef = rng.random((n, p)), rng.random((p, q))
    _, ctx = api.prepare_nnlm(x, Csc(S), absent=absent, check_x=False)
    ctx["weights"] = w
    res = api.finish_nnlm({"coefficient": coef, "n_iteration": 3}, ctx)
    A, C, obs = wc.dense_parts(S, w, absent)
    N = float(S[2].size) if absent == "missing" else float(n * q)
    mse, kl = wc.errors(A, C, obs, x.T, coef, N)
    assert res["error"]["MSE"] == pytest.approx(mse, rel=1e-12)
    assert res["error"]["MKL"] == pytest.approx(wc.kl_const(S, w, absent) + kl, rel=1e-10)
    assert res["error"]["target.error"] == pytest.approx(0.5 * mse, rel=1e-12)


def test_predict_passes_weights_to_the_solver():
    obj = {"W": np.ones((30, 2)), "H": np.ones((2, 20)), "options": {"method": "scd", "loss": "mse"}}
    seen = {}

    def fake(x, y, **kw):
        seen.update(kw)
        return {"coefficients": np.zeros((x.shape[1], y.shape[1]))}
    rng = np.random.default_rng(8)
    nd = wc.rand_csc(30, 7, 0.3, rng)
    w = np.ones(nd[2].size)
    api.predict_nnmf(obj, Csc(nd), which="H", absent="missing", weights=w, _nnlm=fake)
    assert seen.get("weights") is w and seen.get("absent") == "missing"
    seen.clear()
    api.predict_nnmf(obj, Csc(nd), which="H", _nnlm=fake)
    assert "weights" not in seen  # (the default: today's call)
    rows = wc.rand_csc(5, 20, 0.3, rng)
    with pytest.raises(api.NnlmStop, match="which = 'H'"):
        api.predict_nnmf(obj, Csc(rows), which="W", weights=np.ones(rows[2].size), _nnlm=fake)
    assert api.predict_nnmf(obj, which="A", weights=w).shape == (30, 20)  # (W H: nothing is solved)
