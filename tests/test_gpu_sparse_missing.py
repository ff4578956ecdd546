"""Sparse A whose absent entries are MISSING (nnlm_set_matrix_csc_missing, k_sparse_na.h) on the MI355X against the fp64 oracle run on the
densified matrix with NaN at the absent entries (update_with_missing / the oracle's nnmf), against the dense NA path on the same data,
and beyond what the dense NA path can hold.  CSC structures are built with numpy only.  Run with `pytest -m gpu`.

Bounds (those of test_gpu_sparse.py): strict fp64 mode 1e-10 with exact sweep counts; fp32-operand mode 1e-4 (the measured value is in
the failure message)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import relF  # noqa: E402
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402
from oracle import nnlm_oracle, ref  # noqa: E402

pytestmark = pytest.mark.gpu

PRECS = [("f64", _lib.PREC_F64, 1e-10), ("f32", _lib.PREC_F32, 1e-4)]
ERR_ARG, ERR_UNSUPPORTED = 1, 5


@pytest.fixture(autouse=True)
def _default_precision(monkeypatch):
    monkeypatch.delenv("NNLM_PRECISION", raising=False)


def csc_from_flat(flat, vals, n, m):
    """CSC from sorted, unique column-major flat indices j * n + i."""
    flat = np.asarray(flat, dtype=np.int64)
    cols, rows = flat // n, flat % n
    indptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=m), out=indptr[1:])
    return indptr, rows.astype(np.int32), np.asarray(vals, dtype=np.float64), (n, m)


def rand_csc(n, m, density, rng):
    nnz = int(round(density * n * m))
    flat = np.sort(rng.choice(n * m, size=nnz, replace=False)) if nnz < n * m else np.arange(n * m)
    return csc_from_flat(flat, rng.random(flat.size), n, m)


def nan_dense(csc):
    """The matrix the oracle sees: stored entries (zeros included) in place, NaN at the absent ones."""
    indptr, idx, val, (n, m) = csc
    A = np.full((n, m), np.nan)
    A[idx, np.repeat(np.arange(m), np.diff(indptr))] = val
    return A


def err(a, b):
    """Relative Frobenius error, absolute where the reference is (close to) zero."""
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1.0))


def rand_mask(shape, rng, frac=0.15):
    return rng.random(shape) < frac


class Csc:
    """numpy-only duck-typed sparse matrix (what api.nnmf accepts from scipy)."""

    def __init__(self, csc):
        self.indptr, self.indices, self.data, self.shape = csc

    def tocsc(self):
        return self


def half_steps(prec, S, k, W0, H0, Wm, Hm, reg, inner, method):
    """One W and one H half-step on a fresh handle -> W1, H1, sweeps of each."""
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix_csc_missing(*S)
        h.set_factors(k, W0, H0, Wm, Hm)
        h.half_step(0, reg, inner, 1e-9, method)
        W1, _ = h.get_factors()
        s1 = h.take_sweeps()
        h.half_step(1, reg, inner, 1e-9, method)
        _, H1 = h.get_factors()
        s2 = h.take_sweeps()
    return W1, H1, s1, s2


def check_half_steps(pname, prec, tol, S, k, method, reg, rng, masks=True, inner=5, what=""):
    A = nan_dense(S)
    n, m = A.shape
    miss = bool(np.isnan(A).any())
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    Wm, Hm = (rand_mask((n, k), rng), rand_mask((k, m), rng)) if masks else (None, None)
    W1, H1, s1, s2 = half_steps(prec, S, k, W0, H0, Wm, Hm, reg, inner, method)
    Wt_ref, it1 = ref.update(W0.T.copy(), H0, A.T.copy(), None if Wm is None else Wm.T.copy(), reg, inner, 1e-9, method, missing=miss)
    # (strict: the oracle's own W, as the dense tests do -- sweep counts stay exact; fp32: the W this half-step actually had fixed)
    H_ref, it2 = ref.update(H0, Wt_ref if pname == "f64" else W1.T.copy(), A, Hm, reg, inner, 1e-9, method, missing=miss)
    ew, eh = err(W1, Wt_ref.T), err(H1, H_ref)
    assert ew <= tol and eh <= tol, f"{pname} {what}: W {ew:.3e}, H {eh:.3e} (bound {tol:g})"
    assert np.all(W1 >= 0) and np.all(H1 >= 0)
    if masks:
        assert np.array_equal(W1[Wm], W0[Wm]) and np.array_equal(H1[Hm], H0[Hm])
    if pname == "f64":
        assert (s1, s2) == (it1, it2), what


# ---- 1. single half-steps against update_with_missing -----------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", PRECS)
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("density", [0.02, 0.3, 1.0])
@pytest.mark.parametrize("shape", [(200, 100, 5), (257, 129, 17), (515, 131, 50), (64, 700, 64), (150, 90, 16), (33, 1, 1)])
def test_half_steps_match_oracle(pname, prec, tol, method, density, shape):
    n, m, k = shape
    rng = np.random.default_rng(n + 7 * m + 13 * k + method + int(1000 * density))
    S = rand_csc(n, m, density, rng)
    check_half_steps(pname, prec, tol, S, k, method, [0.02, 0.01, 0.03], rng, what=f"method {method} {shape} density {density}")


@pytest.mark.parametrize("pname,prec,tol", PRECS)
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("reg", [[0.0, 0.0, 0.0], [0.05, 0.0, 0.0], [0.0, 0.02, 0.0], [0.0, 0.0, 0.04]])
def test_penalty_positions(pname, prec, tol, method, reg):
    rng = np.random.default_rng(11 + method + int(100 * sum(reg)))
    S = rand_csc(300, 170, 0.08, rng)
    check_half_steps(pname, prec, tol, S, 12, method, reg, rng, what=f"reg {reg}")


# ---- 2. whole runs: the oracle's nnmf on the NaN-dense matrix, and the dense NA path --------------------------------------------------------
@pytest.mark.parametrize("pname,tol", [("f64", 1e-10), ("f32", 1e-4)])
def test_api_nnmf_matches_oracle_nnmf(monkeypatch, pname, tol):
    if pname == "f32":
        monkeypatch.setenv("NNLM_PRECISION", "f32")
    n, m, k = 400, 300, 4
    rng = np.random.default_rng(4)
    S = rand_csc(n, m, 0.08, rng)
    W0 = rng.random((n, 1))  # a known profile
    mask = {"H": rand_mask((k, m), rng)}
    kw = dict(init={"W0": W0}, mask=mask, max_iter=20, rel_tol=1e-12, inner_max_iter=10, alpha=[0.0, 0.0, 0.01], beta=[0.01, 0, 0],
              check_k=False)
    args, ctx = api.prepare_nnmf(Csc(S), k, rng=np.random.default_rng(0), verbose=0, absent="missing", **kw)
    A = nan_dense(args[0])
    o = ref.c_nnmf(A, *args[1:])
    g = _lib.c_nnmf_csc_missing(*args[0], *args[1:])  # the argument tuple api.nnmf() hands over, without host callbacks
    ew, eh = relF(g["W"], o["W"]), relF(g["H"], o["H"])
    assert ew <= tol and eh <= tol, f"{pname}: W {ew:.3e}, H {eh:.3e}"
    assert g["n_iteration"] == o["n_iteration"] == 20 and g["warning"] == o["warning"]
    for key in ("mse_error", "mkl_error", "target_error"):
        d = np.max(np.abs(g[key] - o[key]) / np.abs(o[key]))
        assert len(g[key]) == len(o[key]) and d <= tol, f"{pname} {key}: {d:.3e}"
    if pname == "f64":
        assert np.array_equal(g["average_epoch"], o["average_epoch"])
    # the wrapper end to end (its unif_rand callback included) on the sparse matrix and on the same matrix dense with NaN
    r = api.nnmf(Csc(S), k, rng=np.random.default_rng(0), absent="missing", **kw)
    rd = api.nnmf(nan_dense(S), k, rng=np.random.default_rng(0), **kw)
    ew, eh = relF(r["W"], rd["W"]), relF(r["H"], rd["H"])
    assert ew <= tol and eh <= tol and r["options"]["absent"] == "missing", f"{pname} api sparse vs dense NA: W {ew:.3e}, H {eh:.3e}"
    assert r["n_iteration"] == rd["n_iteration"] == 20
    assert np.array_equal(r["W"][:, k], W0[:, 0])  # the known profile stays fixed


@pytest.mark.parametrize("pname,prec,tol", PRECS)
def test_run_matches_dense_na_path(pname, prec, tol):
    n, m, k = 3000, 2000, 20
    rng = np.random.default_rng(2)
    S = rand_csc(n, m, 0.02, rng)
    A = nan_dense(S)
    W0, H0 = rng.random((n, k)) * 0.1, rng.random((k, m)) * 0.1
    alpha, beta = [0.01, 0.0, 0.001], [0.0, 0.002, 0.0]
    outs = []
    for sparse in (False, True):
        with nnlm_amd.Handle(0, prec) as h:
            h.set_matrix_csc_missing(*S) if sparse else h.set_matrix(A)
            h.set_factors(k, W0, H0)
            r = h.run(alpha, beta, 20, 1e-300, 0, False, 50, 1e-9, 1, 2)
            r["W"], r["H"] = h.get_factors()
            outs.append(r)
    d, s = outs
    ew, eh = relF(s["W"], d["W"]), relF(s["H"], d["H"])
    assert ew <= tol and eh <= tol, f"{pname}: W {ew:.3e}, H {eh:.3e}"
    assert s["n_iteration"] == d["n_iteration"] == 20
    for key in ("mse_error", "mkl_error", "target_error"):
        dd = np.max(np.abs(s[key] - d[key]) / np.abs(d[key]))
        assert dd <= tol, f"{pname} {key}: {dd:.3e}"
    # (the two paths sum each Gram in a different order: a column whose stopping test sits at the rounding edge may take one sweep more
    #  or less -- against the oracle, whose Grams are the reference's, the sweep counts are exact: test_half_steps_match_oracle)
    de = np.max(np.abs(s["average_epoch"] - d["average_epoch"]) / d["average_epoch"])
    assert de <= 1e-3, de


# ---- 3. explicit zeros are observations -----------------------------------------------------------------------------------------------------
def test_explicit_zeros_are_observations():
    n, m, k = 250, 160, 6
    rng = np.random.default_rng(3)
    indptr, idx, val, shp = rand_csc(n, m, 0.15, rng)
    val = val.copy()
    zero = rng.random(val.size) < 0.3
    val[zero] = 0.0
    S = (indptr, idx, val, shp)
    keep = ~zero  # the same matrix with its stored zeros dropped
    cols = np.repeat(np.arange(m), np.diff(indptr))
    S_nz = csc_from_flat(cols[keep] * n + idx[keep], val[keep], n, m)
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    reg = [0.01, 0.0, 0.0]
    res = []
    for T in (S, S_nz):
        with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
            h.set_matrix_csc_missing(*T)
            assert h.matrix_info()["n_non_missing"] == T[1].size
            h.set_factors(k, W0, H0)
            h.iterate(3, reg, reg, 10, 1e-9, 1)
            res.append(h.get_factors())
    Wr, Hr = W0.T.copy(), H0.copy()
    A = nan_dense(S)
    assert np.sum(A == 0.0) == zero.sum()
    for _ in range(3):
        Wr, _ = ref.update(Wr, Hr, A.T.copy(), None, reg, 10, 1e-9, 1, missing=True)
        Hr, _ = ref.update(Hr, Wr, A, None, reg, 10, 1e-9, 1, missing=True)
    assert err(res[0][0], Wr.T) <= 1e-10 and err(res[0][1], Hr) <= 1e-10, (err(res[0][0], Wr.T), err(res[0][1], Hr))
    assert relF(res[1][1], res[0][1]) > 1e-3  # dropping the zeros changes the fit


# ---- 4. edge structure ---------------------------------------------------------------------------------------------------------------------
def empty_lines_csc(rng):
    """60 x 45 at 30 %, with rows 0, 7, 59 and columns 0, 10, 44 left empty."""
    n, m = 60, 45
    obs = rng.random((n, m)) < 0.3
    obs[[0, 7, 59], :] = False
    obs[:, [0, 10, 44]] = False
    flat = np.flatnonzero(obs.T.ravel())
    return csc_from_flat(flat, rng.random(flat.size), n, m)


def heavy_column_csc(rng, n=4000, m=4000):
    """Column 5 fully observed (half of all entries), every other column one entry at a random row."""
    rows = rng.integers(0, n, m)
    rows[5] = -1
    flat = [j * n + rows[j] for j in range(m) if j != 5] + [5 * n + i for i in range(n)]
    flat = np.sort(np.array(flat, dtype=np.int64))
    return csc_from_flat(flat, rng.random(flat.size) + 0.1, n, m)


@pytest.mark.parametrize("pname,prec,tol", PRECS)
@pytest.mark.parametrize("case", ["empty_lines", "heavy_column", "heavy_row"])
def test_edge_structure_half_steps(pname, prec, tol, case):
    rng = np.random.default_rng({"empty_lines": 21, "heavy_column": 22, "heavy_row": 23}[case])
    if case == "empty_lines":
        S, k = empty_lines_csc(rng), 4
    else:
        S, k = heavy_column_csc(rng), 16
        if case == "heavy_row":  # the transpose: one row holding half of all entries (the W half-step's CSR has the long line)
            A = nan_dense(S).T
            flat = np.flatnonzero(~np.isnan(A.T.ravel()))
            S = csc_from_flat(flat, A.T.ravel()[flat], A.shape[0], A.shape[1])
    for method in (1, 2):
        check_half_steps(pname, prec, tol, S, k, method, [0.01, 0.0, 0.0], rng, masks=False, what=f"{case} method {method}")


@pytest.mark.parametrize("pname,prec,tol", PRECS)
def test_empty_lines_full_run(pname, prec, tol):
    rng = np.random.default_rng(24)
    S = empty_lines_csc(rng)
    A = nan_dense(S)
    n, m = A.shape
    k = 3
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix_csc_missing(*S)
        h.set_factors(k, W0, H0)
        r = h.run([0, 0, 0], [0, 0, 0], 6, 1e-300, 0, False, 5, 1e-9, 1, 2)
        W, H = h.get_factors()
    o = ref.c_nnmf(A, k, W0, H0, None, None, [0, 0, 0], [0, 0, 0], 6, 1e-300, 1, 0, False, 5, 1e-9, 1, 2)
    assert err(W, o["W"]) <= tol and err(H, o["H"]) <= tol, (err(W, o["W"]), err(H, o["H"]))
    assert r["n_iteration"] == o["n_iteration"]
    assert np.all(W[[0, 7, 59]] == 0) and np.all(H[:, [0, 10, 44]] == 0)  # nothing observed: the solution is 0, as in the reference


@pytest.mark.parametrize("pname,prec,tol", PRECS)
def test_nothing_stored(pname, prec, tol):
    n, m, k = 50, 40, 3
    rng = np.random.default_rng(25)
    S = csc_from_flat(np.zeros(0, dtype=np.int64), np.zeros(0), n, m)
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix_csc_missing(*S)
        info = h.matrix_info()
        h.set_factors(k, W0, H0)
        r = h.run([0, 0, 0], [0, 0, 0], 5, 1e-4, 0, False, 5, 1e-9, 1, 1)
        W, H = h.get_factors()
    o = ref.c_nnmf(nan_dense(S), k, W0, H0, None, None, [0, 0, 0], [0, 0, 0], 5, 1e-4, 1, 0, False, 5, 1e-9, 1, 1)
    assert info["n_non_missing"] == 0 and info["any_missing"]
    # (nothing observed: x - (TINY x) / TINY, the reference's step, is 0 up to a rounding of x)
    assert np.max(np.abs(W)) <= 1e-15 * np.max(W0) and np.max(np.abs(H)) <= 1e-15 * np.max(H0)
    if pname == "f64":
        assert np.array_equal(W, o["W"]) and np.array_equal(H, o["H"])
    assert r["n_iteration"] == o["n_iteration"]
    assert np.array_equal(np.isnan(r["mse_error"]), np.isnan(o["mse_error"]))


# ---- 5. chunked Grams, determinism --------------------------------------------------------------------------------------------------------
def chunk_case(rng):
    """3000 x 2000 at 1.5 %, plus a fully observed column and row (segments across chunks and workers)."""
    n, m = 3000, 2000
    obs = rng.random((n, m)) < 0.015
    obs[:, 17] = True
    obs[1234, :] = True
    flat = np.flatnonzero(obs.T.ravel())
    return csc_from_flat(flat, rng.random(flat.size), n, m)


def chunk_run(prec, S, k, W0, H0, limit):
    _lib.debug_alloc_limit(limit)
    try:
        with nnlm_amd.Handle(0, prec) as h:
            h.set_matrix_csc_missing(*S)
            h.set_factors(k, W0, H0)
            r = h.run([0.01, 0, 0], [0, 0, 0.01], 4, 1e-300, 0, False, 20, 1e-9, 1, 1)
            chunks = h.get_info("sp_gram_chunks")  # (of the last half-step: H)
            gbytes = h.get_info("sp_gram_bytes")
            W, H = h.get_factors()
    finally:
        _lib.debug_alloc_limit(0)
    return W, H, r, chunks, gbytes


@pytest.mark.parametrize("pname,prec,tol", PRECS)
def test_chunked_grams_match_unchunked(pname, prec, tol):
    rng = np.random.default_rng(26)
    S = chunk_case(rng)
    n, m = S[3]
    k = 16
    W0, H0 = rng.random((n, k)) * 0.1, rng.random((k, m)) * 0.1
    W1, H1, r1, c1, b1 = chunk_run(prec, S, k, W0, H0, 0)
    limit = 600 * 16 * 16 * 8  # 600 Gram slots: >= 3 chunks of the 2000 H columns
    W2, H2, r2, c2, b2 = chunk_run(prec, S, k, W0, H0, limit)
    assert c1 == 1 and c2 >= 3 and b2 <= limit, (c1, c2, b2)
    if pname == "f64":
        assert np.array_equal(W1, W2) and np.array_equal(H1, H2)
        assert all(np.array_equal(r1[key], r2[key]) for key in ("mse_error", "mkl_error", "target_error", "average_epoch"))
    else:
        assert relF(W2, W1) <= 1e-6 and relF(H2, H1) <= 1e-6, (relF(W2, W1), relF(H2, H1))


@pytest.mark.parametrize("pname,prec,tol", PRECS)
def test_runs_are_bit_identical(pname, prec, tol):
    rng = np.random.default_rng(27)
    S = heavy_column_csc(rng, 3000, 2500)
    n, m = S[3]
    k = 17
    W0, H0 = rng.random((n, k)) * 0.1, rng.random((k, m)) * 0.1
    res = []
    for _ in range(2):
        with nnlm_amd.Handle(0, prec) as h:
            h.set_matrix_csc_missing(*S)
            h.set_factors(k, W0, H0)
            r = h.run([0, 0, 0], [0.01, 0, 0], 6, 1e-300, 0, False, 20, 1e-9, 1, 2)
            res.append(h.get_factors() + (r,))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert all(np.array_equal(res[0][2][key], res[1][2][key]) for key in ("mse_error", "mkl_error", "target_error", "average_epoch"))


# ---- 6. switching semantics on one handle, matrix_info / get_info, refusals ---------------------------------------------------------------
def code_of(fn, *a):
    with pytest.raises(_lib.NnlmError) as ei:
        fn(*a)
    return ei.value.code, str(ei.value)


@pytest.mark.parametrize("pname,prec,tol", PRECS)
def test_switching_semantics_on_one_handle(pname, prec, tol):
    n, m, k = 180, 120, 5
    rng = np.random.default_rng(28)
    S = rand_csc(n, m, 0.1, rng)
    A0, An = np.nan_to_num(nan_dense(S)), nan_dense(S)
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    reg = [0.01, 0.0, 0.0]
    with nnlm_amd.Handle(0, prec) as h:
        for miss, A in ((False, A0), (True, An)):
            h.set_matrix_csc_missing(*S) if miss else h.set_matrix_csc(*S)
            assert h.get_info("matrix_absent_missing") == float(miss)
            h.set_factors(k, W0, H0)
            h.half_step(1, reg, 10, 1e-9, 1)
            _, H1 = h.get_factors()
            H_ref, _ = ref.update(H0, W0.T.copy(), A, None, reg, 10, 1e-9, 1, missing=miss)
            assert err(H1, H_ref) <= tol, (miss, err(H1, H_ref))
        h.set_matrix(An)
        assert h.get_info("matrix_absent_missing") == 0.0


def test_matrix_info_and_get_info():
    n, m = 90, 70
    rng = np.random.default_rng(29)
    S = rand_csc(n, m, 0.2, rng)
    val = S[2]
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
        h.set_matrix_csc_missing(*S)
        info = h.matrix_info()
        assert h.get_info("matrix_nnz") == val.size and h.get_info("matrix_absent_missing") == 1.0
        h.set_matrix_csc_missing(*rand_csc(n, m, 1.0, rng))
        full = h.matrix_info()
    klc = float(np.mean((val + 1e-16) * np.log(val + 1e-16) - val))  # src/nnmf.cpp:70, over the stored entries
    assert info["n_non_missing"] == val.size and info["any_missing"] and abs(info["kl_const"] - klc) <= 1e-12 * abs(klc)
    assert full["n_non_missing"] == n * m and not full["any_missing"]


@pytest.mark.parametrize("pname,prec,tol", PRECS)
def test_refusals(pname, prec, tol):
    n, m, k = 150, 90, 4
    rng = np.random.default_rng(30)
    S = rand_csc(n, m, 0.1, rng)
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix_csc_missing(*S)
        code, msg = code_of(h.set_factors, 65)
        assert code == ERR_UNSUPPORTED and "rank" in msg
        h.set_factors(k, rng.random((n, k)), rng.random((k, m)))
        for method in (3, 4):
            code, msg = code_of(h.half_step, 1, [0, 0, 0], 5, 1e-9, method)
            assert code == ERR_UNSUPPORTED and "KL" in msg
            code, msg = code_of(h.run, [0, 0, 0], [0, 0, 0], 3, 1e-4, 0, False, 1, 1e-9, method, 1)
            assert code == ERR_UNSUPPORTED and "KL" in msg
        code, msg = code_of(h.debug_partial, 1)
        assert code == ERR_UNSUPPORTED and "sparse" in msg
        code, msg = code_of(h.set_factors_batch, [2, 3])
        assert code == ERR_UNSUPPORTED and "batched" in msg
        code, msg = code_of(h.comm_init, None, 0, 2)
        assert code == ERR_UNSUPPORTED and "sparse" in msg
        ptr, idx, val, shp = S
        bad = val.copy()
        bad[2] = np.nan
        code, msg = code_of(h.set_matrix_csc_missing, ptr, idx, bad, shp)
        assert code == ERR_ARG and "nnlm_set_matrix_csc_missing" in msg


# ---- 7. fold-in: nnlm / predict_nnmf with a sparse y whose absent entries are missing ---------------------------------------------------
@pytest.mark.parametrize("pname,tol", [("f64", 1e-10), ("f32", 1e-4)])
def test_fold_in_matches_oracle(monkeypatch, pname, tol):
    if pname == "f32":
        monkeypatch.setenv("NNLM_PRECISION", "f32")
    n, q, p = 400, 250, 6
    rng = np.random.default_rng(31)
    S = rand_csc(n, q, 0.06, rng)
    Y = nan_dense(S)
    x = rng.random((n, p))
    B0 = rng.random((p, q))
    for method, mname in ((1, "scd"), (2, "lee")):
        fit = api.nnlm(x, Csc(S), method=mname, init=B0, max_iter=200, rel_tol=1e-12, absent="missing", alpha=[0.01, 0, 0])
        B_ref, it = ref.update(B0, x.T.copy(), Y, None, [0.01, 0, 0], 200, 1e-12, method, missing=True)
        e = relF(fit["coefficients"], B_ref)
        assert e <= tol, f"{pname} {mname}: {e:.3e}"
        assert fit["n_iteration"] == it or pname == "f32"
        obs = ~np.isnan(Y)
        assert fit["error"]["MSE"] == pytest.approx(float(np.mean((Y[obs] - (x @ fit["coefficients"])[obs]) ** 2)), rel=1e-12)
    model = {"W": x, "H": B0, "options": {"method": "scd", "loss": "mse", "absent": "missing"}}
    Bh = rng.random((p, q))
    pr = api.predict_nnmf(model, Csc(S), which="H", absent="missing", init=Bh, max_iter=200, rel_tol=1e-12)
    pref, _ = ref.update(Bh, x.T.copy(), Y, None, [0, 0, 0], 200, 1e-12, 1, missing=True)
    assert relF(pr["coefficients"], pref) <= tol


# ---- 8. beyond the dense NA path -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def huge():
    n, m, nnz = 2_000_000, 50_000, 5_000_000
    rng = np.random.default_rng(7)
    flat = np.unique(rng.integers(0, n * m, size=nnz + 4000, dtype=np.int64))[:nnz]  # (the last few columns stay empty)
    return csc_from_flat(flat, rng.random(flat.size), n, m)


@pytest.mark.parametrize("pname,prec,tol", PRECS)
def test_beyond_dense_2e6_by_5e4(huge, pname, prec, tol):
    indptr, idx, val, (n, m) = huge
    nnz, k = val.size, 8
    cols = np.repeat(np.arange(m), np.diff(indptr))
    rng = np.random.default_rng(8)
    W0, H0 = rng.random((n, k)) * 1e-4, rng.random((k, m))
    reg, inner = [0.01, 0.0, 0.0], 10
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix_csc_missing(*huge)
        es = 8 if prec == _lib.PREC_F64 else 4
        # (the dense NA path would hold n m = 1e11 entries, and a per-column Gram buffer of max(n, m) KP^2 8 = 4 GB)
        assert h.get_info("matrix_bytes") <= 3 * nnz * (4 + es) + 40 * (n + m)
        h.set_factors(k, W0, H0)
        h.half_step(0, reg, inner, 1e-9, 1)
        W1, _ = h.get_factors()
        assert h.get_info("sp_gram_chunks") >= 4 and h.get_info("sp_gram_bytes") <= 2 ** 30  # (2e6 W rows x 2 KiB in 1 GiB chunks)
        h.half_step(1, reg, inner, 1e-9, 1)
        _, H1 = h.get_factors()
        h.iterate(2, reg, reg, inner, 1e-9, 1)
        mse, _, _ = h.errors()
        W3, H3 = h.get_factors()
    assert np.all(np.isfinite(W3)) and np.all(np.isfinite(H3)) and np.isfinite(mse)
    # sampled H columns against a host solve over their stored rows (fixed factor W1, what the half-step had)
    cols_s = np.sort(rng.choice(m - 10, 64, replace=False))
    Href = np.empty((k, 64))
    for t, j in enumerate(cols_s):
        rows = idx[indptr[j]:indptr[j + 1]]
        Wj = W1[rows]
        G = nnlm_oracle._gram_edits(Wj.T @ Wj, reg)
        x = H0[:, j].copy()
        mu = G @ x - Wj.T @ val[indptr[j]:indptr[j + 1]]
        nnlm_oracle.scd_ls_update(x, G, mu, None, inner, 1e-9)
        Href[:, t] = x
    eh = relF(H1[:, cols_s], Href)
    assert eh <= tol, f"{pname}: H columns {eh:.3e}"
    # the error block over the stored entries: mse = mean (a - wh)^2 over them
    wh = np.einsum("ek,ek->e", W3[idx], H3.T[cols])
    mse_ref = float(np.mean(((val if pname == "f64" else val.astype(np.float32).astype(np.float64)) - wh) ** 2))  # (what the mode stores)
    assert abs(mse - mse_ref) <= 1e-9 * mse_ref, (mse, mse_ref)
