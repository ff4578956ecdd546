"""Sparse A (nnlm_set_matrix_csc, k_sparse.h) on the MI355X against the fp64 oracle on the densified matrix, against the dense path, and
beyond what a dense matrix can hold.  CSC structures are built with numpy only.  Run with `pytest -m gpu`.

Bounds: strict fp64 mode 1e-10 with exact sweep counts; fp32-operand mode 1e-4 for both factors (the measured worst case is printed in
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


def rand_csc(n, m, density, rng):
    """(indptr, indices, data, shape) of a random n x m matrix with round(density n m) non-zeros in U(0, 1)."""
    nnz = int(round(density * n * m))
    flat = np.sort(rng.choice(n * m, size=nnz, replace=False)) if nnz < n * m else np.arange(n * m)
    return csc_from_flat(flat, rng.random(flat.size), n, m)


def csc_from_flat(flat, vals, n, m):
    """CSC from sorted, unique column-major flat indices j * n + i."""
    cols, rows = flat // n, flat % n
    indptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=m), out=indptr[1:])
    return indptr, rows.astype(np.int32), np.asarray(vals, dtype=np.float64), (n, m)


def dense(csc):
    indptr, idx, val, (n, m) = csc
    A = np.zeros((n, m))
    A[idx, np.repeat(np.arange(m), np.diff(indptr))] = val
    return A


def err(a, b):
    """Relative Frobenius error, absolute where the reference is (close to) zero."""
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1.0))


def rand_mask(shape, rng, frac=0.15):
    return rng.random(shape) < frac


# ---- 1. single half-steps against the oracle on the densified matrix -----------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", PRECS)
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("density", [0.0, 0.01, 0.2, 1.0])
@pytest.mark.parametrize("shape", [(200, 100, 5), (257, 129, 17), (515, 131, 50), (64, 700, 64), (33, 1, 1), (300, 200, 80)])
def test_half_steps_match_oracle(pname, prec, tol, method, density, shape):
    n, m, k = shape
    rng = np.random.default_rng(n + 7 * m + 13 * k + method + int(1000 * density))
    S = rand_csc(n, m, density, rng)
    A = dense(S)
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    Wm, Hm = rand_mask((n, k), rng), rand_mask((k, m), rng)
    reg = [0.02, 0.01, 0.03]
    inner = 5
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix_csc(*S)
        h.set_factors(k, W0, H0, Wm, Hm)
        h.half_step(0, reg, inner, 1e-9, method)
        W1, _ = h.get_factors()
        s1 = h.take_sweeps()
        Wt_ref, it1 = ref.update(W0.T.copy(), H0, A.T.copy(), Wm.T.copy(), reg, inner, 1e-9, method, missing=False)
        ew = err(W1, Wt_ref.T)
        h.half_step(1, reg, inner, 1e-9, method)
        _, H1 = h.get_factors()
        s2 = h.take_sweeps()
        # (strict: the oracle's own W, as the dense tests do -- sweep counts stay exact; fp32: the W this half-step actually had fixed)
        H_ref, it2 = ref.update(H0, Wt_ref if pname == "f64" else W1.T.copy(), A, Hm, reg, inner, 1e-9, method, missing=False)
        eh = err(H1, H_ref)
    assert ew <= tol and eh <= tol, f"{pname} method {method} {shape} density {density}: W {ew:.3e}, H {eh:.3e} (bound {tol:g})"
    assert np.all(W1 >= 0) and np.all(H1 >= 0)
    assert np.array_equal(W1[Wm], W0[Wm]) and np.array_equal(H1[Hm], H0[Hm])
    if pname == "f64":
        assert (s1, s2) == (it1, it2)


# ---- 2. strict sparse against strict dense, whole runs ---------------------------------------------------------------------------------
def test_strict_sparse_run_matches_strict_dense_run():
    n, m, k = 3000, 2000, 20
    rng = np.random.default_rng(2)
    S = rand_csc(n, m, 0.02, rng)
    A = dense(S)
    W0, H0 = rng.random((n, k)) * 0.1, rng.random((k, m)) * 0.1
    alpha, beta = [0.01, 0.0, 0.001], [0.0, 0.0, 0.0]
    outs = []
    for sparse in (False, True):
        with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
            h.set_matrix_csc(*S) if sparse else h.set_matrix(A)
            h.set_factors(k, W0, H0)
            r = h.run(alpha, beta, 30, 1e-300, 0, False, 50, 1e-9, 1, 2)
            r["W"], r["H"] = h.get_factors()
            outs.append(r)
    d, s = outs
    assert relF(s["W"], d["W"]) <= 1e-10 and relF(s["H"], d["H"]) <= 1e-10, (relF(s["W"], d["W"]), relF(s["H"], d["H"]))
    assert s["n_iteration"] == d["n_iteration"] == 30
    assert np.array_equal(s["average_epoch"], d["average_epoch"])
    for key in ("mkl_error", "target_error"):
        assert np.all(np.abs(s[key] - d[key]) <= 1e-10 * np.abs(d[key])), (key, np.max(np.abs(s[key] - d[key]) / np.abs(d[key])))
    bound = 1e-12 * np.mean(A * A) + 1e-10 * d["mse_error"]
    assert np.all(np.abs(s["mse_error"] - d["mse_error"]) <= bound), np.max(np.abs(s["mse_error"] - d["mse_error"]) / bound)


# ---- 3. near-exact fit: the sum of squares at its worst cancellation ------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", PRECS)
def test_error_block_of_a_near_exact_fit(pname, prec, tol):
    n, m, k = 700, 500, 6
    rng = np.random.default_rng(3)
    Ws = rng.random((n, k)) * (rng.random((n, k)) < 0.08)
    Hs = rng.random((k, m)) * (rng.random((k, m)) < 0.08)
    A = Ws @ Hs
    if prec == _lib.PREC_F32:
        A = A.astype(np.float32).astype(np.float64)  # (what the fp32 mode stores)
    flat = np.flatnonzero(A.T.ravel())
    S = csc_from_flat(flat, A.T.ravel()[flat], n, m)
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix_csc(*S)
        h.set_factors(k, Ws, Hs)
        mse, kl, _ = h.errors()
        info = h.matrix_info()
    mse_ref, kl_ref = nnlm_oracle._errors(A, Ws.T, Hs, None, False)
    assert abs(mse - mse_ref) <= 1e-12 * np.mean(A * A) + 1e-10 * mse_ref, (mse, mse_ref)
    assert abs(kl - kl_ref) <= 1e-10 * abs(kl_ref) + 4e-15, (kl, kl_ref)
    assert info["n_non_missing"] == n * m and not info["any_missing"]
    with np.errstate(divide="ignore", invalid="ignore"):
        klc = float(np.mean((A + 1e-16) * np.log(A + 1e-16) - A))
    assert abs(info["kl_const"] - klc) <= 1e-12 * abs(klc)


# ---- 4. the Python API against the oracle --------------------------------------------------------------------------------------------
class Csc:
    """numpy-only duck-typed sparse matrix (what api.nnmf accepts from scipy)."""

    def __init__(self, csc):
        self.indptr, self.indices, self.data, self.shape = csc

    def tocsc(self):
        return self

    @property
    def T(self):
        A = dense((self.indptr, self.indices, self.data, self.shape)).T
        flat = np.flatnonzero(A.T.ravel())
        return Csc(csc_from_flat(flat, A.T.ravel()[flat], A.shape[0], A.shape[1]))


@pytest.mark.parametrize("pname,tol", [("f64", 1e-10), ("f32", 1e-4)])
def test_api_nnmf_nnlm_predict_match_oracle(monkeypatch, pname, tol):
    if pname == "f32":
        monkeypatch.setenv("NNLM_PRECISION", "f32")
    n, m, k = 400, 300, 4
    rng = np.random.default_rng(4)
    S = rand_csc(n, m, 0.05, rng)
    A = dense(S)
    W0 = rng.random((n, 1))  # a known profile
    mask = {"H": rand_mask((k, m), rng)}
    kw = dict(init={"W0": W0}, mask=mask, max_iter=20, rel_tol=1e-12, inner_max_iter=10, beta=[0.01, 0, 0])
    args, ctx = api.prepare_nnmf(Csc(S), k, rng=np.random.default_rng(0), verbose=0, **kw)
    o = ref.c_nnmf(dense(args[0]), *args[1:])
    g = _lib.c_nnmf_csc(*args[0], *args[1:])  # the argument tuple api.nnmf() hands over, without host callbacks
    ew, eh = relF(g["W"], o["W"]), relF(g["H"], o["H"])
    assert ew <= tol and eh <= tol, f"{pname}: W {ew:.3e}, H {eh:.3e}"
    assert g["n_iteration"] == o["n_iteration"] == 20
    assert np.all(np.abs(g["mse_error"] - o["mse_error"]) <= (1e-4 if pname == "f32" else 1e-10) * o["mse_error"])
    # the wrapper end to end (its unif_rand callback included) on the sparse matrix and on the same matrix dense
    r = api.nnmf(Csc(S), k, rng=np.random.default_rng(0), **kw)
    rd = api.nnmf(A, k, rng=np.random.default_rng(0), **kw)
    ew, eh = relF(r["W"], rd["W"]), relF(r["H"], rd["H"])
    assert ew <= tol and eh <= tol, f"{pname} api sparse vs dense: W {ew:.3e}, H {eh:.3e}"
    assert r["n_iteration"] == rd["n_iteration"] == 20
    assert np.array_equal(r["W"][:, k], W0[:, 0])  # the known profile stays fixed

    x = rng.random((n, 3))
    B0 = rng.random((3, m))
    fit = api.nnlm(x, Csc(S), init=B0, max_iter=200, rel_tol=1e-12)
    oref = ref.c_nnlm(x, A, [0, 0, 0], None, B0, 200, 1e-12, 1, 1)
    assert relF(fit["coefficients"], oref["coefficient"]) <= tol
    assert fit["n_iteration"] == oref["n_iteration"] or pname == "f32"
    assert fit["error"]["MSE"] == pytest.approx(float(np.mean((A - x @ fit["coefficients"]) ** 2)), rel=1e-12)

    model = {"W": r["W"], "H": r["H"], "options": r["options"]}
    Bh = rng.random((k + 1, m))
    pr = api.predict_nnmf(model, Csc(S), which="H", init=Bh, max_iter=200, rel_tol=1e-12)
    pref = ref.c_nnlm(r["W"], A, [0, 0, 0], None, Bh, 200, 1e-12, 1, 1)
    assert relF(pr["coefficients"], pref["coefficient"]) <= tol


# ---- 5. determinism, including power-law columns / rows --------------------------------------------------------------------------------
def heavy_line_csc(n, m, which, rng):
    """About half of all non-zeros in one column (which = "col") or one row ("row"), the rest spread at random."""
    A = np.zeros((n, m))
    if which == "col":
        A[:, 3] = rng.random(n) + 0.1
        extra = n
    else:
        A[5, :] = rng.random(m) + 0.1
        extra = m
    fl = rng.choice(n * m, size=extra, replace=False)
    A[fl % n, fl // n] = rng.random(extra) + 0.1
    At = A.T.ravel()  # (column-major flat copy of A)
    flat = np.flatnonzero(At)
    return csc_from_flat(flat, At[flat], n, m), A


@pytest.mark.parametrize("pname,prec,tol", PRECS)
@pytest.mark.parametrize("which,n,m,k", [("col", 20000, 300, 16), ("row", 300, 20000, 16), ("col", 20000, 200, 50), ("row", 200, 9000, 32)])
def test_runs_are_bit_identical_and_heavy_lines_match_oracle(pname, prec, tol, which, n, m, k):
    rng = np.random.default_rng(5)
    S, A = heavy_line_csc(n, m, which, rng)
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    reg = [0.01, 0.0, 0.0]
    res = []
    for _ in range(2):
        with nnlm_amd.Handle(0, prec) as h:
            h.set_matrix_csc(*S)
            h.set_factors(k, W0, H0)
            h.half_step(1, reg, 5, 1e-9, 1)  # H half-step: CSC (heavy column)
            h.half_step(0, reg, 5, 1e-9, 1)  # W half-step: CSR (heavy row)
            h.iterate(2, reg, reg, 5, 1e-9, 2)
            W, H = h.get_factors()
            res.append((W, H, h.errors()[0]))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and res[0][2] == res[1][2]
    with nnlm_amd.Handle(0, prec) as h:  # the straddled columns / rows against the oracle (one half-step each)
        h.set_matrix_csc(*S)
        h.set_factors(k, W0, H0)
        h.half_step(1, reg, 5, 1e-9, 1)
        _, H1 = h.get_factors()
        h.half_step(0, reg, 5, 1e-9, 1)
        W1, _ = h.get_factors()
    H_ref, _ = ref.update(H0, W0.T.copy(), A, None, reg, 5, 1e-9, 1, missing=False)
    Wt_ref, _ = ref.update(W0.T.copy(), H1 if pname == "f32" else H_ref, A.T.copy(), None, reg, 5, 1e-9, 1, missing=False)
    eh, ew = err(H1, H_ref), err(W1, Wt_ref.T)
    bh = bw = tol
    if pname == "f32":
        # the fp32 SCD chain (k_sweep_f.h) errs in proportion to how far a column moves from a cold start: on these 20000-long
        # contractions the DENSE path exceeds 1e-4 on the same half-steps too.  The sparse path must add nothing to it.
        with nnlm_amd.Handle(0, prec) as h:
            h.set_matrix(A)
            h.set_factors(k, W0, H0)
            h.half_step(1, reg, 5, 1e-9, 1)
            _, H1d = h.get_factors()
            h.half_step(0, reg, 5, 1e-9, 1)
            W1d, _ = h.get_factors()
        Wt_refd, _ = ref.update(W0.T.copy(), H1d, A.T.copy(), None, reg, 5, 1e-9, 1, missing=False)
        bh, bw = max(tol, 1.5 * err(H1d, H_ref)), max(tol, 1.5 * err(W1d, Wt_refd.T))
    assert eh <= bh and ew <= bw, f"{pname} {which}: H {eh:.3e} (bound {bh:.3e}), W {ew:.3e} (bound {bw:.3e})"


# ---- 6. refusals, switching, edges ---------------------------------------------------------------------------------------------------
def code_of(fn, *a):
    with pytest.raises(_lib.NnlmError) as ei:
        fn(*a)
    return ei.value.code


@pytest.mark.parametrize("pname,prec,tol", PRECS)
def test_refusals_and_switching(pname, prec, tol):
    rng = np.random.default_rng(6)
    n, m, k = 150, 90, 4
    S = rand_csc(n, m, 0.1, rng)
    A = dense(S)
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix_csc(*S)
        assert h.get_info("matrix_nnz") == S[1].size
        h.set_factors(k, W0, H0)
        for method in (3, 4):
            assert code_of(h.half_step, 1, [0, 0, 0], 5, 1e-9, method) == ERR_UNSUPPORTED
            assert code_of(h.run, [0, 0, 0], [0, 0, 0], 3, 1e-4, 0, False, 1, 1e-9, method, 1) == ERR_UNSUPPORTED
        assert code_of(h.comm_init, None, 0, 2) == ERR_UNSUPPORTED
        assert code_of(h.debug_partial, 1) == ERR_UNSUPPORTED
        ptr, idx, val, shp = S
        bad_val = val.copy()
        bad_val[3] = np.nan
        assert code_of(h.set_matrix_csc, ptr, idx, bad_val, shp) == ERR_ARG
        bad_val[3] = np.inf
        assert code_of(h.set_matrix_csc, ptr, idx, bad_val, shp) == ERR_ARG
        j = int(np.argmax(np.diff(ptr)))
        swapped = idx.copy()
        swapped[ptr[j]], swapped[ptr[j] + 1] = idx[ptr[j] + 1], idx[ptr[j]]
        assert code_of(h.set_matrix_csc, ptr, swapped, val, shp) == ERR_ARG  # unsorted
        dup = idx.copy()
        dup[ptr[j] + 1] = dup[ptr[j]]
        assert code_of(h.set_matrix_csc, ptr, dup, val, shp) == ERR_ARG  # duplicate
        oob = idx.copy()
        oob[0] = n
        assert code_of(h.set_matrix_csc, ptr, oob, val, shp) == ERR_ARG
        badp = ptr.copy()
        badp[0] = 1
        assert code_of(h.set_matrix_csc, badp, idx, val, shp) == ERR_ARG
        badp = ptr.copy()
        badp[1] = ptr[-1]
        assert code_of(h.set_matrix_csc, badp, idx, val, shp) == ERR_ARG  # (colptr decreases)
        # dense -> sparse -> dense on one handle equals fresh handles
        seq = []
        for use_sparse in (False, True, False):
            h.set_matrix_csc(*S) if use_sparse else h.set_matrix(A)
            h.set_factors(k, W0, H0)
            h.iterate(2, [0, 0, 0], [0, 0, 0], 5, 1e-9, 1)
            seq.append(h.get_factors() + (h.get_info("matrix_nnz"), h.get_info("matrix_bytes")))
    for use_sparse, got in zip((False, True, False), seq):
        with nnlm_amd.Handle(0, prec) as f:
            f.set_matrix_csc(*S) if use_sparse else f.set_matrix(A)
            f.set_factors(k, W0, H0)
            f.iterate(2, [0, 0, 0], [0, 0, 0], 5, 1e-9, 1)
            fresh = f.get_factors() + (f.get_info("matrix_nnz"), f.get_info("matrix_bytes"))
        assert np.array_equal(got[0], fresh[0]) and np.array_equal(got[1], fresh[1]) and got[2:] == fresh[2:]
    assert seq[0][2] == -1 and seq[1][2] == S[1].size and seq[1][3] < seq[0][3]


@pytest.mark.parametrize("pname,prec,tol", PRECS)
@pytest.mark.parametrize("n,m,k,density", [(120, 80, 3, 0.0), (1, 50, 1, 0.5), (60, 1, 1, 0.5), (1, 1, 1, 1.0), (40, 30, 1, 0.2)])
def test_edges(pname, prec, tol, n, m, k, density):
    rng = np.random.default_rng(n * 31 + m)
    S = rand_csc(n, m, density, rng)
    A = dense(S)
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix_csc(*S)
        h.set_factors(k, W0, H0)
        r = h.run([0, 0, 0], [0, 0, 0], 6, 1e-300, 0, False, 5, 1e-9, 1, 2)
        W, H = h.get_factors()
    Wr, Hr = W0.T.copy(), H0.copy()
    for _ in range(6):
        nnlm_oracle.update(Wr, Hr, A.T.copy(), None, [0, 0, 0], 5, 1e-9, 1)
        nnlm_oracle.update(Hr, Wr, A, None, [0, 0, 0], 5, 1e-9, 1)
    assert err(W, Wr.T) <= tol and err(H, Hr) <= tol, (err(W, Wr.T), err(H, Hr))
    assert np.all(np.isfinite(r["mse_error"])) and 1 <= r["n_iteration"] <= 6  # (A = 0: the run stops once the target stops moving)


# ---- 7. beyond dense ---------------------------------------------------------------------------------------------------------------
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
    # (W0 random at the scale of the solution -- about 2.5 non-zeros per row against a Gram of 1e4: W1 ~ 1e-4.  From U(0, 1) the fp32
    #  SCD chain of the F32 mode would cancel four digits away on every row, dense or sparse alike; the strict mode does not care.)
    W0, H0 = rng.random((n, k)) * 1e-4, rng.random((k, m))
    reg, inner = [0.01, 0.0, 0.0], 10
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix_csc(*huge)
        es = 8 if prec == _lib.PREC_F64 else 4
        assert h.get_info("matrix_nnz") == nnz
        assert h.get_info("matrix_bytes") <= 3 * nnz * (4 + es) + 16 * (n + m)
        h.set_factors(k, W0, H0)
        h.half_step(0, reg, inner, 1e-9, 1)
        W1, _ = h.get_factors()
        h.half_step(1, reg, inner, 1e-9, 1)
        _, H1 = h.get_factors()
        h.iterate(2, reg, reg, inner, 1e-9, 1)
        W3, H3 = h.get_factors()
    assert np.all(np.isfinite(W3)) and np.all(np.isfinite(H3))
    rows_s = np.sort(rng.choice(n, 256, replace=False))
    cols_s = np.sort(rng.choice(m, 256, replace=False))
    # W rows: fixed factor H0; cross product A H0^T of the sampled rows by bincount over the structure
    pos = np.full(n, -1)
    pos[rows_s] = np.arange(256)
    sel = pos[idx] >= 0
    Cw = np.stack([np.bincount(pos[idx[sel]], weights=val[sel] * H0[q, cols[sel]], minlength=256) for q in range(k)])
    G = nnlm_oracle._gram_edits(H0 @ H0.T, reg)
    Wref = np.empty((256, k))
    for t, i in enumerate(rows_s):
        x = W0[i].copy()
        mu = G @ x - Cw[:, t]
        nnlm_oracle.scd_ls_update(x, G, mu, None, inner, 1e-9)
        Wref[t] = x
    # H columns: fixed factor W1 (what the half-step had)
    pos = np.full(m, -1)
    pos[cols_s] = np.arange(256)
    sel = pos[cols] >= 0
    Ch = np.stack([np.bincount(pos[cols[sel]], weights=val[sel] * W1[idx[sel], q], minlength=256) for q in range(k)])
    G = nnlm_oracle._gram_edits(W1.T @ W1, reg)
    Href = np.empty((k, 256))
    for t, j in enumerate(cols_s):
        x = H0[:, j].copy()
        mu = G @ x - Ch[:, t]
        nnlm_oracle.scd_ls_update(x, G, mu, None, inner, 1e-9)
        Href[:, t] = x
    ew, eh = relF(W1[rows_s], Wref), relF(H1[:, cols_s], Href)
    assert ew <= tol and eh <= tol, f"{pname}: W rows {ew:.3e}, H columns {eh:.3e}"
