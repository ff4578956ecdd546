"""Per-entry weights on a sparse A (nnlm_set_matrix_csc_weighted, k_sparse_na.h / k_sparse.h) on the MI355X against the reference of
weighted_cases.py: the C oracle's update() / update_with_missing() on the one-column problems whose rows are scaled by sqrt(c), and the
oracle's outer loop restated around it.  absent = "missing": weighted NMF over the stored entries; absent = "zero": every entry is an
observation and an absent one is a zero of weight 1 (implicit feedback).  Run with `pytest -m gpu`.

Bounds (those of test_gpu_sparse_missing.py): strict fp64 mode 1e-10 with exact sweep counts; fp32-operand mode 1e-4 (the measured value
is in the failure message).  A reference is computed once per case and shared by the two modes: both half-steps of a case start from the
same (W0, H0), so the reference does not depend on what the GPU returned."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import relF  # noqa: E402
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402
import weighted_cases as wc  # noqa: E402
from weighted_cases import Csc, csc_from_flat, rand_csc  # noqa: E402

pytestmark = pytest.mark.gpu

PRECS = [("f64", _lib.PREC_F64, 1e-10), ("f32", _lib.PREC_F32, 1e-4)]
ABSENT = ["zero", "missing"]
ERR_ARG, ERR_UNSUPPORTED = 1, 5
REG = [0.02, 0.01, 0.03]


@pytest.fixture(autouse=True)
def _default_precision(monkeypatch):
    monkeypatch.delenv("NNLM_PRECISION", raising=False)


def err(a, b):
    """Relative Frobenius error, absolute where the reference is (close to) zero."""
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1.0))


def make_weights(absent, size, rng, kind=None):
    """zero semantics: confidences 1 + 40 u; missing: {0, 0.25, 1, 3.5} (exact zeros and weights below 1); "below_one": (0, 1)."""
    if kind == "below_one":
        return 0.05 + 0.9 * rng.random(size)
    if absent == "zero":
        return 1.0 + 40.0 * rng.random(size)
    return rng.choice([0.0, 0.25, 1.0, 3.5], size)


def set_weighted(h, S, w, absent):
    h.set_matrix_csc_weighted(S[0], S[1], S[2], w, S[3], absent_missing=absent == "missing")


def gpu_half_steps(prec, S, w, absent, k, W0, H0, Wm, Hm, reg, inner, method):
    """The W half-step and the H half-step, each from (W0, H0), on one handle -> W1, H1 and the sweeps of each."""
    with nnlm_amd.Handle(0, prec) as h:
        set_weighted(h, S, w, absent)
        h.set_factors(k, W0, H0, Wm, Hm)
        h.half_step(0, reg, inner, 1e-9, method)
        W1, _ = h.get_factors()
        s1 = h.take_sweeps()
        h.set_factors(k, W0, H0, Wm, Hm)
        h.half_step(1, reg, inner, 1e-9, method)
        _, H1 = h.get_factors()
        s2 = h.take_sweeps()
    return W1, H1, s1, s2


_REF = {}


def ref_half_steps(key, S, w, absent, W0, H0, Wm, Hm, reg, inner, method):
    """The helper's two half-steps from (W0, H0), computed once per case."""
    if key not in _REF:
        A, C, obs = wc.dense_parts(S, w, absent)
        missing = absent == "missing"
        At, Ct, obst = (np.ascontiguousarray(x.T) for x in (A, C, obs))
        Wt, it1 = wc.half_step(W0.T, H0, At, Ct, obst, None if Wm is None else Wm.T, reg, inner, 1e-9, method, missing)
        H1, it2 = wc.half_step(H0, W0.T, A, C, obs, Hm, reg, inner, 1e-9, method, missing)
        _REF[key] = (Wt.T.copy(), H1, it1, it2)
    return _REF[key]


def check_half_steps(key, pname, prec, tol, S, w, absent, k, method, reg, rng_seed, masks=True, inner=5):
    n, m = S[3]
    rng = np.random.default_rng(rng_seed)
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    Wm, Hm = (rng.random((n, k)) < 0.15, rng.random((k, m)) < 0.15) if masks else (None, None)
    W1, H1, s1, s2 = gpu_half_steps(prec, S, w, absent, k, W0, H0, Wm, Hm, reg, inner, method)
    W_ref, H_ref, it1, it2 = ref_half_steps(key, S, w, absent, W0, H0, Wm, Hm, reg, inner, method)
    ew, eh = err(W1, W_ref), err(H1, H_ref)
    print(f"{key} {pname}: W {ew:.3e}, H {eh:.3e}, sweeps {(s1, s2)} ref {(it1, it2)}")
    assert ew <= tol and eh <= tol, f"{pname} {key}: W {ew:.3e}, H {eh:.3e} (bound {tol:g})"
    assert np.all(W1 >= 0) and np.all(H1 >= 0)
    if masks:
        assert np.array_equal(W1[Wm], W0[Wm]) and np.array_equal(H1[Hm], H0[Hm])
    # Sweep counts, strict mode: exact for absent = "missing".  For absent = "zero" they are printed only: the Gram is the shared one plus
    # a weighted sum, the reference's is one sum over sqrt(c)-scaled rows, and a line WITHOUT stored entries (b = 0: the solution decays
    # to 0) ends its sweeps at the rounding of that Gram -- on empty_lines the GPU counts (294, 224), the C oracle (292, 219) and the
    # Python oracle on the same scaled problem (293, 222); the three differ in rows / columns 59, 10 and 44 only, the empty ones.
    if pname == "f64" and absent == "missing":
        assert (s1, s2) == (it1, it2), key


# ---- 1. single half-steps against the helper ------------------------------------------------------------------------------------------------
SHAPES = [(n, m, k, d) for (n, m, k) in [(200, 100, 5), (257, 129, 17), (515, 131, 50), (64, 700, 64), (33, 1, 1)] for d in (0.02, 0.3)]
SHAPES.append((150, 90, 16, 1.0))


@pytest.mark.parametrize("pname,prec,tol", PRECS)
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("absent", ABSENT)
@pytest.mark.parametrize("shape", SHAPES)
def test_half_steps_match_helper(pname, prec, tol, method, absent, shape):
    n, m, k, density = shape
    seed = n + 7 * m + 13 * k + method + int(1000 * density)
    rng = np.random.default_rng(seed)
    S = rand_csc(n, m, density, rng)
    w = make_weights(absent, S[2].size, rng)
    check_half_steps(("half", shape, absent, method), pname, prec, tol, S, w, absent, k, method, REG, seed + 1)


@pytest.mark.parametrize("pname,prec,tol", PRECS)
@pytest.mark.parametrize("method", [1, 2])
def test_half_steps_weights_below_the_absent_weight(pname, prec, tol, method):
    """absent = zero with every stored weight in (0, 1): c - c0 < 0, the per-column Gram is the shared one MINUS a weighted sum."""
    n, m, k = 257, 129, 17
    rng = np.random.default_rng(40 + method)
    S = rand_csc(n, m, 0.3, rng)
    w = make_weights("zero", S[2].size, rng, "below_one")
    assert np.all(w > 0) and np.all(w < 1)
    check_half_steps(("below_one", method), pname, prec, tol, S, w, "zero", k, method, REG, 50 + method)


# ---- 2. structure edges: empty lines, one line of more than 2048 stored entries ---------------------------------------------------------------
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


_EDGE = {}


def edge_case(case):
    if case not in _EDGE:
        rng = np.random.default_rng({"empty_lines": 21, "heavy_column": 22, "heavy_row": 23}[case])
        if case == "empty_lines":
            S, k = empty_lines_csc(rng), 4
        else:
            S, k = heavy_column_csc(rng), 16
            if case == "heavy_row":  # the transpose: the W half-step's CSR has the long line
                S = wc.transpose(*S)
        _EDGE[case] = (S, k, {a: make_weights(a, S[2].size, rng) for a in ABSENT})
    return _EDGE[case]


@pytest.mark.parametrize("pname,prec,tol", PRECS)
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("absent", ABSENT)
@pytest.mark.parametrize("case", ["empty_lines", "heavy_column", "heavy_row"])
def test_edge_structure_half_steps(pname, prec, tol, method, absent, case):
    """Segment slots, the fix-up and, for absent = zero, the shared Gram added once to long and to empty columns.

    heavy_column / heavy_row under the zero semantics are also why that path solves SCD in fp64 in both modes: every column but one has
    ONE stored entry among 4000 zeros, so from the random start the scaled gradient is ~6.7 where the solution is ~0.02 (77 % of it exact
    zeros); with the fp32 state of colsolve_row_kernel these two cases measured W 1.339e-04, H 1.305e-04 and W 1.302e-04, H 1.225e-04
    against the mode's 1e-4 (the same solve in fp64 from operands rounded to fp32 is 1.3e-07 from the reference)."""
    S, k, ws = edge_case(case)
    assert case == "empty_lines" or max(int(np.diff(S[0]).max()), int(np.bincount(S[1]).max())) > 2048
    check_half_steps(("edge", case, absent, method), pname, prec, tol, S, ws[absent], absent, k, method, [0.01, 0.0, 0.0], 60 + method,
                     masks=False)


@pytest.mark.parametrize("pname,prec,tol", PRECS)
def test_empty_column_under_zero_semantics_is_an_all_zero_column(pname, prec, tol):
    """absent = zero: an empty column has G = G_full and b = 0 -- the solve of an all-zero column of weight 1, which the plain zero door
    gives too (its Gram is the shared one)."""
    rng = np.random.default_rng(70)
    S = empty_lines_csc(rng)
    n, m = S[3]
    k = 4
    w = make_weights("zero", S[2].size, rng)
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    res = []
    for weighted in (True, False):
        with nnlm_amd.Handle(0, prec) as h:
            set_weighted(h, S, w, "zero") if weighted else h.set_matrix_csc(*S)
            h.set_factors(k, W0, H0)
            h.half_step(1, [0.01, 0, 0], 20, 1e-9, 1)
            res.append(h.get_factors()[1])
    empty = [0, 10, 44]
    e = err(res[0][:, empty], res[1][:, empty])
    assert e <= tol, e
    assert err(res[0], res[1]) > 1e-3  # (the other columns carry weights)


# ---- 3. chunked Grams, determinism ------------------------------------------------------------------------------------------------------------
def chunk_case(rng):
    """3000 x 2000 at 1.5 %, plus a fully observed column and row (segments across chunks and workers)."""
    n, m = 3000, 2000
    obs = rng.random((n, m)) < 0.015
    obs[:, 17] = True
    obs[1234, :] = True
    flat = np.flatnonzero(obs.T.ravel())
    return csc_from_flat(flat, rng.random(flat.size), n, m)


def chunk_run(prec, S, w, absent, k, W0, H0, limit):
    _lib.debug_alloc_limit(limit)
    try:
        with nnlm_amd.Handle(0, prec) as h:
            set_weighted(h, S, w, absent)
            h.set_factors(k, W0, H0)
            r = h.run([0.01, 0, 0], [0, 0, 0.01], 4, 1e-300, 0, False, 20, 1e-9, 1, 1)
            chunks = h.get_info("sp_gram_chunks")  # (of the last half-step: H)
            gbytes = h.get_info("sp_gram_bytes")
            W, H = h.get_factors()
    finally:
        _lib.debug_alloc_limit(0)
    return W, H, r, chunks, gbytes


@pytest.mark.parametrize("pname,prec,tol", PRECS)
@pytest.mark.parametrize("absent", ABSENT)
def test_chunked_grams_and_repeated_runs_are_bit_identical(pname, prec, tol, absent):
    rng = np.random.default_rng(26)
    S = chunk_case(rng)
    n, m = S[3]
    k = 16
    w = make_weights(absent, S[2].size, rng)
    W0, H0 = rng.random((n, k)) * 0.1, rng.random((k, m)) * 0.1
    limit = 600 * 16 * 16 * 8  # 600 Gram slots: >= 3 chunks of the 2000 H columns
    runs = [chunk_run(prec, S, w, absent, k, W0, H0, lim) for lim in (0, 0, limit)]
    (W1, H1, r1, c1, _), (W2, H2, r2, c2, _), (W3, H3, r3, c3, b3) = runs
    assert c1 == 1 and c2 == 1 and c3 >= 3 and b3 <= limit, (c1, c2, c3, b3)
    keys = ("mse_error", "mkl_error", "target_error", "average_epoch")
    assert np.array_equal(W1, W2) and np.array_equal(H1, H2) and all(np.array_equal(r1[x], r2[x]) for x in keys), "two runs differ"
    dw, dh = relF(W3, W1), relF(H3, H1)
    print(f"{pname} {absent}: chunked vs unchunked W {dw:.3e}, H {dh:.3e}")
    assert np.array_equal(W1, W3) and np.array_equal(H1, H3), f"{pname} {absent}: chunked run differs: W {dw:.3e}, H {dh:.3e}"
    assert all(np.array_equal(r1[x], r3[x]) for x in keys)


# ---- 4. / 5. every weight 1: the unweighted doors --------------------------------------------------------------------------------------------
def unit_case():
    rng = np.random.default_rng(80)
    n, m, k = 257, 129, 17
    S = rand_csc(n, m, 0.1, rng)
    return S, k, rng.random((n, k)), rng.random((k, m)), rng.random((n, k)) < 0.1, rng.random((k, m)) < 0.1


def unit_run(prec, S, k, W0, H0, Wm, Hm, door, method):
    with nnlm_amd.Handle(0, prec) as h:
        door(h)
        info = h.matrix_info()
        h.set_factors(k, W0, H0, Wm, Hm)
        r = h.run([0.01, 0.0, 0.001], [0.0, 0.002, 0.01], 3, 1e-300, 0, False, 10, 1e-9, method, 1)
        W, H = h.get_factors()
    return W, H, r, info


@pytest.mark.parametrize("pname,prec,tol", PRECS)
@pytest.mark.parametrize("method", [1, 2])
def test_unit_weights_absent_missing_equal_the_missing_door_bit_for_bit(pname, prec, tol, method):
    S, k, W0, H0, Wm, Hm = unit_case()
    ones = np.ones(S[2].size)
    Ww, Hw, rw, iw = unit_run(prec, S, k, W0, H0, Wm, Hm, lambda h: set_weighted(h, S, ones, "missing"), method)
    Wu, Hu, ru, iu = unit_run(prec, S, k, W0, H0, Wm, Hm, lambda h: h.set_matrix_csc_missing(*S), method)
    assert iw == iu
    assert np.array_equal(Ww, Wu) and np.array_equal(Hw, Hu), (relF(Ww, Wu), relF(Hw, Hu))
    assert len(rw["mse_error"]) == 3
    for key in ("mse_error", "mkl_error", "target_error", "average_epoch"):
        assert np.array_equal(rw[key], ru[key]), (key, rw[key], ru[key])


@pytest.mark.parametrize("pname,prec,tol", PRECS)
@pytest.mark.parametrize("method", [1, 2])
def test_unit_weights_absent_zero_match_the_zero_door(pname, prec, tol, method):
    S, k, W0, H0, Wm, Hm = unit_case()
    ones = np.ones(S[2].size)
    Ww, Hw, rw, iw = unit_run(prec, S, k, W0, H0, Wm, Hm, lambda h: set_weighted(h, S, ones, "zero"), method)
    Wu, Hu, ru, iu = unit_run(prec, S, k, W0, H0, Wm, Hm, lambda h: h.set_matrix_csc(*S), method)
    assert iw["n_non_missing"] == iu["n_non_missing"] and iw["any_missing"] == iu["any_missing"]
    assert abs(iw["kl_const"] - iu["kl_const"]) <= 1e-14 * abs(iu["kl_const"])
    ew, eh = relF(Ww, Wu), relF(Hw, Hu)
    assert ew <= tol and eh <= tol, f"{pname}: W {ew:.3e}, H {eh:.3e}"
    for key in ("mse_error", "mkl_error", "target_error"):
        d = float(np.max(np.abs(rw[key] - ru[key]) / np.abs(ru[key])))
        assert len(rw[key]) == len(ru[key]) == 3 and d <= tol, f"{pname} {key}: {d:.3e}"


# ---- 6. full runs and the fold-in against the helper ----------------------------------------------------------------------------------------
_FULL = {}


@pytest.mark.parametrize("pname,tol", [("f64", 1e-10), ("f32", 1e-4)])
@pytest.mark.parametrize("absent", ABSENT)
def test_api_nnmf_matches_helper(monkeypatch, pname, tol, absent):
    if pname == "f32":
        monkeypatch.setenv("NNLM_PRECISION", "f32")
    n, m, k = 200, 100, 5
    rng = np.random.default_rng(90)
    S = rand_csc(n, m, 0.2, rng)
    w = make_weights(absent, S[2].size, rng)
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    alpha, beta = [0.0, 0.0, 0.01], [0.01, 0.0, 0.0]
    # (the stopping tolerance: from the helper's own trace, whose relative decrease of the target passes it inside the run with a margin
    #  of 15 % or more on both sides -- zero: 1.16e-3 then 4.96e-4; missing: 9.7e-3 then 6.8e-3)
    rel_tol = {"zero": 1e-3, "missing": 8e-3}[absent]
    kw = dict(init={"W": W0, "H": H0}, max_iter=30, rel_tol=rel_tol, inner_max_iter=10, trace=2, alpha=alpha, beta=beta)
    if absent not in _FULL:
        _FULL[absent] = wc.c_nnmf(S, w, absent, k, W0, H0, None, None, alpha, beta, 30, rel_tol, 10, 1e-9, 1, 2)
    o = _FULL[absent]
    g = api.nnmf(Csc(S), k, absent=absent, weights=w, **kw)
    gs = api.nnmf(Csc(S), k, absent=absent, weights=Csc((S[0], S[1], w, S[3])), **kw)  # (the sparse form of the same weights)
    assert np.array_equal(g["W"], gs["W"]) and np.array_equal(g["H"], gs["H"])
    ew, eh = relF(g["W"], o["W"]), relF(g["H"], o["H"])
    print(f"{pname} {absent}: W {ew:.3e}, H {eh:.3e}, iterations {g['n_iteration']} ref {o['n_iteration']}")
    assert ew <= tol and eh <= tol, f"{pname} {absent}: W {ew:.3e}, H {eh:.3e}"
    assert g["n_iteration"] == o["n_iteration"], (g["n_iteration"], o["n_iteration"])
    assert 2 < o["n_iteration"] < 30  # (the stopping rule ended the run)
    for key, okey in (("mse", "mse_error"), ("mkl", "mkl_error"), ("target_loss", "target_error")):
        d = float(np.max(np.abs(g[key] - o[okey]) / np.abs(o[okey])))
        assert len(g[key]) == len(o[okey]) and d <= tol, f"{pname} {absent} {key}: {d:.3e}"
    if pname == "f64":
        assert np.array_equal(g["average_epochs"], o["average_epoch"])
    assert g["options"]["absent"] == absent


@pytest.mark.parametrize("pname,tol", [("f64", 1e-10), ("f32", 1e-4)])
@pytest.mark.parametrize("absent", ABSENT)
def test_fold_in_matches_helper(monkeypatch, pname, tol, absent):
    if pname == "f32":
        monkeypatch.setenv("NNLM_PRECISION", "f32")
    n, q, p = 400, 250, 6
    rng = np.random.default_rng(91)
    S = rand_csc(n, q, 0.06, rng)
    w = make_weights(absent, S[2].size, rng)
    x, Bh = rng.random((n, p)), rng.random((p, q))
    model = {"W": x, "H": Bh, "options": {"method": "scd", "loss": "mse", "absent": absent}}
    A, C, obs = wc.dense_parts(S, w, absent)
    for method, mname in ((1, "scd"), (2, "lee")):
        pr = api.predict_nnmf(model, Csc(S), which="H", method=mname, absent=absent, weights=w, init=Bh, max_iter=200, rel_tol=1e-12,
                              alpha=[0.01, 0, 0])
        B_ref, it = wc.half_step(Bh, x.T, A, C, obs, None, [0.01, 0, 0], 200, 1e-12, method, absent == "missing")
        e = relF(pr["coefficients"], B_ref)
        assert e <= tol, f"{pname} {absent} {mname}: {e:.3e}"
        assert pr["n_iteration"] == it or pname == "f32"
        N = float(S[2].size) if absent == "missing" else float(n * q)
        mse, _ = wc.errors(A, C, obs, x.T, pr["coefficients"], N)
        assert pr["error"]["MSE"] == pytest.approx(mse, rel=1e-10)


# ---- 7. refusals, get_info, matrix_info ----------------------------------------------------------------------------------------------------
def code_of(fn, *a, **kw):
    with pytest.raises(_lib.NnlmError) as ei:
        fn(*a, **kw)
    return ei.value.code, str(ei.value)


@pytest.mark.parametrize("pname,prec,tol", PRECS)
@pytest.mark.parametrize("absent", ABSENT)
def test_refusals_and_info(pname, prec, tol, absent):
    n, m, k = 150, 90, 4
    rng = np.random.default_rng(30)
    S = rand_csc(n, m, 0.1, rng)
    ptr, idx, val, shp = S
    w = make_weights("missing", val.size, rng)
    w[7] = 0.0
    miss = absent == "missing"
    with nnlm_amd.Handle(0, prec) as h:
        assert h.get_info("sparse_weighted") == 0.0
        for bad, word in ((-0.5, "-0.5"), (np.nan, "nan")):
            wb = w.copy()
            wb[11] = bad
            code, msg = code_of(h.set_matrix_csc_weighted, ptr, idx, val, wb, shp, miss)
            assert code == ERR_ARG and "nnlm_set_matrix_csc_weighted" in msg and "entry 11 " in msg and word in msg.lower(), msg
        code, msg = code_of(h.set_matrix_csc_weighted, ptr, idx, val, None, shp, miss)
        assert code == ERR_ARG and "weight is NULL" in msg
        set_weighted(h, S, w, absent)
        assert h.get_info("sparse_weighted") == 1.0 and h.get_info("matrix_absent_missing") == float(miss)
        info = h.matrix_info()
        assert info["n_non_missing"] == (val.size if miss else n * m)  # (a weight-0 entry is still counted)
        assert info["any_missing"] == miss
        klc = wc.kl_const(S, w, absent)
        assert abs(info["kl_const"] - klc) <= 1e-12 * abs(klc)
        code, msg = code_of(h.set_factors, 65)
        assert code == ERR_UNSUPPORTED and "rank" in msg and "weights" in msg
        h.set_factors(k, rng.random((n, k)), rng.random((k, m)))
        for method in (3, 4):
            code, msg = code_of(h.half_step, 1, [0, 0, 0], 5, 1e-9, method)
            assert code == ERR_UNSUPPORTED and "KL" in msg and "weights" in msg
            code, msg = code_of(h.run, [0, 0, 0], [0, 0, 0], 3, 1e-4, 0, False, 1, 1e-9, method, 1)
            assert code == ERR_UNSUPPORTED and "KL" in msg and "weights" in msg
        code, msg = code_of(h.debug_partial, 1)
        assert code == ERR_UNSUPPORTED and "weights" in msg
        code, msg = code_of(h.set_factors_batch, [2, 3])
        assert code == ERR_UNSUPPORTED and "batched" in msg and "weights" in msg
        code, msg = code_of(h.set_factors_nndsvd_batch, [2, 3])
        assert code == ERR_UNSUPPORTED and "weights" in msg
        code, msg = code_of(h.comm_init, None, 0, 2)
        assert code == ERR_UNSUPPORTED and "weights" in msg
        code, msg = code_of(h.svd, 6, 1, rng.random((6, m)))
        assert code == ERR_UNSUPPORTED and "SVD" in msg and "weights" in msg
        code, msg = code_of(h.set_factors_nndsvd, 4)
        assert code == ERR_UNSUPPORTED and "NNDSVD" in msg and "weights" in msg
        # another door on the same handle ends the weighted state
        h.set_matrix_csc(*S)
        assert h.get_info("sparse_weighted") == 0.0


def test_one_shot_entries_take_weights():
    n, m, k = 60, 40, 3
    rng = np.random.default_rng(31)
    S = rand_csc(n, m, 0.3, rng)
    w = make_weights("zero", S[2].size, rng)
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    g = _lib.c_nnmf_csc_weighted(S[0], S[1], S[2], w, False, S[3], k, W0, H0, None, None, [0, 0, 0], [0, 0, 0], 4, 1e-300, 1, 0, False, 5, 1e-9, 1, 1)
    o = wc.c_nnmf(S, w, "zero", k, W0, H0, None, None, [0, 0, 0], [0, 0, 0], 4, 1e-300, 5, 1e-9, 1, 1)
    assert relF(g["W"], o["W"]) <= 1e-10 and relF(g["H"], o["H"]) <= 1e-10 and g["n_iteration"] == 4
    wb = w.copy()
    wb[0] = -1.0
    code, msg = code_of(_lib.c_nnlm_csc_weighted, W0, S[0], S[1], S[2], wb, True, S[3], [0, 0, 0], None, H0, 5, 1e-9, 1, 1)
    assert code == ERR_ARG and "nnlm_set_matrix_csc_weighted" in msg and "entry 0 " in msg


# ---- 8. scores of a weighted fit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("absent", ABSENT)
def test_top_n_on_a_weighted_fit(absent):
    n, m, k = 120, 80, 4
    rng = np.random.default_rng(32)
    S = rand_csc(n, m, 0.1, rng)
    w = make_weights(absent, S[2].size, rng)
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    fit = api.nnmf(Csc(S), k, absent=absent, weights=w, init={"W": W0, "H": H0}, max_iter=5, rel_tol=1e-300, inner_max_iter=5,
                   check_k=False)  # (absent = missing: a column of this matrix stores fewer than k entries)
    by_hand = {"W": np.array(fit["W"]), "H": np.array(fit["H"])}
    for by in ("column", "row"):
        i1, s1 = api.top_n(fit, 5, by=by, seen=Csc(S))
        i2, s2 = api.top_n(by_hand, 5, by=by, seen=Csc(S))
        assert np.array_equal(i1, i2) and np.array_equal(s1, s2)
    # the weighted handle itself: its stored pattern is what exclude = 1 leaves out, as on any sparse handle
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
        set_weighted(h, S, w, absent)
        h.set_factors(k, by_hand["W"], by_hand["H"])
        ih, sh = h.top_n(5, by="column", exclude=True)
        pe = h.predict_entries(S[1][:50], np.repeat(np.arange(m), np.diff(S[0]))[:50])
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
        h.set_matrix_csc(*S)
        h.set_factors(k, by_hand["W"], by_hand["H"])
        iu, su = h.top_n(5, by="column", exclude=True)
        pu = h.predict_entries(S[1][:50], np.repeat(np.arange(m), np.diff(S[0]))[:50])
    assert np.array_equal(ih, iu) and np.array_equal(sh, su) and np.array_equal(pe, pu)
