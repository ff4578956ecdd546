"""KL loss on a sparse A (nnlm_set_matrix_csc_kl, k_sparse_kl.h) on the MI355X against the fp64 oracle on the DENSIFIED matrix, against
the dense GPU path, and through every door.  Cases: tests/sparse_kl_cases.py (tests/test_sparse_kl_host.py shows them well posed).

Bounds (the project's existing ones for this arithmetic): factors and traces 1e-10 in the strict mode, 1e-4 in the fp32-operand mode
(PRECS of test_gpu_sparse.py); mkl_error additionally gets the absolute 4e-15 of test_gpu_fuzz_sparse.py for the zeros that
sp_err_final_kernel leaves out; strict-mode sweep counts are equal.  Every test fails without the feature: the symbols do not exist."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_cases as sc  # noqa: E402
import sparse_kl_cases as kc  # noqa: E402
from helpers import relF  # noqa: E402
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402
from oracle import ref  # noqa: E402

pytestmark = pytest.mark.gpu

PRECS = [("f64", _lib.PREC_F64, 1e-10), ("f32", _lib.PREC_F32, 1e-4)]
ERR_ARG, ERR_UNSUPPORTED = 1, 5
CASES = kc.all_half_step_cases()
_REFS = {}


@pytest.fixture(autouse=True)
def _default_precision(monkeypatch):
    monkeypatch.delenv("NNLM_PRECISION", raising=False)


def refs(i, method):
    """The oracle's two half-steps of CASES[i], computed once per (case, method)."""
    if (i, method) not in _REFS:
        _REFS[(i, method)] = kc.half_step_refs(CASES[i], ref, method)
    return _REFS[(i, method)]


def code_of(fn, *a):
    with pytest.raises(_lib.NnlmError) as ei:
        fn(*a)
    return ei.value.code


def check_traces(r, o, A, pname, tol, what):
    for key in ("mse_error", "mkl_error", "target_error", "average_epoch"):
        assert r[key].shape == o[key].shape, (what, key)
    dm = np.abs(r["mse_error"] - o["mse_error"])
    bm = tol * o["mse_error"] + 1e-12 * np.mean(A * A)  # (the sum of squares over the zeros is a Gram cancellation, test_gpu_sparse.py)
    print(what, "mse", float(np.max(dm / bm)), "of bound")
    assert np.all(dm <= bm), (what, float(np.max(dm / bm)))
    for key in ("mkl_error", "target_error"):
        d = np.abs(r[key] - o[key])
        b = tol * np.abs(o[key]) + 4e-15
        print(what, key, float(np.max(d / b)), "of bound")
        assert np.all(d <= b), (what, key, float(np.max(d / b)))


# ---- 1. single half-steps: every case, both methods, both modes; the form each half-step took -------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", PRECS)
@pytest.mark.parametrize("method", [3, 4])
@pytest.mark.parametrize("i", range(len(CASES)), ids=[c["name"].replace(" ", "_") for c in CASES])
def test_half_steps_match_oracle(pname, prec, tol, method, i):
    c = CASES[i]
    W1_ref, it1, H1_ref, it2 = refs(i, method)
    fw, fh = kc.line_forms(c["S"])
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix_csc_kl(*c["S"])
        assert h.get_info("sparse_kl") == 1 and h.get_info("sparse_kl_short_max") == kc.SHORT_MAX
        assert h.get_info("sparse_kl_form_w") == -1 and h.get_info("sparse_kl_form_h") == -1
        h.set_factors(c["k"], c["W0"], c["H0"], c["Wm"], c["Hm"])
        h.half_step(0, c["alpha"], c["inner"], 1e-9, method)
        W1, _ = h.get_factors()
        s1 = h.take_sweeps()
        h.half_step(1, c["beta"], c["inner"], 1e-9, method)
        _, H1 = h.get_factors()
        s2 = h.take_sweeps()
        assert (h.get_info("sparse_kl_form_w"), h.get_info("sparse_kl_form_h")) == (fw, fh)
    if pname == "f32":  # (strict: the oracle's own W1, sweep counts stay exact; fp32: the W this half-step actually had fixed -- test_gpu_sparse.py)
        H1_ref, _ = ref.update(c["H0"].copy(), W1.T.copy(), kc.dense_of(c), c["Hm"], c["beta"], c["inner"], 1e-9, method, missing=False)
    ew, eh = sc.err(W1, W1_ref), sc.err(H1, H1_ref)
    print(c["name"], pname, method, "W %.3e H %.3e" % (ew, eh))
    assert np.all(np.isfinite(W1)) and np.all(np.isfinite(H1))
    assert ew <= tol and eh <= tol, f"{c['name']} {pname} method {method}: W {ew:.3e}, H {eh:.3e} (bound {tol:g})"
    assert np.all(W1 >= 0) and np.all(H1 >= 0)
    if c["Wm"] is not None:
        assert np.array_equal(W1[c["Wm"] != 0], c["W0"][c["Wm"] != 0])
    if c["Hm"] is not None:
        assert np.array_equal(H1[c["Hm"] != 0], c["H0"][c["Hm"] != 0])
    if pname == "f64":
        assert (s1, s2) == (it1, it2)


def test_designed_lines_sit_on_the_threshold():
    """The restated dispatch rule against the library's own threshold, and the designed lines on both sides of it in both orientations."""
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
        for tr in (False, True):
            c = kc.lines_case(kc.THRESHOLD_COUNTS, 5, tr)
            h.set_matrix_csc_kl(*c["S"])
            assert h.get_info("sparse_kl_short_max") == kc.SHORT_MAX
            h.set_factors(c["k"], c["W0"], c["H0"])
            h.half_step(0, [0, 0, 0], 1, 1e-9, 3)
            h.half_step(1, [0, 0, 0], 1, 1e-9, 3)
            got = (h.get_info("sparse_kl_form_w"), h.get_info("sparse_kl_form_h"))
            assert got == ((3, 1) if tr else (1, 3)), got  # (the designed lines take both forms; the other orientation's lines are short)


# ---- 2. whole runs: 150 x 90, k = 4, density 0.1, five iterations, trace 1 --------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", PRECS)
@pytest.mark.parametrize("method", [3, 4])
def test_run_with_traces_matches_oracle(pname, prec, tol, method):
    c = kc.count_case(150, 90, 4, 0.1, 1)
    A = kc.dense_of(c)
    reg_a, reg_b = [0.01, 0, 0.01], [0, 0.01, 0.02]
    # SCD-KL with more than one inner sweep is chaotic on this data: the ORACLE's own five-iteration run moves by 1e-5 ... 1e-1 under a 1e-13
    # perturbation of the start (tests/test_sparse_kl_host.py pins that, and that the configurations run here move by < 1e-11)
    for inner in ((1,) if method == 3 else (1, 2)):
        with nnlm_amd.Handle(0, prec) as h:
            h.set_matrix_csc_kl(*c["S"])
            h.set_factors(c["k"], c["W0"], c["H0"])
            r = h.run(reg_a, reg_b, 5, -1.0, 0, False, inner, 1e-9, method, 1)
            W, H = h.get_factors()
        o = ref.c_nnmf(A, c["k"], c["W0"], c["H0"], None, None, reg_a, reg_b, 5, -1.0, 1, 0, False, inner, 1e-9, method, 1)
        ew, eh = relF(W, o["W"]), relF(H, o["H"])
        print(pname, method, inner, "W %.3e H %.3e" % (ew, eh))
        assert ew <= tol and eh <= tol, f"{pname} method {method} inner {inner}: W {ew:.3e}, H {eh:.3e}"
        assert r["n_iteration"] == o["n_iteration"] == 5
        check_traces(r, o, A, pname, tol, f"{pname} method {method} inner {inner}")
        if pname == "f64":
            assert np.array_equal(r["average_epoch"], o["average_epoch"])
        else:
            # (fp32-operand mode: sweep counts are tolerance-only, DESIGN 2 -- the dense fuzz's (2 inner) / (n + m))
            assert np.allclose(r["average_epoch"], o["average_epoch"], rtol=0, atol=2.0 * inner / (150 + 90))


# ---- 3. the rank limit ---------------------------------------------------------------------------------------------------------------------
def test_rank_65_is_refused():
    c = kc.count_case(300, 200, 4, 0.1, 3)
    rng = np.random.default_rng(65)
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
        h.set_matrix_csc_kl(*c["S"])
        h.set_factors(65, rng.random((300, 65)), rng.random((65, 200)))
        for method in (3, 4):
            for which in (0, 1):
                assert code_of(h.half_step, which, [0, 0, 0], 1, 1e-9, method) == ERR_UNSUPPORTED
            with pytest.raises(_lib.NnlmError) as ei:
                h.run([0, 0, 0], [0, 0, 0], 2, -1.0, 0, False, 1, 1e-9, method, 1)
            assert ei.value.code == ERR_UNSUPPORTED and "64" in str(ei.value)
        h.half_step(1, [0, 0, 0], 2, 1e-9, 1)  # (square loss keeps its rank > 64 path)


# ---- 4. a state that returns to exactly 0 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", PRECS)
@pytest.mark.parametrize("method", [3, 4])
def test_exact_state_gives_no_nan_and_keeps_live_coordinates(pname, prec, tol, method):
    c = kc.exact_state_case()
    A = kc.dense_of(c)
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix_csc_kl(*c["S"])
        h.set_factors(c["k"], c["W0"], c["H0"])
        h.half_step(1, [0, 0, 0], 3, 1e-9, method)
        _, H1 = h.get_factors()
    H_ref, _ = ref.update(c["H0"].copy(), c["W0"].T.copy(), A, None, [0, 0, 0], 3, 1e-9, method, missing=False)
    assert np.all(np.isfinite(H1))
    eh = sc.err(H1, H_ref)
    assert eh <= tol, f"{pname} method {method}: H {eh:.3e}"
    assert np.array_equal(H1 > 0, H_ref > 0), int(np.sum((H1 > 0) != (H_ref > 0)))  # no live coordinate lost, none revived


# ---- 5. against the dense GPU path on the same matrix, the same mode, the same bounds ------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", PRECS)
@pytest.mark.parametrize("method", [3, 4])
def test_sparse_run_matches_dense_gpu_run(pname, prec, tol, method):
    c = kc.count_case(150, 90, 4, 0.1, 1)
    A = kc.dense_of(c)
    outs = []
    for sparse in (False, True):
        with nnlm_amd.Handle(0, prec) as h:
            h.set_matrix_csc_kl(*c["S"]) if sparse else h.set_matrix(A)
            h.set_factors(c["k"], c["W0"], c["H0"])
            r = h.run([0.01, 0, 0], [0, 0, 0.01], 4, -1.0, 0, False, 1, 1e-9, method, 1)
            r["W"], r["H"] = h.get_factors()
            outs.append(r)
    d, s = outs
    ew, eh = relF(s["W"], d["W"]), relF(s["H"], d["H"])
    print(pname, method, "sparse vs dense: W %.3e H %.3e" % (ew, eh))
    assert ew <= tol and eh <= tol, f"{pname} method {method}: W {ew:.3e}, H {eh:.3e}"
    check_traces(s, d, A, pname, tol, f"{pname} method {method} vs dense")
    if pname == "f64":
        assert np.array_equal(s["average_epoch"], d["average_epoch"])


# ---- 6. two runs are bit-identical (short and long lines, a line holding half of all entries) ---------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", PRECS)
def test_two_runs_are_bit_identical(pname, prec, tol):
    for c in (kc.half_case(700, 60, 6, False), kc.half_case(700, 60, 6, True), kc.lines_case(kc.THRESHOLD_COUNTS, 5, False)):
        res = []
        for _ in range(2):
            with nnlm_amd.Handle(0, prec) as h:
                h.set_matrix_csc_kl(*c["S"])
                h.set_factors(c["k"], c["W0"], c["H0"])
                h.iterate(2, [0.01, 0, 0], [0, 0, 0.01], 2, 1e-9, 3)
                h.iterate(2, [0.01, 0, 0], [0, 0, 0.01], 2, 1e-9, 4)
                res.append(h.get_factors() + (h.errors()[1], h.take_sweeps()))
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and res[0][2:] == res[1][2:], c["name"]


# ---- 7. the doors ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,tol", [("f64", 1e-10), ("f32", 1e-4)])
def test_one_shot_entries_and_api(monkeypatch, pname, tol):
    if pname == "f32":
        monkeypatch.setenv("NNLM_PRECISION", "f32")
    c = kc.count_case(150, 90, 4, 0.1, 1)
    S, A, k = c["S"], kc.dense_of(c), c["k"]
    z = [0, 0, 0]
    for method in (3, 4):
        args = (k, c["W0"], c["H0"], None, None, [0.01, 0, 0], z, 4, -1.0, 1, 0, False, 1, 1e-9, method, 2)
        g, o = _lib.c_nnmf_csc_kl(*S, *args), ref.c_nnmf(A, *args)
        assert relF(g["W"], o["W"]) <= tol and relF(g["H"], o["H"]) <= tol, (method, relF(g["W"], o["W"]), relF(g["H"], o["H"]))
        assert g["n_iteration"] == o["n_iteration"] == 4
        check_traces(g, o, A, pname, tol, f"one-shot {pname} method {method}")
        x, B0 = c["W0"], c["H0"]
        gl = _lib.c_nnlm_csc_kl(x, *S, z, None, B0, 6, 1e-9, 1, method)
        ol = ref.c_nnlm(x, A, z, None, B0, 6, 1e-9, 1, method)
        assert relF(gl["coefficient"], ol["coefficient"]) <= tol, (method, relF(gl["coefficient"], ol["coefficient"]))
        assert gl["n_iteration"] == ol["n_iteration"] or pname == "f32"
    Sx = sc.Csc(S)
    kw = dict(loss="mkl", max_iter=4, rel_tol=-1.0, init={"W": c["W0"], "H": c["H0"]})
    for method in ("scd", "lee"):
        r = api.nnmf(Sx, k, method=method, rng=np.random.default_rng(0), sparse_kl=True, **kw)
        rd = api.nnmf(A, k, method=method, rng=np.random.default_rng(0), **kw)
        ew, eh = relF(r["W"], rd["W"]), relF(r["H"], rd["H"])
        assert ew <= tol and eh <= tol, f"{pname} api.nnmf {method} sparse vs dense: W {ew:.3e}, H {eh:.3e}"
        assert r["n_iteration"] == rd["n_iteration"] == 4 and r["options"]["loss"] == "mkl"
    # the default init drawn from the same seeded rng: the sparse call and the dense call start alike
    r = api.nnmf(Sx, k, loss="mkl", max_iter=3, rel_tol=-1.0, rng=np.random.default_rng(5), sparse_kl=True)
    rd = api.nnmf(A, k, loss="mkl", max_iter=3, rel_tol=-1.0, rng=np.random.default_rng(5))
    assert relF(r["W"], rd["W"]) <= tol and relF(r["H"], rd["H"]) <= tol, (relF(r["W"], rd["W"]), relF(r["H"], rd["H"]))
    fit = api.nnlm(c["W0"], Sx, loss="mkl", init=c["H0"], max_iter=6, rel_tol=1e-9, sparse_kl=True)
    fd = api.nnlm(c["W0"], A, loss="mkl", init=c["H0"], max_iter=6, rel_tol=1e-9)
    assert relF(fit["coefficients"], fd["coefficients"]) <= tol
    assert fit["error"]["MKL"] == pytest.approx(fd["error"]["MKL"], rel=max(tol, 1e-9))
    model = {"W": c["W0"], "H": c["H0"], "options": {"method": "scd", "loss": "mkl"}}
    pr = api.predict_nnmf(model, Sx, which="H", init=c["H0"], max_iter=6, rel_tol=1e-9, sparse_kl=True)
    pref = ref.c_nnlm(c["W0"], A, z, None, c["H0"], 6, 1e-9, 1, 3)
    assert relF(pr["coefficients"], pref["coefficient"]) <= tol


# ---- 8. a handle loaded for KL is the sparse handle for everything else ------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", PRECS)
def test_square_loss_is_bit_for_bit_the_csc_handle(pname, prec, tol):
    c = kc.family_case("heavy")
    res = []
    for loader in ("set_matrix_csc", "set_matrix_csc_kl"):
        with nnlm_amd.Handle(0, prec) as h:
            getattr(h, loader)(*c["S"])
            h.set_factors(c["k"], c["W0"], c["H0"])
            out = []
            for method in (1, 2):
                r = h.run([0.01, 0, 0], [0, 0, 0.01], 3, -1.0, 0, False, 5, 1e-9, method, 1)
                out += [r[key] for key in ("mse_error", "mkl_error", "target_error", "average_epoch")] + list(h.get_factors())
            idx, score = h.top_n(3, by="column", exclude=True)
            res.append(out + [idx, score, np.array([h.get_info("matrix_nnz")])])
            assert h.get_info("sparse_kl") == (1 if loader.endswith("_kl") else 0)
    assert len(res[0]) == len(res[1]) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(*res))


# ---- 9. refusals and switching loaders ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", PRECS)
def test_refusals_and_switching(pname, prec, tol):
    c = kc.count_case(150, 90, 4, 0.1, 1)
    S, A, k = c["S"], kc.dense_of(c), c["k"]
    ptr, idx, val, shp = S
    z = [0, 0, 0]
    with nnlm_amd.Handle(0, prec) as h:
        for bad in (-1.0, np.nan, np.inf):
            v = val.copy()
            v[3] = bad
            with pytest.raises(_lib.NnlmError) as ei:
                h.set_matrix_csc_kl(ptr, idx, v, shp)
            assert ei.value.code == ERR_ARG and "entry 3" in str(ei.value)
        swapped = idx.copy()
        j = int(np.argmax(np.diff(ptr)))
        swapped[ptr[j]], swapped[ptr[j] + 1] = idx[ptr[j] + 1], idx[ptr[j]]
        assert code_of(h.set_matrix_csc_kl, ptr, swapped, val, shp) == ERR_ARG  # (the canonical-CSC checks of nnlm_set_matrix_csc)
        h.set_matrix_csc_kl(*S)
        assert code_of(h.comm_init, None, 0, 2) == ERR_UNSUPPORTED
        assert code_of(h.set_factors_batch, [2, 2]) == ERR_UNSUPPORTED
        # (nnlm_set_factors_batch is the gate of the batch entries on a resident handle: nnlm_run_batch needs the batch it refuses, and
        #  nnlm_c_nnmf_batch takes a dense matrix)
        with pytest.raises(_lib.NnlmError) as ei:
            h.set_factors_batch([1, 3])
        assert ei.value.code == ERR_UNSUPPORTED and "nnlm_set_matrix_csc_kl" in str(ei.value)

        def fit(hh, method):
            hh.set_factors(k, c["W0"], c["H0"])
            hh.iterate(2, z, z, 1, 1e-9, method)
            return hh.get_factors() + (hh.get_info("matrix_nnz"), hh.get_info("sparse_kl"), hh.take_sweeps())

        seq = []
        for loader, method in (("set_matrix_csc", 1), ("set_matrix_csc_kl", 3), ("set_matrix", 3), ("set_matrix_csc_kl", 4), ("set_matrix_csc", 2)):
            getattr(h, loader)(A) if loader == "set_matrix" else getattr(h, loader)(*S)
            seq.append((loader, method, fit(h, method)))
            if loader == "set_matrix_csc":  # the old refusal is back after a KL handle was replaced
                assert code_of(h.half_step, 1, z, 1, 1e-9, 3) == ERR_UNSUPPORTED and h.get_info("sparse_kl") == 0
    for loader, method, got in seq:
        with nnlm_amd.Handle(0, prec) as f:
            getattr(f, loader)(A) if loader == "set_matrix" else getattr(f, loader)(*S)
            fresh = fit(f, method)
        assert np.array_equal(got[0], fresh[0]) and np.array_equal(got[1], fresh[1]) and got[2:] == fresh[2:], (loader, method)
