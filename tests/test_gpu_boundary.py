"""GPU tests of the boundary's loose ends: host callbacks (interrupt, progress bar, verbose = 2 table), the stacked
known-profile / mask inputs of R/misc.R:48-129, W.norm (R/nnmf.R:197-205) and the vignette's rank selection by
imputation (vignettes/Fast-And-Versatile-NMF.Rmd:613-694) -- all through the C ABI, checked against the oracle."""
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


def _problem(seed=5, n=80, m=60, k=4):
    rng = np.random.default_rng(seed)
    A = rng.random((n, k)) @ rng.random((k, m)) + 0.01 * rng.random((n, m))
    return A, 0.01 * rng.random((n, k)), 0.01 * rng.random((k, m))


# ---- callbacks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [_lib.PREC_F64, _lib.PREC_F32])
@pytest.mark.parametrize("stop_at", [0, 1, 4, 5])  # 4: a trace iteration has just queued a speculative W half-step
def test_check_interrupt_aborts_at_the_iteration_and_leaves_the_handle_consistent(prec, stop_at):
    """Rcpp::checkUserInterrupt() is polled once per outer iteration before any work of that iteration
    (src/nnmf.cpp:111).  A non-zero answer at the top of iteration i must return NNLM_ERR_INTERRUPT with exactly i
    iterations applied -- in particular the speculative W half-step queued behind a trace iteration must be dropped --
    and the resident handle must remain usable: continuing from there reproduces an uninterrupted run."""
    A, W0, H0 = _problem()
    z = [0.0, 0.0, 0.0]
    calls = []

    def intr():
        calls.append(len(calls))
        return len(calls) - 1 == stop_at

    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix(A)
        h.set_factors(4, W0, H0)
        cb = _lib.make_callbacks(check_interrupt=intr)
        with pytest.raises(_lib.NnlmError) as ei:
            h.run(z, z, 10, -1.0, 0, False, 5, 1e-9, 1, 1, callbacks=cb)
        assert ei.value.code == 3 and len(calls) == stop_at + 1
        assert _lib.load().nnlm_last_error(h._h) == b"interrupted"
        Wi, Hi = h.get_factors()
        sweeps_i = h.take_sweeps(reset=False)
        # continue for the remaining iterations on the same handle
        h.run(z, z, 10 - stop_at, -1.0, 0, False, 5, 1e-9, 1, 1)
        Wc, Hc = h.get_factors()
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix(A)
        h.set_factors(4, W0, H0)
        if stop_at:
            h.iterate(stop_at, z, z, 5, 1e-9, 1)
        Wr, Hr = h.get_factors()
        h.iterate(10 - stop_at, z, z, 5, 1e-9, 1)
        Wf, Hf = h.get_factors()
    tol = 1e-12 if prec == _lib.PREC_F64 else 1e-6
    assert relF(Wi, Wr) < tol and relF(Hi, Hr) < tol          # exactly stop_at iterations were applied
    assert relF(Wc, Wf) < 10 * tol and relF(Hc, Hf) < 10 * tol  # and the handle carried on correctly
    assert sweeps_i <= (80 + 60) * 5  # at most the open trace window's sweeps; never the dropped half-step's


@pytest.mark.parametrize("loop", ["solo", "batch"])
def test_progress_callback_counts_every_iteration(monkeypatch, loop):
    """verbose == 1: RcppProgress is incremented once per outer iteration (src/nnmf.cpp:60,112) -- once per iteration of the
    batch, not per member."""
    monkeypatch.setenv("NNLM_PRECISION", "f64")
    A, W0, H0 = _problem()
    seen = []
    cb = _lib.make_callbacks(progress=lambda d, t: seen.append((d, t)))

    def run(verbose):
        z = [0, 0, 0]
        if loop == "solo":
            return [nnlm_amd.c_nnmf(A, 4, W0, H0, None, None, z, z, 7, -1.0, 1, verbose, False, 5, 1e-9, 1, 2, callbacks=cb)]
        return nnlm_amd.c_nnmf_batch(A, [2, 4], None, None, z, z, 7, -1.0, 1, verbose, False, 5, 1e-9, 1, 2, callbacks=cb)

    assert [r["n_iteration"] for r in run(1)] == ([7] if loop == "solo" else [7, 7]) and seen == [(i + 1, 7) for i in range(7)]
    seen.clear()
    run(0)
    run(2)
    assert seen == []  # verbose 0 and 2 do not drive the bar


@pytest.mark.parametrize("method,trace", [(1, 2), (4, 3)])
def test_verbose2_table_text(monkeypatch, method, trace):
    """verbose == 2: the Rprintf table of src/nnmf.cpp:100-104,155-156,188-189,194-198 -- header, one row per trace entry
    (iteration number, MSE, MKL, target, relative error in the reference's formats), footer."""
    monkeypatch.setenv("NNLM_PRECISION", "f64")
    A, W0, H0 = _problem()
    out = []
    cb = _lib.make_callbacks(print_fn=out.append)
    args = (A, 4, W0, H0, None, None, [0.01, 0, 0], [0, 0, 0.01], 6, -1.0, 1, 2, False, 5, 1e-9, method, trace)
    r = nnlm_amd.c_nnmf(*args, callbacks=cb)
    o = ref.c_nnmf(*args)
    text = "".join(out)
    head = "\n%10s | %10s | %10s | %10s | %10s\n" % ("Iteration", "MSE", "MKL", "Target", "Rel. Err.")
    rule = "--------------------------------------------------------------\n"
    foot = "%10s | %10s | %10s | %10s | %10s\n\n" % ("Iteration", "MSE", "MKL", "Target", "Rel. Err.")
    assert text.startswith(head + rule) and text.endswith(rule + foot)
    rows = text[len(head + rule):-len(rule + foot)].splitlines()
    assert len(rows) == len(o["mse_error"]) == len(r["mse_error"])
    its = [i + 1 for i in range(6) if i % trace == 0]
    if (6 - 1) % trace != 0:
        its.append(6 + 1)  # the closing block prints i+1 with i == max_iter (src/nnmf.cpp:188-189)
    last = 1e99
    for row, it, mse, mkl, terr in zip(rows, its, o["mse_error"], o["mkl_error"], o["target_error"]):
        rel = 2 * (last - terr) / (last + terr + 1e-16)
        last = terr
        cells = [c.strip() for c in row.split("|")]
        assert int(cells[0]) == it
        assert cells[1] == ("%10.4f" % mse).strip() and cells[2] == ("%10.4f" % mkl).strip() and cells[3] == ("%10.4f" % terr).strip()
        assert abs(float(cells[4]) - rel) <= 0.35 * abs(rel)  # "%10.g": one significant digit
        assert len(row) == 5 * 10 + 4 * 3


@pytest.mark.parametrize("prec", [_lib.PREC_F64, _lib.PREC_F32])
@pytest.mark.parametrize("stop_at", [0, 1, 3])
def test_check_interrupt_of_the_batch_loop(prec, stop_at):
    """The batched loop polls like the solo one: an interrupt at the top of iteration i returns NNLM_ERR_INTERRUPT with exactly i
    iterations applied to every member, and the handle's last error names it."""
    A, W0, H0 = _problem()
    z, ks = [0.0, 0.0, 0.0], [2, 4]
    Ws, Hs = [W0[:, :k] for k in ks], [H0[:k] for k in ks]
    calls = []

    def intr():
        calls.append(len(calls))
        return len(calls) - 1 == stop_at

    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix(A)
        h.set_factors_batch(ks, Ws, Hs)
        with pytest.raises(_lib.NnlmError) as ei:
            h.run_batch(z, z, 10, -1.0, 0, False, 5, 1e-9, 1, 2, callbacks=_lib.make_callbacks(check_interrupt=intr))
        assert ei.value.code == 3 and len(calls) == stop_at + 1
        assert _lib.load().nnlm_last_error(h._h) == b"interrupted"
        got = h.get_factors_batch()
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix(A)
        h.set_factors_batch(ks, Ws, Hs)
        if stop_at:
            h.run_batch(z, z, stop_at, -1.0, 0, False, 5, 1e-9, 1, 2)
        want = h.get_factors_batch()
    tol = 1e-12 if prec == _lib.PREC_F64 else 1e-6
    for (Wg, Hg), (Ww, Hw) in zip(got, want):
        assert relF(Wg, Ww) < tol and relF(Hg, Hw) < tol


@pytest.mark.parametrize("max_iter,rel_tol,trace", [(6, -1.0, 2), (40, 1e-3, 1)])
def test_verbose2_table_text_of_the_batch(monkeypatch, max_iter, rel_tol, trace):
    """verbose == 2 of the batched loop: the member column in front of the solo table's header and rule, then one row per booked
    trace entry -- the solo row behind its member's number, in the order the entries are booked (by iteration, then member) and
    holding exactly that member's trace -- and no footer."""
    monkeypatch.setenv("NNLM_PRECISION", "f64")
    A, W0, H0 = _problem()
    ks = [1, 4]
    out = []
    res = nnlm_amd.c_nnmf_batch(A, ks, [W0[:, :k] for k in ks], [H0[:k] for k in ks], [0.01, 0, 0], [0, 0, 0.01], max_iter, rel_tol, 1,
                                2, False, 5, 1e-9, 1, trace, callbacks=_lib.make_callbacks(print_fn=out.append))
    head = "\n%6s %10s | %10s | %10s | %10s | %10s\n" % ("Member", "Iteration", "MSE", "MKL", "Target", "Rel. Err.")
    rule = "---------------------------------------------------------------------\n"
    rows = []
    for b, r in enumerate(res):
        nit = r["n_iteration"]
        its = [i + 1 for i in range(nit) if i % trace == 0]
        if nit == max_iter and (max_iter - 1) % trace != 0:
            its.append(max_iter + 1)  # the closing entry prints i+1 with i == max_iter (src/nnmf.cpp:188-189)
        assert len(its) == len(r["mse_error"])
        last = 1e99
        for it, mse, mkl, terr in zip(its, r["mse_error"], r["mkl_error"], r["target_error"]):
            rel = 2 * (last - terr) / (last + terr + 1e-16)
            last = terr
            rows.append((it, b, "%6d %10d | %10.4f | %10.4f | %10.4f | %10.g\n" % (b, it, mse, mkl, terr, rel)))
    assert "".join(out) == head + rule + "".join(row for _, _, row in sorted(rows))


def test_warning_callback_and_flag(monkeypatch):
    monkeypatch.setenv("NNLM_PRECISION", "f64")
    A, W0, H0 = _problem()
    msgs = []
    cb = _lib.make_callbacks(warning=msgs.append)
    r = nnlm_amd.c_nnmf(A, 4, W0, H0, None, None, [0, 0, 0], [0, 0, 0], 3, 1e-12, 1, 0, True, 5, 1e-9, 1, 1, callbacks=cb)
    assert r["warning"] and msgs == ["Target tolerance not reached. Try a larger max.iter."]
    msgs.clear()
    r = nnlm_amd.c_nnmf(A, 4, W0, H0, None, None, [0, 0, 0], [0, 0, 0], 3, 1e-12, 1, 0, False, 5, 1e-9, 1, 1, callbacks=cb)
    assert not r["warning"] and msgs == []


def test_default_precision_of_the_one_shot_entries_is_fp64(monkeypatch):
    """The .Call boundary defaults to the strict mode (the reference is fp64 and its testthat vectors are held at 1.5e-8);
    NNLM_PRECISION=f32 opts into the fp32-operand mode."""
    monkeypatch.delenv("NNLM_PRECISION", raising=False)
    rng = np.random.default_rng(3)
    x = rng.random((30, 5))
    b = np.array([1.0, 2.0, 0.0, 0.5, 3.0])
    r = nnlm_amd.c_nnlm(x, x @ b, [0, 0, 0], None, np.ones((5, 1)), 10000, 1e-12, 1, 1)
    assert np.max(np.abs(r["coefficient"].ravel() - b)) < 1e-9
    monkeypatch.setenv("NNLM_PRECISION", "f32")
    r32 = nnlm_amd.c_nnlm(x, x @ b, [0, 0, 0], None, np.ones((5, 1)), 10000, 1e-12, 1, 1)
    assert 1e-12 < np.max(np.abs(r32["coefficient"].ravel() - b)) < 1e-4


def test_release_caches_between_one_shot_calls_changes_nothing(monkeypatch):
    """nnlm_release_caches (the R package's unload hook): the streams / events / bounce buffers a destroyed handle left behind go, the
    next one-shot call creates fresh ones and returns the same factors; calling it twice, or with nothing cached, is fine."""
    monkeypatch.delenv("NNLM_PRECISION", raising=False)
    A, W0, H0 = _problem(seed=11)
    args = (A, 4, W0, H0, None, None, [0, 0, 0], [0, 0, 0], 30, -1.0, 1, 0, False, 10, 1e-6, 1, 1)
    r1 = nnlm_amd.c_nnmf(*args)
    _lib.release_caches()
    _lib.release_caches()
    r2 = nnlm_amd.c_nnmf(*args)
    assert np.array_equal(r1["W"], r2["W"]) and np.array_equal(r1["H"], r2["H"])
    r3 = nnlm_amd.c_nnmf(*args)  # (on the cached resources of r2's handle)
    assert np.array_equal(r1["W"], r3["W"])


# ---- stacked known profiles, masks, W.norm through the R-interface mirror ------------------------------------------
@pytest.mark.parametrize("pname,tol", [("f64", 1e-8), ("f32", 1e-4)])
def test_known_profiles_and_masks_stacked_like_reformat_input(monkeypatch, pname, tol):
    """tests/testthat/test-nnmf.R:41-47: nnmf(A2, k, init = list(W0 = W1, H0 = H2)) -- K = k + k1 + k2 columns, W0 and
    H0 blocks fully masked (R/misc.R:60-82,119-128) so they come back bit-identical, partially masked W/H blocks next to
    them.  The same 17 arguments go to the GPU and to the oracle."""
    monkeypatch.setenv("NNLM_PRECISION", pname)
    rng = np.random.default_rng(21)
    n, m, k, k1, k2 = 120, 70, 3, 2, 1
    W, H = rng.random((n, k)), rng.random((k, m))
    W1, H1 = rng.random((n, k1)), rng.random((k1, m))
    W2, H2 = rng.random((n, k2)), np.ones((k2, m))
    A2 = W @ H + W1 @ H1 + W2 @ H2
    mask = {"W": rng.random((n, k)) < 0.1, "H": rng.random((k, m)) < 0.1}
    kw = dict(init={"W0": W1, "H0": H2}, mask=mask, max_iter=40, rel_tol=-1, inner_max_iter=20, show_warning=False)
    args, ctx = api.prepare_nnmf(A2, k, rng=np.random.default_rng(1), **kw)
    assert args[1] == k + k1 + k2
    o = api.finish_nnmf(ref.c_nnmf(*args), ctx)
    r = api.finish_nnmf(nnlm_amd.c_nnmf(*args), ctx)
    assert r.W.shape == (n, k + k1 + k2) and r.H.shape == (k + k1 + k2, m)
    assert np.array_equal(r.W[:, k:k + k1], W1) and np.array_equal(r.H[k + k1:], H2)  # fixed profiles untouched
    # masked entries of the free blocks keep their (random) initial values bit for bit: the reference leaves the
    # `init[[mat]][mask[[mat]]] <- 0` of R/misc.R:113 commented out
    Wi, Hi = args[2], args[3]
    assert np.array_equal(r.W[:, :k][mask["W"]], Wi[:, :k][mask["W"]]) and np.array_equal(r.H[:k][mask["H"]], Hi[:k][mask["H"]])
    assert np.array_equal(o.W[:, :k][mask["W"]], Wi[:, :k][mask["W"]])
    assert relF(r.W @ r.H, o.W @ o.H) < tol and relF(r.W, o.W) < 50 * tol and relF(r.H, o.H) < 50 * tol
    assert np.allclose(r.mse, o.mse, rtol=100 * tol, atol=1e-14)
    if pname == "f64":
        assert np.array_equal(r.average_epochs, o.average_epochs)


@pytest.mark.parametrize("W_norm", [1, 2, np.inf])
def test_w_norm_rescaling(monkeypatch, W_norm):
    """R/nnmf.R:197-205: columns of W rescaled to unit W.norm, rows of H scaled back; W H unchanged."""
    monkeypatch.setenv("NNLM_PRECISION", "f64")
    A, W0, H0 = _problem()
    r0 = api.nnmf(A, 4, init={"W": W0, "H": H0}, max_iter=20, rel_tol=-1, show_warning=False)
    r = api.nnmf(A, 4, init={"W": W0, "H": H0}, max_iter=20, rel_tol=-1, show_warning=False, W_norm=W_norm)
    norms = r.W.max(axis=0) if np.isinf(W_norm) else np.sum(r.W ** W_norm, axis=0) ** (1.0 / W_norm)
    assert np.allclose(norms, 1.0, rtol=1e-12)
    assert relF(r.W @ r.H, r0.W @ r0.H) < 1e-12


def test_rank_selection_by_imputation_matches_oracle(monkeypatch):
    """vignettes/Fast-And-Versatile-NMF.Rmd:640-665 at the vignette's size (400 x 50, true rank 3, 30 % of the entries held
    out): for k = 1..6 the held-out MSE of the GPU factorisation equals the oracle's, and is minimised at the true rank."""
    monkeypatch.setenv("NNLM_PRECISION", "f64")
    rng = np.random.default_rng(678)
    n, m, k0 = 400, 50, 3
    A = rng.random((n, k0)) @ (10 * rng.random((k0, m))) + rng.standard_normal((n, m))
    A[A < 0] = 0
    ind = rng.choice(A.size, int(0.3 * A.size), replace=False)
    A2 = A.copy()
    A2.ravel()[ind] = np.nan
    held, held_o = [], []
    for k in range(1, 7):
        g = np.random.default_rng(100 + k)
        init = {"W": 0.01 * g.random((n, k)), "H": 0.01 * g.random((k, m))}
        kw = dict(init=init, max_iter=60, rel_tol=1e-4, show_warning=False)
        r = api.nnmf(A2, k, **kw)
        args, ctx = api.prepare_nnmf(A2, k, **kw)
        o = api.finish_nnmf(ref.c_nnmf(*args), ctx)
        assert r.n_iteration == o.n_iteration
        held.append(float(np.mean(((r.W @ r.H).ravel()[ind] - A.ravel()[ind]) ** 2)))
        held_o.append(float(np.mean(((o.W @ o.H).ravel()[ind] - A.ravel()[ind]) ** 2)))
        assert abs(r.mse[-1] - o.mse[-1]) < 1e-8 * o.mse[-1]
    assert np.allclose(held, held_o, rtol=1e-6)
    assert int(np.argmin(held)) + 1 == k0


# ---- the R glue end to end, on a mock of the R API ------------------------------------------------------------------------
def _mock_r(tmp_path):
    """Build pkg/src/r_glue.c + tests/r_stub/mock_r.c against the in-tree libnnlm_mi355x.so and load it."""
    import ctypes as C
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = str(tmp_path / "libmockr.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-std=gnu99", "-O1", "-Wno-cast-function-type", "-I" + os.path.join(root, "tests", "r_stub"),
                           "-I" + os.path.join(root, "include"), os.path.join(root, "pkg", "src", "r_glue.c"),
                           os.path.join(root, "tests", "r_stub", "mock_r.c"), "-L" + os.path.join(root, "nnlm_amd"), "-lnnlm_mi355x",
                           "-Wl,-rpath," + os.path.join(root, "nnlm_amd"), "-o", so])
    lib = C.CDLL(so)
    vp = C.c_void_p
    for name, res, args in (("mock_real", vp, [C.POINTER(C.c_double), C.c_int, C.c_int]), ("mock_lgl", vp, [C.POINTER(C.c_int), C.c_int, C.c_int]),
                            ("mock_int", vp, [C.c_int]), ("mock_dbl", vp, [C.c_double]), ("mock_elt", vp, [vp, C.c_int]),
                            ("mock_name", C.c_char_p, [vp, C.c_int]), ("mock_real_ptr", C.POINTER(C.c_double), [vp]),
                            ("mock_int_value", C.c_int, [vp]), ("mock_length", C.c_long, [vp]), ("mock_nrow", C.c_int, [vp]),
                            ("mock_ncol", C.c_int, [vp]), ("mock_last_error", C.c_char_p, []), ("mock_last_warning", C.c_char_p, []),
                            ("mock_printed", C.c_char_p, []), ("mock_dotcall", vp, [C.c_char_p, C.c_int, C.POINTER(vp)]),
                            ("mock_registered_name", C.c_char_p, [C.c_int]), ("mock_reset", None, [C.c_int])):
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
    lib.mock_load_package()
    return lib


def _sexp_real(lib, a):
    import ctypes as C
    a = np.asfortranarray(np.asarray(a, dtype=np.float64))
    if a.ndim == 1:
        a = a.reshape(-1, 1, order="F")
    return lib.mock_real(a.ctypes.data_as(C.POINTER(C.c_double)), a.shape[0], a.shape[1])


def _sexp_lgl(lib, a, shape):
    import ctypes as C
    if a is None:
        return lib.mock_lgl(None, shape[0], 0) if shape[1] == 0 else lib.mock_lgl(None, 0, shape[1])
    a = np.asfortranarray(np.asarray(a, dtype=np.int32))
    return lib.mock_lgl(a.ctypes.data_as(C.POINTER(C.c_int)), a.shape[0], a.shape[1])


def _dotcall(lib, name, sexps):
    import ctypes as C
    arr = (C.c_void_p * len(sexps))(*sexps)
    return lib.mock_dotcall(name.encode(), len(sexps), arr)


def _mat(lib, s):
    n, m = lib.mock_nrow(s), lib.mock_ncol(s)
    return np.ctypeslib.as_array(lib.mock_real_ptr(s), shape=(n * m,)).reshape((n, m), order="F").copy()


def test_r_glue_end_to_end_with_a_mock_r_runtime(monkeypatch, tmp_path):
    """The .Call boundary itself (reference src/RcppExports.cpp:10-65): registration table, arities, argument order, result
    list names and order (R/nnmf.R:184 and R/nnlm.R:122 rename BY POSITION), trace truncation, empty matrices = "not given",
    RNG scope, warning raised after the library returned, R error on a library error, user interrupt -- with the R API
    mocked (tests/r_stub/mock_r.c) and the MI355X doing the work."""
    monkeypatch.delenv("NNLM_PRECISION", raising=False)
    lib = _mock_r(tmp_path)
    assert lib.mock_registered_count() == 2
    assert {(lib.mock_registered_name(i), lib.mock_registered_arity(i)) for i in range(2)} == {(b"_NNLM_c_nnlm", 9), (b"_NNLM_c_nnmf", 17)}
    A, W0, H0 = _problem()
    n, m, k = 80, 60, 4
    alpha, beta = [0.01, 0.0, 0.0], [0.0, 0.0, 0.02]

    def nnmf_args(W, H, max_iter=7, rel_tol=-1.0, verbose=0, show_warning=1, trace=2, kk=k):
        return [_sexp_real(lib, A), lib.mock_int(kk), _sexp_real(lib, W) if W is not None else lib.mock_real(None, n, 0),
                _sexp_real(lib, H) if H is not None else lib.mock_real(None, 0, m), _sexp_lgl(lib, None, (n, 0)), _sexp_lgl(lib, None, (0, m)),
                _sexp_real(lib, alpha), _sexp_real(lib, beta), lib.mock_int(max_iter), lib.mock_dbl(rel_tol), lib.mock_int(1),
                lib.mock_int(verbose), lib.mock_int(show_warning), lib.mock_int(5), lib.mock_dbl(1e-9), lib.mock_int(1), lib.mock_int(trace)]

    # 1. explicit init: same result as the oracle called with the same 17 arguments
    lib.mock_reset(-1)
    out = _dotcall(lib, "_NNLM_c_nnmf", nnmf_args(W0, H0))
    assert out, lib.mock_last_error()
    o = ref.c_nnmf(A, k, W0, H0, None, None, alpha, beta, 7, -1.0, 1, 0, True, 5, 1e-9, 1, 2)
    assert [lib.mock_name(out, i) for i in range(7)] == [b"W", b"H", b"mse_error", b"mkl_error", b"target_error", b"average_epoch", b"n_iteration"]
    assert relF(_mat(lib, lib.mock_elt(out, 0)), o["W"]) < 1e-9 and relF(_mat(lib, lib.mock_elt(out, 1)), o["H"]) < 1e-9
    ntr = len(o["mse_error"])
    for i, key in ((2, "mse_error"), (3, "mkl_error"), (4, "target_error"), (5, "average_epoch")):
        v = lib.mock_elt(out, i)
        assert lib.mock_length(v) == ntr  # truncated to the used length (src/nnmf.cpp:200-206)
        assert np.allclose(_mat(lib, v).ravel(), o[key], rtol=1e-9)
    assert lib.mock_int_value(lib.mock_elt(out, 6)) == 7
    assert lib.mock_warning_count() == 1 and lib.mock_last_warning() == b"Target tolerance not reached. Try a larger max.iter."
    assert lib.mock_protect_balance() == 0 and lib.mock_rng_balance() == 0 and lib.mock_rng_draws() == 0

    # 2. empty W / H = default init through R's RNG: W first (n*k draws), then H (k*m) (src/nnmf.cpp:82-98); verbose = 2 prints
    lib.mock_reset(-1)
    out = _dotcall(lib, "_NNLM_c_nnmf", nnmf_args(None, None, max_iter=3, show_warning=0, verbose=2))
    assert out, lib.mock_last_error()
    assert lib.mock_rng_draws() == n * k + k * m and lib.mock_warning_count() == 0
    assert b"Iteration" in lib.mock_printed() and b"Rel. Err." in lib.mock_printed()
    W = _mat(lib, lib.mock_elt(out, 0))
    assert W.shape == (n, k) and np.all(W >= 0)

    # 3. a library error becomes an R error (BEGIN_RCPP / END_RCPP): method 9 does not exist
    lib.mock_reset(-1)
    bad = nnmf_args(W0, H0)
    bad[15] = lib.mock_int(9)
    assert not _dotcall(lib, "_NNLM_c_nnmf", bad) and b"method" in lib.mock_last_error()
    # wrong arity is refused by the registration table, as R does
    assert not _dotcall(lib, "_NNLM_c_nnmf", bad[:16]) and b"Incorrect number of arguments" in lib.mock_last_error()

    # 4. user interrupt at the third poll (Rcpp::checkUserInterrupt, src/nnmf.cpp:111)
    lib.mock_reset(2)
    assert not _dotcall(lib, "_NNLM_c_nnmf", nnmf_args(W0, H0, max_iter=50)) and lib.mock_onintr_count() == 1

    # 5. c_nnlm: 9 arguments, list (coefficient, n_iteration) (src/nnlm.cpp:49-52); the reference's known-answer vector
    from helpers import kat_case3
    A2, b3, expected, _ = kat_case3()
    lib.mock_reset(-1)
    y = A2 @ b3
    p = A2.shape[1]
    out = _dotcall(lib, "_NNLM_c_nnlm", [_sexp_real(lib, A2), _sexp_real(lib, y), _sexp_real(lib, [0.0, 0.0, 0.0]), _sexp_lgl(lib, None, (p, 0)),
                                         _sexp_real(lib, np.ones((p, 1))), lib.mock_int(10000), lib.mock_dbl(1e-12), lib.mock_int(1), lib.mock_int(1)])
    assert out, lib.mock_last_error()
    assert [lib.mock_name(out, i) for i in range(2)] == [b"coefficient", b"n_iteration"]
    coef = _mat(lib, lib.mock_elt(out, 0)).ravel()
    assert np.max(np.abs(coef - expected)) < 1.5e-8  # expect_equal's tolerance, tests/testthat/test-nnlm.R:40-43
    assert lib.mock_int_value(lib.mock_elt(out, 1)) > 0
    # dimension mismatch is the reference's message (tests/testthat/test-nnlm.R:54)
    assert not _dotcall(lib, "_NNLM_c_nnlm", [_sexp_real(lib, A2), _sexp_real(lib, y[:-1]), _sexp_real(lib, [0.0, 0.0, 0.0]), _sexp_lgl(lib, None, (p, 0)),
                                              _sexp_real(lib, np.ones((p, 1))), lib.mock_int(10), lib.mock_dbl(1e-12), lib.mock_int(1), lib.mock_int(1)])
    assert lib.mock_last_error() == b"Dimensions of x and y do not match."


# ---- bench.py's N > 1 plumbing on a one-GPU box ------------------------------------------------------------------------------
def test_bench_multi_gpu_branch_runs_with_a_forced_one_rank_communicator(tmp_path):
    """bench.py --gpus N takes a different path from N = 1: gloo process group, RCCL id broadcast, LOCAL_RANK -> device,
    nnlm_comm_init, barriers, max over ranks, the sharded half-steps.  No multi-GPU box is available to this suite, so the branch
    is forced with WORLD_SIZE = 1 (NNLM_BENCH_FORCE_COMM=1: a real RCCL communicator of size 1) on a reduced size and its line
    is compared with the plain single-GPU line of the same size: same final mse, same JSON contract."""
    import json
    import socket
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    base = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2", "--full", "--cpu-iters", "0", "--repeats", "1",
            "--size", "3000,2000,20"]
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), NNLM_BENCH_FORCE_COMM="1")
    def line_of(environment):
        out = subprocess.run(base, env=environment, capture_output=True, text=True, check=True).stdout.strip().splitlines()
        assert out and out[-1].startswith("{"), out[-3:]  # the JSON line is the LAST line of stdout (RCCL's banner is flushed before it)
        return json.loads(out[-1])

    sharded = line_of(env)
    env.pop("NNLM_BENCH_FORCE_COMM")
    plain = line_of(env)
    for line in (sharded, plain):
        for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
                    "config", "roofline", "cpu_baseline"):
            assert key in line, key
        assert line["n_gpus"] == 1 and line["steps"] == 6 and line["value"] > 0 and line["scaling"] == "strong"
    assert "all-gather" in sharded["config"]["parallelism"] and plain["config"]["parallelism"] == "1 GPU"
    assert abs(sharded["final_mse"] - plain["final_mse"]) < 1e-6 * plain["final_mse"]


def test_plain_bench_line_is_the_headline_and_its_dump_is_what_the_timed_steps_computed(tmp_path):
    """A plain bench.py run (no --full) times --steps steps once and prints the headline alone: what takes runs of its own (profiled
    replay, CPU baseline, other configurations, call-level metric, repeated regions) belongs to --full.  --dump-outputs DIR writes what
    its timed nnlm_run() returned after the last step -- W, H and the error traces -- and that must be what the same warm-up and steps
    compute on a handle of this process from bench.py's own seeded inputs."""
    import json
    import subprocess
    import bench  # (the repository root is on sys.path: tests/conftest.py)
    n, m, k, steps, warmup = 3000, 2000, 20, 6, 2
    cmd = [sys.executable, bench.__file__, "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--size", f"{n},{m},{k}",
           "--dump-outputs", str(tmp_path)]
    env = {v: x for v, x in os.environ.items() if v not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "NNLM_BENCH_FORCE_COMM")}
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, check=True, timeout=600).stdout.strip().splitlines()
    assert len(out) == 1, out[-3:]
    line = json.loads(out[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "final_mse"):
        assert key in line, key
    assert line["steps"] == steps and line["unit"] == "iterations/s" and line["higher_is_better"] is True
    assert abs(line["value"] * line["ms_per_step"] - 1e3) < 1e-9 * 1e3
    assert not {"repeats", "roofline", "kernels", "phases_ms", "cpu_baseline", "other_configs", "call", "forms"} & set(line)

    cfg = bench.CONFIGS[2]
    A, W0, H0 = bench.make_inputs(n, m, k, cfg["na"])
    cus = int(os.environ.get("NNLM_TEST_CUS", "0") or 0)
    _lib.debug_set_cus(0)  # (plan the launches as bench.py's process does, for the device's own CU count)
    try:
        with nnlm_amd.Handle(0, _lib.PREC_F32) as h:
            h.set_matrix(A)
            h.set_factors(k, W0, H0)
            bench.run_steps(h, cfg, warmup, cfg["trace"])
            r = bench.run_steps(h, cfg, steps, cfg["trace"])
            W, H = h.get_factors()
    finally:
        _lib.debug_set_cus(cus)
    want = dict(W=W, H=H, mse_error=r["mse_error"], mkl_error=r["mkl_error"], target_error=r["target_error"], average_epoch=r["average_epoch"])
    assert sorted(os.listdir(tmp_path)) == sorted(f"{nm}.npy" for nm in want)
    for nm, w in want.items():
        got = np.load(tmp_path / f"{nm}.npy")
        assert got.dtype == np.float64 and got.shape == w.shape, (nm, got.dtype, got.shape, w.shape)
        assert np.allclose(got, w, rtol=1e-12, atol=0.0), (nm, relF(got, w))
    assert abs(float(np.load(tmp_path / "mse_error.npy")[-1]) - line["final_mse"]) <= 1e-12 * line["final_mse"]


def test_profile_scopes_account_for_the_step_and_the_fused_error_reduction_is_not_a_pass_over_A():
    """VERDICT r5 item 4a.  On a trace iteration of the fused flow the error sums come out of the speculative W half-step's cross
    product (xprod16_err_kernel); what is left is a 5 us reduction.  Round 5 opened the "errors" scope BEFORE waiting for that cross
    product and bench.py priced the wait as 0.8 GB of HBM work.  Now: the reduction has its own scope ("err_reduce", opened behind the
    wait), "errors" only ever holds real passes over A, and the scopes of a profiled replay sum to its wall time up to the launch
    gaps (they can never exceed it: one stream, no scope inside another)."""
    import time
    rng = np.random.default_rng(4)
    n, m, k, steps = 6000, 4000, 50, 10
    A = rng.random((n, m))
    with nnlm_amd.Handle(0, _lib.PREC_F32) as h:
        h.set_matrix(A)
        h.set_factors(k, 0.01 * rng.random((n, k)), 0.01 * rng.random((k, m)))
        z = [0, 0, 0]
        h.run(z, z, 4, -1.0, 0, False, 50, 1e-9, 1, 2)  # warm-up (also the first, separate error pass of a run)
        h.sync()
        h.profile_reset()
        h.profile_enable(True)
        t0 = time.perf_counter()
        h.run(z, z, steps, -1.0, 0, False, 50, 1e-9, 1, 2)
        h.sync()
        wall_ms = 1e3 * (time.perf_counter() - t0)
        names = ("xprod_h", "xprod_w", "xprod_w_err", "gram", "sweep_h", "sweep_w", "errors", "err_reduce", "allgather", "allreduce", "unpack")
        sc = {nm: h.profile_get(nm) for nm in names}
        h.profile_enable(False)
    total = sum(ms for ms, _ in sc.values())
    # trace = 2: every second iteration is a trace iteration whose sums come fused (steps / 2 reductions); separate passes only at the
    # start and the end of the run (src/nnmf.cpp:121-126, 164-177)
    assert sc["err_reduce"][1] >= steps // 2 - 1 and sc["errors"][1] <= 3, sc
    assert sc["err_reduce"][0] / sc["err_reduce"][1] < 0.05, sc["err_reduce"]           # a reduction, not a wait for a cross product
    assert sc["xprod_w_err"][1] >= steps // 2 - 1
    assert 0.6 * wall_ms < total <= 1.02 * wall_ms, (total, wall_ms, sc)


# ---- N > 1 on real hardware: runs the moment the suite lands on a box with two or more GPUs ------------------------------------
def _gpu_count():
    try:
        import ctypes
        hip = ctypes.CDLL("libamdhip64.so")
        n = ctypes.c_int(0)
        return n.value if hip.hipGetDeviceCount(ctypes.byref(n)) == 0 else 0
    except OSError:
        return 0


@pytest.mark.skipif(_gpu_count() < 2, reason="needs >= 2 GPUs on the node (the gpurun lease has one); live on a multi-GPU box")
@pytest.mark.parametrize("form", ["cols", "reduce"])
def test_two_ranks_over_rccl_match_the_single_gpu_run(form):
    """BASELINE configs[3] at two ranks, for real: bench.py --gpus 2 under torch.distributed.run (one process per GPU, RCCL over
    xGMI) on a reduced size, both exchange forms, against the single-GPU line of the same size: same final mse (the sharded
    half-steps reproduce the unsharded factors up to summation order), strong scaling declared, n_gpus = 2."""
    import json
    import socket
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    tail = ["--steps", "6", "--warmup", "2", "--cpu-iters", "0", "--repeats", "1", "--size", "6000,4000,50", "--others", "0"]
    env = dict(os.environ, NNLM_SHARD_DENSE=form, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k_ in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k_, None)

    def last_json(cmd, environment):
        out = subprocess.run(cmd, env=environment, capture_output=True, text=True, check=True, timeout=600).stdout.strip().splitlines()
        assert out and out[-1].startswith("{"), out[-3:]
        return json.loads(out[-1])

    two = last_json([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                     "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2"] + tail, env)
    one = last_json([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1"] + tail, env)
    assert two["n_gpus"] == 2 and two["scaling"] == "strong" and two["value"] > 0
    assert ("all-reduce" in two["config"]["parallelism"]) == (form == "reduce")
    assert abs(two["final_mse"] - one["final_mse"]) < 1e-6 * one["final_mse"]
