"""KL loss on a sparse A, host side (no GPU): the routing of the `sparse_kl` keyword, the refusals of the wrapper (new and old), the ABI
exports, the restated dispatch rule -- and the conditions on the cases of tests/sparse_kl_cases.py that tests/test_gpu_sparse_kl.py runs:
each is shown well posed from the oracle alone (finite factors, nothing that dies, no line whose sweep count or whose clamp sits at a
tie that the comparison's tolerance could hide: the counts do not move with the inner tolerance nor with the order of the sums).  No skip rule."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_cases as sc  # noqa: E402
import sparse_kl_cases as kc  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402
from oracle import ref  # noqa: E402


def small():
    c = kc.count_case(40, 30, 3, 0.3, 5)
    return c, sc.Csc(c["S"])


# ---- the wrapper ---------------------------------------------------------------------------------------------------------------------------
def test_sparse_kl_routes_through_the_new_entries(monkeypatch):
    c, S = small()
    args, ctx = api.prepare_nnmf(S, 3, loss="mkl", sparse_kl=True, rng=np.random.default_rng(0))
    assert isinstance(args[0], api.CSC) and ctx["sparse_kl"] is True and args[15] == 3 and args[13] == 1  # (scd + mkl; R's inner.max.iter for KL)
    assert api.prepare_nnmf(S, 3, loss="mkl", method="lee", sparse_kl=True)[0][15] == 4
    assert api.prepare_nnmf(S, 3, loss="mse", sparse_kl=True)[1]["sparse_kl"] is False  # (square loss: the entries it always took)
    assert api.prepare_nnmf(kc.dense_of(c), 3, loss="mkl", sparse_kl=True)[1]["sparse_kl"] is False  # (a dense A: nothing to route)
    called = []

    def fake(name, out):
        def f(*a, **kw):
            called.append(name)
            return out
        return f

    n, m = S.shape
    nn = dict(W=np.ones((n, 3)), H=np.ones((3, m)), mse_error=[0.0], mkl_error=[0.0], target_error=[0.0], average_epoch=[1.0], n_iteration=1)
    for name in ("c_nnmf_csc", "c_nnmf_csc_kl", "c_nnmf_csc_missing", "c_nnmf"):
        monkeypatch.setattr(_lib, name, fake(name, nn))
    for name in ("c_nnlm_csc", "c_nnlm_csc_kl", "c_nnlm_csc_missing", "c_nnlm"):
        monkeypatch.setattr(_lib, name, fake(name, dict(coefficient=np.ones((3, m)), n_iteration=1)))
    api.nnmf(S, 3, loss="mkl", sparse_kl=True)
    api.nnmf(S, 3, loss="mse", sparse_kl=True)
    api.nnmf(S, 3, loss="mse")
    x = np.random.default_rng(1).random((n, 3))
    api.nnlm(x, S, loss="mkl", sparse_kl=True)
    api.nnlm(x, S, loss="mse", sparse_kl=True)
    model = {"W": x, "H": np.ones((3, m)), "options": {"method": "scd", "loss": "mkl"}}
    api.predict_nnmf(model, S, which="H", sparse_kl=True)
    assert called == ["c_nnmf_csc_kl", "c_nnmf_csc", "c_nnmf_csc", "c_nnlm_csc_kl", "c_nnlm_csc", "c_nnlm_csc_kl"]


def test_the_two_new_refusals():
    c, S = small()
    x = np.ones((40, 3))
    for call in (lambda: api.prepare_nnmf(S, 3, loss="mkl", sparse_kl=True, absent="missing"),
                 lambda: api.prepare_nnmf(S, 3, loss="mse", sparse_kl=True, absent="missing"),
                 lambda: api.prepare_nnlm(x, S, loss="mkl", sparse_kl=True, absent="missing")):
        with pytest.raises(api.NnlmStop) as ei:
            call()
        assert "sparse_kl" in str(ei.value) and "absent" in str(ei.value)
    ptr, idx, val, shp = c["S"]
    v = val.copy()
    v[2] = -1.0
    neg = sc.Csc((ptr, idx, v, shp))
    with pytest.raises(api.NnlmStop, match="negative"):
        api.prepare_nnmf(neg, 3, loss="mkl", sparse_kl=True)
    with pytest.raises(api.NnlmStop, match="negative"):
        api.prepare_nnlm(x, neg, loss="mkl", sparse_kl=True)
    api.prepare_nnmf(neg, 3, loss="mse", sparse_kl=True)  # (square loss takes negative data, as before)


def test_the_default_still_raises_the_old_text():
    c, S = small()
    old_A = "Sparse A is supported for loss = 'mse' only; use a dense matrix for loss = 'mkl'."
    old_y = "Sparse y is supported for loss = 'mse' only; use a dense matrix for loss = 'mkl'."
    for kw in ({}, {"sparse_kl": False}):
        with pytest.raises(api.NnlmStop) as ei:
            api.prepare_nnmf(S, 3, loss="mkl", **kw)
        assert str(ei.value) == old_A
        with pytest.raises(api.NnlmStop) as ei:
            api.nnmf(S, 3, loss="mkl", **kw)
        assert str(ei.value) == old_A
        with pytest.raises(api.NnlmStop) as ei:
            api.prepare_nnlm(np.ones((40, 3)), S, loss="mkl", **kw)
        assert str(ei.value) == old_y


def test_abi_exports():
    hdr = open(os.path.join(ROOT, "include", "nnlm_mi355x.h")).read()
    lib = _lib.load()
    for name in ("nnlm_set_matrix_csc_kl", "nnlm_c_nnmf_csc_kl", "nnlm_c_nnlm_csc_kl"):
        assert name in _lib.EXPORTS and ("int " + name + "(") in hdr and hasattr(lib, name)
        assert getattr(lib, name).argtypes == getattr(lib, name[:-3]).argtypes  # the signatures of the square-loss entries
    for key in ("sparse_kl", "sparse_kl_form_h", "sparse_kl_form_w"):
        assert '"' + key + '"' in hdr
    assert callable(_lib.c_nnmf_csc_kl) and callable(_lib.c_nnlm_csc_kl) and callable(_lib.Handle.set_matrix_csc_kl)


# ---- the dispatch rule ---------------------------------------------------------------------------------------------------------------------
def test_dispatch_rule_covers_both_forms():
    src = open(os.path.join(ROOT, "nnlm_amd", "csrc", "k_sparse_kl.h")).read()
    assert "#define SPKL_EPL 4 " in src and "#define SPKL_SHORT_MAX (64 * SPKL_EPL)" in src and kc.SHORT_MAX == 64 * 4
    assert [kc.form_of(v) for v in (0, 1, kc.SHORT_MAX - 1, kc.SHORT_MAX)] == [kc.FORM_SHORT] * 4
    assert [kc.form_of(v) for v in (kc.SHORT_MAX + 1, 4097, 10 ** 6)] == [kc.FORM_LONG] * 3
    for tr in (False, True):
        c = kc.lines_case(kc.THRESHOLD_COUNTS, 5, tr)
        rows, cols = sc.line_counts(c["S"])
        assert sorted(rows if tr else cols) == sorted(kc.THRESHOLD_COUNTS)  # exactly the designed counts, on the designed side
        assert kc.line_forms(c["S"]) == ((3, 1) if tr else (1, 3))
    # every family reaches the long form in at least one orientation somewhere, and the short one everywhere
    seen = 0
    for c in kc.all_half_step_cases():
        fw, fh = kc.line_forms(c["S"])
        assert fw & kc.FORM_SHORT and fh & kc.FORM_SHORT, c["name"]
        seen |= (fw | fh)
    assert seen == 3
    for tr in (False, True):  # one line holding half of all stored entries
        c = kc.half_case(700, 60, 6, tr)
        rows, cols = sc.line_counts(c["S"])
        big = (rows if tr else cols).max()
        assert big == 700 and 2 * big >= c["S"][1].size and kc.form_of(int(big)) == kc.FORM_LONG
    assert {c["name"] for c in kc.boundary_family()} == {"boundary " + n + t for n in kc.BOUNDARY_NAMES for t in ("", "^T")}


# ---- the cases are well posed (the oracle alone) -------------------------------------------------------------------------------------------
CASES = kc.all_half_step_cases() + [kc.exact_state_case()]


@pytest.mark.parametrize("method", [3, 4])
@pytest.mark.parametrize("i", range(len(CASES)), ids=[c["name"].replace(" ", "_") for c in CASES])
def test_cases_are_well_posed(i, method):
    c = CASES[i]
    _, _, val, _ = c["S"]
    assert np.all(val > 0) and np.all(val == np.rint(val))  # counts, zeros dropped from the structure
    W1, it1, H1, it2 = kc.half_step_refs(c, ref, method)
    assert np.all(np.isfinite(W1)) and np.all(np.isfinite(H1)) and np.all(W1 >= 0) and np.all(H1 >= 0)
    # no factor dies (a column of W / a row of H at 1e-8 of the median norm: degenerate() of sparse_cases.py)
    dw, dh = (W1 * W1).sum(axis=0), (H1 * H1).sum(axis=1)
    assert dw.min() > 1e-8 * np.median(dw) and dh.min() > 1e-8 * np.median(dh)
    # no line at a tie of the stopping rule: the sweep counts do not move when the inner tolerance does, by far more than the 1e-10 the
    # strict comparison allows the factors (a line whose relative change sat within 1e-3 of the tolerance would change its count)
    for tol in (1e-9 * (1 - 1e-3), 1e-9 * (1 + 1e-3)):
        _, a1, _, a2 = kc.half_step_refs(c, ref, method, rel_tol=tol)
        assert (a1, a2) == (it1, it2)
    # well conditioned: a 1e-13 perturbation of the start moves the oracle's result by less than 1e-11 and no sweep count (SCD-KL on
    # zero-heavy counts can amplify by 1e5 and more: such cases are not generated, see option_cases)
    rng = np.random.default_rng(1)
    for _ in range(2):
        Wp, p1, Hp, p2 = kc.half_step_refs(kc.perturbed(c, rng), ref, method)
        assert (p1, p2) == (it1, it2)
        assert sc.err(Wp, W1) <= 1e-11 and sc.err(Hp, H1) <= 1e-11, (sc.err(Wp, W1), sc.err(Hp, H1))
    # SCD: no rounding dust in the W1 that the H half-step has fixed.  Several SCD sweeps can leave a coordinate at 1e-16 of the others where
    # its minimiser is 0; the KL quotient w / (wh + 1e-16) sees that size, so whether a summation order lands on 5e-16 or on an exact 0
    # moves the next half-step by 1e-9 ... 1e-5 (the dense strict path deviates from the oracle by the same amounts on such cases:
    # seeds 10 of the penalty cases and 13-16 of the mask case, which are therefore not generated)
    if method == 3 and c["name"] != "exact_state":  # (exact_state runs one H half-step only)
        live = W1[W1 > 0]
        assert live.min() > 1e-7 * W1.max(), float(live.min())
    # no coordinate at a tie that the tolerance could hide (a clamp decided by rounding, a sweep that counts rounding dust as a change):
    # the oracle on the row- and column-reversed problem -- the same sums in another order, which is all the sparse path changes -- gives
    # the same factors to 1e-11 and the same sweep counts (the check of tests/test_data_cases_host.py)
    A = kc.dense_of(c)
    rev = dict(c, S=sc.csc_from_pattern(A[::-1, ::-1] != 0, A[::-1, ::-1]), W0=c["W0"][::-1].copy(), H0=c["H0"][:, ::-1].copy(),
               Wm=None if c["Wm"] is None else np.asarray(c["Wm"])[::-1].copy(), Hm=None if c["Hm"] is None else np.asarray(c["Hm"])[:, ::-1].copy())
    W1r, r1, H1r, r2 = kc.half_step_refs(rev, ref, method)
    assert (r1, r2) == (it1, it2)
    assert sc.err(W1r[::-1], W1) <= 1e-11 and sc.err(H1r[:, ::-1], H1) <= 1e-11, (sc.err(W1r[::-1], W1), sc.err(H1r[:, ::-1], H1))


def test_run_case_is_well_posed():
    """The 150 x 90 whole-run case: the oracle's run is finite, nothing dies and the target error decreases."""
    c = kc.count_case(150, 90, 4, 0.1, 1)
    A = kc.dense_of(c)
    assert abs(c["S"][1].size / (150 * 90) - 0.1) < 0.03  # (density 0.1 of the pattern; the Poisson zeros left the structure)
    for method in (3, 4):
        o = ref.c_nnmf(A, 4, c["W0"], c["H0"], None, None, [0.01, 0, 0.01], [0, 0.01, 0.02], 5, -1.0, 1, 0, False, 1, 1e-9, method, 1)
        assert np.all(np.isfinite(o["W"])) and np.all(np.isfinite(o["H"])) and np.all(np.isfinite(o["mkl_error"]))
        assert np.all(np.diff(o["target_error"]) < 0)
    # the run configurations of the GPU file are well conditioned; SCD-KL with two inner sweeps is NOT (which is why it is not run there)
    def moved(method, inner, iters, ra, rb):
        rng, outs = np.random.default_rng(0), []
        for size in (0.0, 1e-13, 1e-13):
            d = kc.perturbed(c, rng, size)
            outs.append(ref.c_nnmf(A, 4, d["W0"], d["H0"], None, None, ra, rb, iters, -1.0, 1, 0, False, inner, 1e-9, method, 1))
        return max(sc.err(o["W"], outs[0]["W"]) + sc.err(o["H"], outs[0]["H"]) for o in outs[1:])

    ra, rb, z = [0.01, 0, 0.01], [0, 0.01, 0.02], [0, 0, 0]
    for method, inner, iters, a, b in ((3, 1, 5, ra, rb), (4, 1, 5, ra, rb), (4, 2, 5, ra, rb), (3, 1, 4, z, z), (4, 1, 4, z, z),
                                       (3, 1, 4, [0.01, 0, 0], [0, 0, 0.01]), (4, 1, 4, [0.01, 0, 0], [0, 0, 0.01]), (3, 1, 4, [0.01, 0, 0], z)):
        assert moved(method, inner, iters, a, b) <= 1e-11, (method, inner, iters)
    assert moved(3, 2, 5, ra, rb) > 1e-8
