"""Sparse input whose absent entries are missing, host side (no GPU): the `absent` argument of nnmf() / nnlm() / predict_nnmf(), its
refusals, the check_k rule of the reference for missing data, `options`, the error summary of nnlm() over the stored entries, and the
new C entries (declared, exported, failing loudly without a device)."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402

NEW = ("nnlm_set_matrix_csc_missing", "nnlm_c_nnmf_csc_missing", "nnlm_c_nnlm_csc_missing")


class Csc:
    """numpy-only duck-typed sparse matrix (canonical CSC given directly)."""

    def __init__(self, indptr, indices, data, shape):
        self.indptr, self.indices, self.data, self.shape = (np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int32),
                                                            np.asarray(data, dtype=float), shape)

    def tocsc(self):
        return self

    @property
    def T(self):
        n, m = self.shape
        cols = np.repeat(np.arange(m), np.diff(self.indptr))
        order = np.lexsort((cols, self.indices))
        rows_t = cols[order]
        indptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(self.indices, minlength=n), out=indptr[1:])
        return Csc(indptr, rows_t, self.data[order], (m, n))


def from_dense_pattern(A, observed):
    """CSC of the entries of A where `observed` is True (explicit zeros kept)."""
    n, m = A.shape
    flat = np.flatnonzero(observed.T.ravel())
    cols, rows = flat // n, flat % n
    indptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=m), out=indptr[1:])
    return Csc(indptr, rows, A[rows, cols], (n, m))


def test_absent_values():
    rng = np.random.default_rng(1)
    S = from_dense_pattern(rng.random((30, 20)), rng.random((30, 20)) < 0.5)
    for absent in ("zero", "missing", "miss", "z"):  # (match.arg: unique prefixes)
        _, ctx = api.prepare_nnmf(S, 2, rng=np.random.default_rng(0), absent=absent)
        assert ctx["absent"] in ("zero", "missing") and ctx["absent"].startswith(absent)
    with pytest.raises(api.NnlmStop, match="'absent' should be one of"):
        api.prepare_nnmf(S, 2, absent="na")
    _, ctx = api.prepare_nnmf(S, 2, rng=np.random.default_rng(0))
    assert ctx["absent"] == "zero"


def test_dense_with_absent_missing_is_refused():
    A = np.random.default_rng(2).random((20, 10))
    with pytest.raises(api.NnlmStop, match="needs a sparse A"):
        api.prepare_nnmf(A, 2, absent="missing")
    with pytest.raises(api.NnlmStop, match="needs a sparse y"):
        api.prepare_nnlm(np.ones((20, 3)), A, absent="missing", check_x=False)
    obj = {"W": np.ones((20, 2)), "H": np.ones((2, 10)), "options": {"method": "scd", "loss": "mse"}}
    with pytest.raises(api.NnlmStop, match="needs a sparse newdata"):
        api.predict_nnmf(obj, A, which="H", absent="missing", _nnlm=lambda *a, **k: None)
    api.prepare_nnmf(A, 2, absent="zero")  # (the default is today's behaviour)


def test_mkl_is_refused():
    rng = np.random.default_rng(3)
    S = from_dense_pattern(rng.random((30, 20)), rng.random((30, 20)) < 0.5)
    with pytest.raises(api.NnlmStop, match="loss = 'mse' only"):
        api.prepare_nnmf(S, 2, loss="mkl", absent="missing")
    with pytest.raises(api.NnlmStop, match="loss = 'mse' only"):
        api.prepare_nnlm(np.ones((30, 2)), S, loss="mkl", absent="missing", check_x=False)


def test_stored_non_finite_values_are_refused():
    S = Csc([0, 1, 2], [0, 1], [1.0, np.nan], (3, 2))
    with pytest.raises(api.NnlmStop, match="left out of the structure"):
        api.prepare_nnmf(S, 1, absent="missing")


def test_check_k_uses_the_fewest_observed_entries_of_a_row_or_column():
    rng = np.random.default_rng(4)
    n, m = 12, 9
    obs = np.ones((n, m), dtype=bool)
    obs[3, :6] = False  # row 3: 3 stored entries
    obs[5:10, 7] = False  # column 7: 7 stored entries
    S = from_dense_pattern(rng.random((n, m)), obs)
    with pytest.raises(api.NnlmStop, match="k larger than 3"):
        api.prepare_nnmf(S, 4, absent="missing")
    api.prepare_nnmf(S, 3, absent="missing")
    api.prepare_nnmf(S, 4, absent="missing", check_k=False)  # (check.k = FALSE skips it, as in R)
    api.prepare_nnmf(S, 4, absent="missing", alpha=[0.1, 0, 0])  # (regularised: the rule does not apply, R/nnmf.R:164)
    api.prepare_nnmf(S, 9, absent="zero")  # (zeros: min(n, m))
    obs[:, 2] = False  # an empty column: nothing observed, k > 0 is "not recommended"
    S0 = from_dense_pattern(rng.random((n, m)), obs)
    with pytest.raises(api.NnlmStop, match="k larger than 0"):
        api.prepare_nnmf(S0, 1, absent="missing")
    full = from_dense_pattern(rng.random((n, m)), np.ones((n, m), dtype=bool))
    api.prepare_nnmf(full, 9, absent="missing")


def test_options_carry_absent():
    rng = np.random.default_rng(5)
    S = from_dense_pattern(rng.random((30, 20)), rng.random((30, 20)) < 0.5)
    out = dict(W=np.ones((30, 2)), H=np.ones((2, 20)), mse_error=[1.0], mkl_error=[1.0], target_error=[0.5], average_epoch=[1.0],
               n_iteration=1, warning=False)
    for absent in ("zero", "missing"):
        _, ctx = api.prepare_nnmf(S, 2, rng=np.random.default_rng(0), absent=absent)
        assert api.finish_nnmf(out, ctx)["options"]["absent"] == absent
    _, ctx = api.prepare_nnmf(S.T, 2, rng=np.random.default_rng(0))
    assert api.finish_nnmf(out, ctx)["options"]["absent"] == "zero"


def test_nnlm_summary_runs_over_the_stored_entries():
    rng = np.random.default_rng(6)
    n, q, p = 25, 7, 3
    A = rng.random((n, q))
    obs = rng.random((n, q)) < 0.4
    obs[0, :] = True
    S = from_dense_pattern(A, obs)
    x = rng.random((n, p))
    coef = rng.random((p, q))
    args, ctx = api.prepare_nnlm(x, S, absent="missing", check_x=False)
    res = api.finish_nnlm({"coefficient": coef, "n_iteration": 3}, ctx)
    pred = x @ coef
    assert res["error"]["MSE"] == pytest.approx(float(np.mean((A[obs] - pred[obs]) ** 2)), rel=1e-12)
    with np.errstate(divide="ignore", invalid="ignore"):
        mkl = np.mean((A[obs] + 1e-16) * np.log((A[obs] + 1e-16) / (pred[obs] + 1e-16)) - A[obs] + pred[obs])
    assert res["error"]["MKL"] == pytest.approx(float(mkl), rel=1e-12)
    _, ctx0 = api.prepare_nnlm(x, S, check_x=False)  # zeros: the absent entries count
    res0 = api.finish_nnlm({"coefficient": coef, "n_iteration": 3}, ctx0)
    assert res0["error"]["MSE"] == pytest.approx(float(np.mean((np.where(obs, A, 0.0) - pred) ** 2)), rel=1e-12)


def test_predict_passes_absent_to_the_solver():
    obj = {"W": np.ones((30, 2)), "H": np.ones((2, 20)), "options": {"method": "scd", "loss": "mse", "absent": "missing"}}
    seen = {}

    def fake(x, y, **kw):
        seen.update(kw)
        return {"coefficients": np.zeros((x.shape[1], y.shape[1]))}
    rng = np.random.default_rng(7)
    nd = from_dense_pattern(rng.random((30, 7)), rng.random((30, 7)) < 0.3)
    api.predict_nnmf(obj, nd, which="H", absent="missing", _nnlm=fake)
    assert seen.get("absent") == "missing"
    seen.clear()
    api.predict_nnmf(obj, nd, which="H", _nnlm=fake)
    assert "absent" not in seen  # (the default: today's call)
    new_rows = from_dense_pattern(rng.random((5, 20)), rng.random((5, 20)) < 0.3)
    out = api.predict_nnmf(obj, new_rows, which="W", absent="missing", _nnlm=fake)
    assert seen.get("absent") == "missing" and out["coefficients"].shape == (5, 2)
    with pytest.raises(api.NnlmStop, match="needs a sparse newdata"):  # (a dense newdata has NA for missing entries)
        api.predict_nnmf(obj, np.ones((30, 7)), which="H", absent="missing", _nnlm=fake)
    with pytest.raises(api.NnlmStop, match="'absent' should be one of"):
        api.predict_nnmf(obj, nd, which="H", absent="na", _nnlm=fake)
    seen.clear()
    assert api.predict_nnmf(obj, which="A", absent="missing").shape == (30, 20) and not seen  # (W H: nothing is solved)


def test_new_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "nnlm_mi355x.h")).read()
    for sym in NEW:
        assert re.search(r"\bint " + sym + r"\s*\(", header), sym
        assert sym in _lib.EXPORTS
        assert hasattr(_lib.load(), sym)
    assert "matrix_absent_missing" in header
    import inspect
    for a, b in ((_lib.c_nnmf_csc, _lib.c_nnmf_csc_missing), (_lib.c_nnlm_csc, _lib.c_nnlm_csc_missing)):
        assert list(inspect.signature(a).parameters) == list(inspect.signature(b).parameters)
    assert hasattr(_lib.Handle, "set_matrix_csc_missing")


def test_new_entries_fail_loudly_without_gpu(gpu_available):
    if gpu_available:
        pytest.skip("GPU present")
    rng = np.random.default_rng(8)
    S = from_dense_pattern(rng.random((20, 10)), rng.random((20, 10)) < 0.5)
    with pytest.raises(nnlm_amd.NnlmError):
        api.nnmf(S, 2, absent="missing", check_k=False)
    with pytest.raises(nnlm_amd.NnlmError):
        api.nnlm(rng.random((20, 3)), S, absent="missing")
    with pytest.raises(nnlm_amd.NnlmError):
        _lib.c_nnmf_csc_missing(S.indptr, S.indices, S.data, S.shape, 2, None, None, None, None, [0, 0, 0], [0, 0, 0], 5, 1e-4, 1, 0, True,
                                5, 1e-9, 1, 1)
