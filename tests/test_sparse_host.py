"""Sparse input on the host side (no GPU): duck-typed CSC input, its canonicalisation, the argument tuples of the sparse entries, the
refusals of the wrapper and the loud failure of the sparse entries without a device."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402


class Coo:
    """Minimal duck-typed sparse matrix: only tocsc() -> (indptr, indices, data, shape), possibly with duplicates and unsorted rows."""

    def __init__(self, rows, cols, vals, shape):
        self.rows, self.cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
        self.vals, self.shape = np.asarray(vals, dtype=float), shape

    def tocsc(self):
        order = np.argsort(self.cols, kind="stable")  # columns grouped, rows left in the given order (unsorted, duplicates kept)
        r, c, v = self.rows[order], self.cols[order], self.vals[order]
        indptr = np.zeros(self.shape[1] + 1, dtype=np.int32)
        np.cumsum(np.bincount(c, minlength=self.shape[1]), out=indptr[1:])

        class _C:
            pass
        out = _C()
        out.indptr, out.indices, out.data, out.shape = indptr, r.astype(np.int32), v, self.shape
        return out

    @property
    def T(self):
        return Coo(self.cols, self.rows, self.vals, (self.shape[1], self.shape[0]))

    def toarray(self):
        a = np.zeros(self.shape)
        np.add.at(a, (self.rows, self.cols), self.vals)
        return a


def random_coo(n, m, nnz, seed, dup=True):
    rng = np.random.default_rng(seed)
    r, c = rng.integers(0, n, nnz), rng.integers(0, m, nnz)
    if dup and nnz > 2:
        r[1], c[1] = r[0], c[0]  # one duplicate entry at least
    return Coo(r, c, rng.random(nnz), (n, m))


def test_duck_typing_and_canonical_csc():
    A = random_coo(30, 20, 150, 1)
    assert api.is_sparse(A) and not api.is_sparse(A.toarray()) and not api.is_sparse([[1.0]])
    c = api.as_csc(A)
    assert c.indptr.dtype == np.int64 and c.indices.dtype == np.int32 and c.data.dtype == np.float64 and c.shape == (30, 20)
    assert c.indptr[0] == 0 and c.indptr[-1] == c.indices.size == c.data.size
    for j in range(20):
        rows = c.indices[c.indptr[j]:c.indptr[j + 1]]
        assert np.all(np.diff(rows) > 0), j  # sorted, duplicates summed
    np.testing.assert_allclose(api.csc_toarray(c), A.toarray(), rtol=0, atol=1e-15)


def test_canonical_csc_edges():
    empty = api.as_csc(Coo([], [], [], (4, 3)))
    assert empty.indptr.tolist() == [0, 0, 0, 0] and empty.indices.size == 0
    one = api.as_csc(Coo([2, 2, 0], [1, 1, 1], [1.0, 2.0, 5.0], (3, 2)))
    assert one.indptr.tolist() == [0, 0, 2] and one.indices.tolist() == [0, 2] and one.data.tolist() == [5.0, 3.0]


def test_scipy_matrices_qualify_when_present():
    sp = pytest.importorskip("scipy.sparse")
    M = sp.random(40, 25, density=0.1, random_state=3, format="coo")
    for obj in (M, M.tocsr(), sp.csc_array(M)):
        c = api.as_csc(obj)
        np.testing.assert_array_equal(api.csc_toarray(c), M.toarray())


def test_prepare_nnmf_sparse_argument_tuple():
    A = random_coo(30, 20, 150, 2)
    args, ctx = api.prepare_nnmf(A, 3, rng=np.random.default_rng(0))
    assert isinstance(args[0], api.CSC) and len(args) == 17
    np.testing.assert_allclose(api.csc_toarray(args[0]), A.toarray(), atol=1e-15)
    dense_args, _ = api.prepare_nnmf(A.toarray(), 3, rng=np.random.default_rng(0))
    for a, b in zip(args[1:], dense_args[1:]):  # everything after A is what the dense call gets
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    # (the flattened CSC + the rest is exactly the argument list of _lib.c_nnmf_csc)
    import inspect
    params = list(inspect.signature(_lib.c_nnmf_csc).parameters)
    assert params[:4] == ["indptr", "indices", "data", "shape"] and len(params) == 4 + 16 + 1


def test_prepare_nnlm_sparse_argument_tuple():
    rng = np.random.default_rng(4)
    x = rng.random((30, 4))
    y = random_coo(30, 6, 40, 5)
    args, ctx = api.prepare_nnlm(x, y, check_x=False)
    assert isinstance(args[1], api.CSC) and args[1].shape == (30, 6) and len(args) == 9
    assert not ctx["is_y_vector"]
    import inspect
    params = list(inspect.signature(_lib.c_nnlm_csc).parameters)
    assert params[:5] == ["x", "y_indptr", "y_indices", "y_data", "y_shape"] and len(params) == 5 + 7 + 1
    with pytest.raises(api.NnlmStop, match="Dimensions of x and y"):
        api.prepare_nnlm(x[:29], y, check_x=False)


def test_mkl_refusal_names_the_restriction():
    A = random_coo(30, 20, 150, 6)
    with pytest.raises(api.NnlmStop, match="loss = 'mse' only"):
        api.prepare_nnmf(A, 2, loss="mkl")
    with pytest.raises(api.NnlmStop, match="loss = 'mse' only"):
        api.prepare_nnlm(np.ones((30, 2)), A, loss="mkl", check_x=False)


def test_non_finite_sparse_values_are_refused():
    A = Coo([0, 1], [0, 1], [1.0, np.nan], (3, 3))
    with pytest.raises(api.NnlmStop, match="non-finite"):
        api.prepare_nnmf(A, 1)


def test_check_k_uses_min_n_m():
    A = random_coo(12, 5, 30, 7)
    with pytest.raises(api.NnlmStop, match="k larger than 5"):
        api.prepare_nnmf(A, 6)
    api.prepare_nnmf(A, 5)
    api.prepare_nnmf(A, 6, check_k=False)


def test_predict_checks_sparse_newdata_shape():
    obj = {"W": np.ones((30, 2)), "H": np.ones((2, 20)), "options": {"method": "scd", "loss": "mse"}}
    seen = {}

    def fake(x, y, **kw):
        seen["x"], seen["y"] = x, y
        return {"coefficients": np.zeros((x.shape[1], y.shape[1]))}
    nd = random_coo(30, 7, 20, 8)
    api.predict_nnmf(obj, nd, which="H", _nnlm=fake)
    assert seen["y"] is nd  # passed on as it is (duck-typed in nnlm())
    with pytest.raises(api.NnlmStop):
        api.predict_nnmf(obj, random_coo(29, 7, 20, 8), which="H", _nnlm=fake)
    out = api.predict_nnmf(obj, random_coo(5, 20, 20, 9), which="W", _nnlm=fake)
    assert out["coefficients"].shape == (5, 2)


def test_sparse_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "nnlm_mi355x.h")).read()
    for sym in ("nnlm_set_matrix_csc", "nnlm_c_nnmf_csc", "nnlm_c_nnlm_csc"):
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert sym in _lib.EXPORTS
        assert hasattr(_lib.load(), sym)
    assert "long long *colptr" in header


def test_sparse_entries_fail_loudly_without_gpu(gpu_available):
    if gpu_available:
        pytest.skip("GPU present")
    A = random_coo(20, 10, 40, 10)
    with pytest.raises(nnlm_amd.NnlmError):
        api.nnmf(A, 2)
    with pytest.raises(nnlm_amd.NnlmError):
        api.nnlm(np.random.default_rng(0).random((20, 3)), A)
    c = api.as_csc(A)
    with pytest.raises(nnlm_amd.NnlmError):
        _lib.c_nnmf_csc(*c, 2, None, None, None, None, [0, 0, 0], [0, 0, 0], 5, 1e-4, 1, 0, True, 5, 1e-9, 1, 1)
