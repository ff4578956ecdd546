"""Rank selection on held-out entries (api.nnmf_cv, nnlm_set_matrix_holdout / nnlm_holdout_errors / nnlm_c_nnmf_holdout_batch): what needs
no GPU.  The new entries are declared and exported; nnmf_cv's argument checks and refusals come before any device call; a fraction draw
is reproducible; the check_k rule on the training entries fires; ranks are packed into batches in order; and the planted-rank input of
test_gpu_cv.py has a clear minimum of the ORACLE's held-out error at its planted rank, so the GPU test is about parity, not luck."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import cv_cases as cv  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402
from oracle import ref  # noqa: E402

ERR_ARG, ERR_UNSUPPORTED = 1, 5
Z3 = [0.0, 0.0, 0.0]


def small(n=30, m=20, seed=0):
    return np.random.default_rng(seed).random((n, m))


class DuckCSC:
    def __init__(self, A):
        cols, rows = np.nonzero(A.T)
        self.indptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=A.shape[1]))])
        self.indices, self.data, self.shape = rows, A[rows, cols], A.shape

    def tocsc(self):
        return self


@pytest.fixture
def no_device(monkeypatch):
    """Any device call fails the test: the checks below must come before it."""
    def boom(*a, **k):
        raise AssertionError("a device call was reached")
    monkeypatch.setattr(_lib, "Handle", boom)
    monkeypatch.setattr(_lib, "load", boom)


def code_of(fn):
    with pytest.raises(_lib.NnlmError) as e:
        fn()
    assert "batch" in str(e.value) or e.value.code == ERR_ARG, str(e.value)
    return e.value.code


def test_new_entries_are_declared_and_exported():
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "nnlm_mi355x.h")).read()
    for name in ("nnlm_set_matrix_holdout", "nnlm_holdout_errors", "nnlm_c_nnmf_holdout_batch"):
        assert name in _lib.EXPORTS and ("int " + name + "(") in hdr
    assert "#define NNLM_ABI_VERSION 1" in hdr
    for name in ("set_matrix_holdout", "holdout_errors"):
        assert callable(getattr(_lib.Handle, name))
    assert callable(_lib.c_nnmf_holdout_batch) and callable(api.nnmf_cv)


def test_refusals_come_before_any_device_call(no_device):
    A = small()
    assert code_of(lambda: api.nnmf_cv(A, [2, 3], loss="mkl")) == ERR_UNSUPPORTED
    assert code_of(lambda: api.nnmf_cv(A, [2, 3], mask={"H": np.zeros((2, 20), dtype=bool)})) == ERR_UNSUPPORTED
    assert code_of(lambda: api.nnmf_cv(A, [2, 3], init=[{"W0": np.ones((30, 1))}, {}])) == ERR_UNSUPPORTED
    assert code_of(lambda: api.nnmf_cv(DuckCSC(A), [2, 3])) == ERR_UNSUPPORTED
    for bad in (np.nan, np.inf):
        An = A.copy()
        An[3, 4] = bad
        assert code_of(lambda: api.nnmf_cv(An, [2, 3])) == ERR_UNSUPPORTED
    assert code_of(lambda: api.nnmf_cv(small(100, 90), [65], check_k=False)) == ERR_UNSUPPORTED  # a single rank above 64


def test_argument_checks_come_before_any_device_call(no_device):
    A = small()
    for k, nrun in ((0, 1), ([], 1), ([2, 0], 1), (2, 0), ("a", 1)):
        assert code_of(lambda: api.nnmf_cv(A, k, nrun=nrun)) == ERR_ARG
    for h in (0.0, 1.0, -0.1, 1.5, np.zeros((30, 19), dtype=bool), np.zeros((30, 20))):
        assert code_of(lambda: api.nnmf_cv(A, 2, holdout=h)) == ERR_ARG
    good = {"W": np.ones((30, 2)), "H": np.ones((2, 20))}
    assert code_of(lambda: api.nnmf_cv(A, [2, 3], init=[good])) == ERR_ARG
    assert code_of(lambda: api.nnmf_cv(A, [2, 3], init=[good, good])) == ERR_ARG
    with pytest.raises(api.NnlmStop):
        api.nnmf_cv(np.zeros(5), 2)


def test_fraction_draw_is_reproducible_and_canonical():
    n, m = 50, 40
    p1 = api._holdout_pattern(0.2, n, m, np.random.default_rng(7))
    p2 = api._holdout_pattern(0.2, n, m, np.random.default_rng(7))
    p3 = api._holdout_pattern(0.2, n, m, np.random.default_rng(8))
    assert all(np.array_equal(a, b) for a, b in zip(p1, p2)) and not np.array_equal(p1[1], p3[1])
    ptr, idx = p1
    assert ptr.dtype == np.int64 and idx.dtype == np.int32 and ptr[0] == 0 and ptr[-1] == idx.size == round(0.2 * n * m)
    for j in range(m):  # strictly increasing rows within a column, in range: without replacement
        col = idx[ptr[j]:ptr[j + 1]]
        assert np.all(np.diff(col) > 0) and (col.size == 0 or (col[0] >= 0 and col[-1] < n))
    # a boolean array and an earlier result's pattern give the same structure back
    mask = np.zeros((n, m), dtype=bool)
    mask[idx, cv.pattern_cols(ptr)] = True
    for again in (api._holdout_pattern(mask, n, m, None), api._holdout_pattern(dict(indptr=ptr, indices=idx), n, m, None)):
        assert np.array_equal(again[0], ptr) and np.array_equal(again[1], idx)


def test_check_k_rule_on_the_training_entries(no_device):
    A = small(30, 20)
    mask = np.zeros((30, 20), dtype=bool)
    mask[4, :15] = True  # row 4 keeps 5 training entries: ranks up to 4 pass the rule, 5 does not
    with pytest.raises(api.NnlmStop, match="k larger than 4 is not recommended"):
        api.nnmf_cv(A, [2, 5], holdout=mask)
    with pytest.raises(api.NnlmStop, match="is not recommended"):
        api.nnmf_cv(A, [2, 3], holdout=0.9, rng=np.random.default_rng(0))
    # rank 4 passes it (and then reaches the device, which this test forbids)
    with pytest.raises(AssertionError, match="device call"):
        api.nnmf_cv(A, [2, 4], holdout=mask)


def test_packing_into_batches_is_in_order_and_complete():
    ks = list(range(1, 13))  # sum 78
    batches = api._pack_batches(ks)
    assert batches == [(0, 10), (10, 12)]
    assert [b for b0, b1 in batches for b in range(b0, b1)] == list(range(12))
    assert all(sum(ks[b0:b1]) <= 64 for b0, b1 in batches)
    assert api._pack_batches([64]) == [(0, 1)] and api._pack_batches([32, 32, 1]) == [(0, 2), (2, 3)]
    assert api._pack_batches([8] * 8) == [(0, 8)] and api._pack_batches([60, 5, 60]) == [(0, 1), (1, 2), (2, 3)]
    with pytest.raises(_lib.NnlmError) as e:
        api._pack_batches([3, 65])
    assert e.value.code == ERR_UNSUPPORTED


def test_planted_rank_has_a_clear_minimum_of_the_oracles_held_out_error():
    """The oracle alone: held-out MSE over k = 1..6 is lowest at the planted rank 3, at most 0.8 of the runner-up."""
    ks = list(range(1, 7))
    A, inits = cv.planted(ks)
    ptr, idx = api._holdout_pattern(cv.FRACTION, cv.N, cv.M, np.random.default_rng(cv.SEED))
    cv.assert_trainable(A, ptr, idx, max(ks))
    An = cv.with_nan(A, ptr, idx)
    mse = []
    for k, (W, H) in zip(ks, inits):
        o = ref.c_nnmf(An, k, W, H, None, None, Z3, Z3, cv.ITERS, -1.0, 1, 0, True, 50, 1e-9, 1, cv.TRACE)
        mse.append(cv.numpy_holdout_errors(A, ptr, idx, o["W"], o["H"])[0])
    order = np.argsort(mse)
    print("oracle held-out MSE, k = 1..6:", ["%.3e" % v for v in mse], "ratio %.3f" % (mse[order[0]] / mse[order[1]]))
    assert ks[order[0]] == cv.RANK
    assert mse[order[0]] / mse[order[1]] <= 0.8
