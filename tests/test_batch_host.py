"""nnmf_batch argument checks that need no GPU: the batch's own refusals (NNLM_ERR_UNSUPPORTED / NNLM_ERR_ARG) are raised before the
library is touched, and every member's arguments go through prepare_nnmf, so a member gets the errors a solo nnmf() call gets."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnlm_amd import _lib, api  # noqa: E402

ERR_ARG, ERR_UNSUPPORTED = 1, 5


def small(n=30, m=20, seed=0):
    return np.random.default_rng(seed).random((n, m))


class DuckCSC:
    """A sparse matrix as api.is_sparse sees one (anything with tocsc()); no scipy needed."""

    def __init__(self, A):
        cols, rows = np.nonzero(A.T)
        self.indptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=A.shape[1]))])
        self.indices, self.data, self.shape = rows, A[rows, cols], A.shape

    def tocsc(self):
        return self


def code_of(fn):
    with pytest.raises(_lib.NnlmError) as e:
        fn()
    return e.value.code


def test_constants_match_the_header():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nnlm_mi355x.h")).read()
    assert _lib.ERR_ARG == ERR_ARG and _lib.ERR_UNSUPPORTED == ERR_UNSUPPORTED and _lib.BATCH_MAX == 64
    for name in ("nnlm_set_factors_batch", "nnlm_get_factors_batch", "nnlm_run_batch", "nnlm_c_nnmf_batch"):
        assert name in _lib.EXPORTS and ("int " + name + "(") in hdr


@pytest.mark.parametrize("k,nrun,want", [(3, 1, [3]), (2, 3, [2, 2, 2]), ([1, 4], 2, [1, 1, 4, 4]), (range(1, 11), 1, list(range(1, 11))),
                                         (np.int64(5), 2, [5, 5])])
def test_member_list(k, nrun, want):
    assert api._batch_rank_list(k, nrun) == want


@pytest.mark.parametrize("k,nrun", [(0, 1), ([], 1), ([2, 0], 1), (-1, 1), (2, 0), (1, 65), ("a", 1), ([[1, 2]], 1)])
def test_bad_k_list_is_an_argument_error(k, nrun):
    assert code_of(lambda: api.nnmf_batch(small(), k, nrun=nrun)) == ERR_ARG


def test_mismatched_init_is_an_argument_error():
    A = small()
    good = {"W": np.ones((30, 2)), "H": np.ones((2, 20))}
    assert code_of(lambda: api.nnmf_batch(A, [2, 3], init=[good])) == ERR_ARG  # one dict for two members
    assert code_of(lambda: api.nnmf_batch(A, 2, init=good)) == ERR_ARG  # a dict, not a list
    assert code_of(lambda: api.nnmf_batch(A, [2, 3], init=[good, good])) == ERR_ARG  # member 1 has rank 3
    assert code_of(lambda: api.nnmf_batch(A, 2, init=[{"H": np.ones((2, 21))}])) == ERR_ARG
    assert code_of(lambda: _lib._batch_blocks([np.ones((30, 2))], [(30, 2), (30, 3)], "W")) == ERR_ARG


@pytest.mark.parametrize("what", ["kl", "na", "inf", "sparse", "mask", "W0", "H0", "sum65"])
def test_unsupported_inputs_are_refused(what):
    A, k, kw = small(), [2, 3], {}
    if what == "kl":
        kw["loss"] = "mkl"
    elif what == "na":
        A[3, 4] = np.nan
    elif what == "inf":
        A[0, 0] = np.inf
    elif what == "sparse":
        A = DuckCSC(A)
    elif what == "mask":
        kw["mask"] = {"W": np.zeros((30, 2), dtype=bool)}
    elif what == "W0":
        kw["init"] = [{"W0": np.ones((30, 1))}, {}]
    elif what == "H0":
        kw["init"] = [{}, {"H0": np.ones((1, 20))}]
    elif what == "sum65":
        A, k = small(80, 70), [33, 32]
    with pytest.raises(_lib.NnlmError) as e:
        api.nnmf_batch(A, k, **kw)
    assert e.value.code == ERR_UNSUPPORTED
    assert "batch" in str(e.value)


@pytest.mark.parametrize("bad", [dict(A="1d"), dict(method="foo"), dict(k=25), dict(alpha="x"), dict(trace="x")])
def test_member_arguments_get_the_solo_errors(bad):
    """prepare_nnmf checks every member: the exception type and message are nnmf()'s."""
    A = small()
    if bad.get("A") == "1d":
        A = A[:, 0]
    k = bad.get("k", 2)
    opts = {key: v for key, v in bad.items() if key not in ("A", "k")}
    with pytest.raises(Exception) as solo:
        api.prepare_nnmf(A, k, **opts)
    with pytest.raises(type(solo.value)) as batch:
        api.nnmf_batch(A, k, **opts)
    assert str(batch.value) == str(solo.value)


def test_matrix_is_checked_and_converted_once(monkeypatch):
    """An integer count matrix is converted to fp64 once for the whole batch, not once per member; every member (and the C call)
    sees that one array.  The library call is stubbed: no GPU."""
    A = np.random.default_rng(1).integers(0, 20, size=(30, 20))
    calls, seen = [], {}
    real = api._nnmf_matrix

    def counting(A_, loss):
        calls.append(A_)
        return real(A_, loss)

    def fake_batch(A_, ks, W, H, *rest, callbacks=None):
        seen["A"], seen["W"] = A_, W
        return [dict(W=w, H=h, mse_error=np.ones(1), mkl_error=np.ones(1), target_error=np.full(1, float(b)),
                     average_epoch=np.ones(1), n_iteration=1, warning=False) for b, (w, h) in enumerate(zip(W, H))]

    monkeypatch.setattr(api, "_nnmf_matrix", counting)
    monkeypatch.setattr(_lib, "c_nnmf_batch", fake_batch)
    res, best = api.nnmf_batch(A, [2, 3], nrun=3, rng=np.random.default_rng(0))
    assert len(calls) == 1 and calls[0] is A
    assert seen["A"].dtype == np.float64 and seen["A"].shape == (30, 20) and np.array_equal(seen["A"], A)
    assert len(res) == 6 and best == 0 and [w.shape[1] for w in seen["W"]] == [2, 2, 2, 3, 3, 3]
