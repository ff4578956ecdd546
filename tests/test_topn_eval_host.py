"""Ranking evaluation of top-N lists against held-out entries, the part that needs no GPU: the C header against the
binding, api.holdout_split, the numpy restatement eval_oracle on hand-made lists with known answers, and the Python argument refusals
of api.evaluate_top_n (which fire before any device call)."""
import math
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import topn_eval_cases as ec  # noqa: E402
import sparse_cases as sc  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402

ROOT = os.path.dirname(HERE)


def test_header_declares_the_entry_and_the_binding_matches_it():
    text = open(os.path.join(ROOT, "include", "nnlm_mi355x.h")).read()
    assert re.search(r"^#define NNLM_ABI_VERSION 1\s*$", text, re.M)
    flat = re.sub(r"\s+", " ", text)
    assert ("int nnlm_top_n_eval(nnlm_handle *h, int by, const int *cutoffs, int n_cut, const int *lines, long long n_lines, int exclude, "
            "const long long *held_ptr, const int *held_idx, double *agg_out, long long *n_eval_out, double *line_out);") in flat
    assert "nnlm_top_n_eval" in _lib.EXPORTS
    assert _lib.TOPN_EVAL_MAX_CUT == 8 and _lib.TOPN_MAX == 128
    lib = _lib.load()
    assert len(lib.nnlm_top_n_eval.argtypes) == 12 and hasattr(_lib.Handle, "top_n_eval")


# ---- holdout_split -----------------------------------------------------------------------------------------------------------------------
def _ratings(n=60, m=45, seed=3):
    rng = np.random.default_rng(seed)
    P = sc._powerlaw(n, m, rng, False)
    P[:, 4] = False            # an empty column
    P[:, 5] = False
    P[7, 5] = True             # a column with one entry
    P[9, :] = False            # an empty row
    return P, sc.Csc(sc.csc_from_pattern(P, rng.random((n, m)) + 0.5))


@pytest.mark.parametrize("by", ("column", "row"))
@pytest.mark.parametrize("per_line,min_keep", ((1, 1), (3, 2), (2, 0), (100, 1)))
def test_holdout_split_counts_and_patterns(by, per_line, min_keep):
    P, A = _ratings()
    train, held = api.holdout_split(A, per_line=per_line, by=by, min_keep=min_keep, rng=11)
    assert isinstance(train, api.CSC) and isinstance(held, api.CSC) and train.shape == held.shape == A.shape
    Pt, Ph = sc.pattern_of(tuple(train)), sc.pattern_of(tuple(held))
    assert not (Pt & Ph).any() and np.array_equal(Pt | Ph, P)
    full = sc.densify((A.indptr, A.indices, A.data, A.shape), "zero")
    assert np.array_equal(sc.densify(tuple(train), "zero") + sc.densify(tuple(held), "zero"), full)  # (the values went along)
    axis = 0 if by == "column" else 1
    stored, gave = P.sum(axis=axis), Ph.sum(axis=axis)
    want = np.where(stored > min_keep, np.minimum(per_line, stored - min_keep), 0)
    assert np.array_equal(gave, want)
    assert (Pt.sum(axis=axis)[stored > 0] >= np.minimum(min_keep, stored[stored > 0])).all()
    assert (gave[stored <= min_keep] == 0).all() and (stored <= min_keep).any() and (want > 0).any()
    for c in (train, held):  # canonical CSC
        assert c.indptr.dtype == np.int64 and c.indices.dtype == np.int32 and c.indptr[-1] == c.indices.size == c.data.size
        for j in range(c.shape[1]):
            assert (np.diff(c.indices[c.indptr[j]:c.indptr[j + 1]]) > 0).all()


def test_holdout_split_is_a_function_of_the_rng_state():
    _, A = _ratings()
    a, b = api.holdout_split(A, 2, rng=5), api.holdout_split(A, 2, rng=5)
    c = api.holdout_split(A, 2, rng=np.random.default_rng(5))
    d = api.holdout_split(A, 2, rng=6)
    for x, y in ((a, b), (a, c)):
        assert all(np.array_equal(u, v) for s, t in zip(x, y) for u, v in zip(s[:3], t[:3]))
    assert not np.array_equal(a[1].indices, d[1].indices)
    g = np.random.default_rng(5)
    first, second = api.holdout_split(A, 2, rng=g), api.holdout_split(A, 2, rng=g)  # (the generator moved on)
    assert np.array_equal(first[1].indices, a[1].indices) and not np.array_equal(second[1].indices, a[1].indices)


def test_holdout_split_results_are_sparse_arguments_and_refusals():
    _, A = _ratings()
    train, held = api.holdout_split(A, rng=1)
    assert api.is_sparse(train) and api.as_csc(held).indices.size == held.indices.size
    with pytest.raises(api.NnlmStop, match="tocsc"):
        api.holdout_split(np.zeros((3, 3)))
    with pytest.raises(api.NnlmStop, match="'column' or 'row'"):
        api.holdout_split(A, by="both")
    with pytest.raises(api.NnlmStop, match="per_line"):
        api.holdout_split(A, per_line=0)


# ---- eval_oracle on lists with known answers -------------------------------------------------------------------------------------------
def d(p):
    return 1.0 / math.log2(p + 2.0)


def test_oracle_perfect_list_scores_one_everywhere():
    o = ec.eval_oracle([[4, 2, 9]], [{2, 4, 9}], (1, 2, 3))
    assert o["n_evaluated"] == 1 and o["t"].tolist() == [3] and o["first"].tolist() == [0] and o["hits"].tolist() == [[1, 2, 3]]
    assert np.allclose(o["agg"][:, [0, 2, 3, 4, 5]], 1.0, rtol=0, atol=1e-15)
    assert np.allclose(o["agg"][:, 1], [1 / 3, 2 / 3, 1.0])


def test_oracle_no_hit_scores_zero():
    o = ec.eval_oracle([[1, 2, 3, 4]], [{0, 7}], (2, 4))
    assert o["first"].tolist() == [-1] and o["hits"].tolist() == [[0, 0]] and np.array_equal(o["agg"], np.zeros((2, 6))) and o["n_evaluated"] == 1


def test_oracle_known_values_with_more_held_out_than_the_cutoff():
    # hits at positions 1 and 3 of 5, t = 7 > c
    o = ec.eval_oracle([[10, 3, 11, 5, 12]], [{3, 5, 20, 21, 22, 23, 24}], (1, 2, 5))
    assert o["t"].tolist() == [7] and o["first"].tolist() == [1] and o["hits"].tolist() == [[0, 1, 2]]
    assert o["dcg"][0].tolist() == [0.0, d(1), d(1) + d(3)] and o["apn"][0].tolist() == [0.0, 0.5, 0.5 + 2 / 4]
    a = o["agg"]
    assert a[:, 0].tolist() == [0.0, 0.5, 0.4] and a[:, 1].tolist() == [0.0, 1 / 7, 2 / 7] and a[:, 2].tolist() == [0.0, 1.0, 1.0]
    ideal5 = d(0) + d(1) + d(2) + d(3) + d(4)  # min(c, t) = 5 terms, not 7
    assert a[:, 3].tolist() == [0.0, d(1) / (d(0) + d(1)), (d(1) + d(3)) / ideal5]
    assert a[:, 4].tolist() == [0.0, 0.5 / 2, 1.0 / 5] and a[:, 5].tolist() == [0.0, 0.5, 0.5]  # (RR = 0 while first is beyond the cutoff)


def test_oracle_padding_never_hits_and_lines_without_held_out_entries_are_not_evaluated():
    lists = [[3, -1, -1, -1], [0, 1, 2, 3], [5, 6, -1, -1]]
    o = ec.eval_oracle(lists, [{3}, set(), {6, 9}], (1, 4))
    assert o["n_evaluated"] == 2 and o["t"].tolist() == [1, 0, 2] and o["first"].tolist() == [0, -1, 1]
    assert o["hits"].tolist() == [[1, 1], [0, 0], [0, 1]]
    # line 0: everything 1 but the precision 1 / c (t = 1: the ideal list has one entry); line 2 at c = 4: precision 1/4, recall 1/2, NDCG d(1) / (d(0) + d(1)), AP (1/2) / 2, RR 1/2
    want4 = [(0.25 + 0.25) / 2, (1.0 + 0.5) / 2, 1.0, (1.0 + d(1) / (d(0) + d(1))) / 2, (1.0 + 0.25) / 2, (1.0 + 0.5) / 2]
    assert np.allclose(o["agg"][1], want4, rtol=1e-15, atol=0) and o["agg"][0].tolist() == [0.5] * 6
    e = ec.eval_oracle([[1, 2]], [set()], (2,))
    assert e["n_evaluated"] == 0 and np.isnan(e["agg"]).all()
    assert -1 not in (set(lists[0]) & {3})  # (and a held-out "-1" cannot exist: indices are >= 0)


def test_oriented_patterns_and_held_sets():
    P = np.zeros((4, 3), dtype=bool)
    P[[0, 3], 1] = True
    P[2, 2] = True
    ptr, idx = ec.oriented(P, "column")
    assert ptr.tolist() == [0, 0, 2, 3] and idx.tolist() == [0, 3, 2] and ptr.dtype == np.int64 and idx.dtype == np.int32
    ptr, idx = ec.oriented(P, "row")
    assert ptr.tolist() == [0, 1, 1, 2, 3] and idx.tolist() == [1, 2, 1]
    assert [s.tolist() for s in ec.held_sets(ptr, idx, [3, 1])] == [[1], []]


# ---- Python refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to open a handle is an error: the refusals below must fire before it."""
    def boom(*a, **k):
        raise AssertionError("a device call was made before the arguments were checked")
    monkeypatch.setattr(_lib, "Handle", boom)
    monkeypatch.setattr(_lib, "load", boom)


class FakeDevice:
    type, index = "cuda", 0


class FakeDeviceTensor:
    """A tensor-like object in device memory: data_ptr(), stride() in elements, shape, dtype, device."""
    shape, dtype, device = (6, 5), "fake.float64", FakeDevice()

    def data_ptr(self):
        return 4096

    def stride(self):
        return (5, 1)


def test_python_refusals_fire_without_a_device(no_device):
    rng = np.random.default_rng(1)
    fit = dict(W=rng.random((6, 2)), H=rng.random((2, 5)))
    held = sc.Csc(sc.csc_from_pattern(np.eye(6, 5, dtype=bool), np.ones((6, 5))))
    stop = api.NnlmStop
    with pytest.raises(stop, match="heldout .*does not match the fit"):
        api.evaluate_top_n(fit, sc.Csc(sc.csc_from_pattern(np.eye(5, 6, dtype=bool), np.ones((5, 6)))))
    with pytest.raises(stop, match="seen .*does not match the fit"):
        api.evaluate_top_n(fit, held, seen=sc.Csc(sc.csc_from_pattern(np.eye(5, 6, dtype=bool), np.ones((5, 6)))))
    with pytest.raises(stop, match="heldout must be a sparse matrix .*tocsc"):
        api.evaluate_top_n(fit, np.zeros((6, 5)))
    with pytest.raises(stop, match="seen must be a sparse matrix .*tocsc"):
        api.evaluate_top_n(fit, held, seen=np.zeros((6, 5)))
    with pytest.raises(stop, match="'column' or 'row'"):
        api.evaluate_top_n(fit, held, by="col")
    with pytest.raises(stop, match="lines .*out of range"):
        api.evaluate_top_n(fit, held, by="row", lines=[6])
    for bad in (0, 129, (1, 129), (0, 5), -3):
        with pytest.raises(stop, match=r"n_top must be in 1 \.\. 128"):
            api.evaluate_top_n(fit, held, bad)
    for bad in ((5, 5), (10, 5), (1, 3, 2)):
        with pytest.raises(stop, match="ascending"):
            api.evaluate_top_n(fit, held, bad)
    with pytest.raises(stop, match="1 .. 8"):
        api.evaluate_top_n(fit, held, tuple(range(1, 10)))
    with pytest.raises(stop, match="1 .. 8"):
        api.evaluate_top_n(fit, held, ())
    with pytest.raises(stop, match="integers"):
        api.evaluate_top_n(fit, held, 2.5)
    assert _lib.is_device_array(FakeDeviceTensor())
    with pytest.raises(stop, match="evaluate_top_n: heldout lives in device memory"):
        api.evaluate_top_n(fit, FakeDeviceTensor())
    with pytest.raises(stop, match="evaluate_top_n: seen lives in device memory"):
        api.evaluate_top_n(fit, held, seen=FakeDeviceTensor())
