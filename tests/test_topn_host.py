"""Top-N scores and listed entries of a fit, the part that needs no GPU: the C header, the Python argument
refusals (which fire before any device call), the numpy restatement topn_oracle on hand-made cases, and the near-tie condition of every
random case tests/test_gpu_topn.py uses -- evaluated from the oracle alone, its exempt share asserted to be zero."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import topn_cases as tc  # noqa: E402
import sparse_cases as sc  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402

ROOT = os.path.dirname(HERE)


def test_header_declares_both_entries_and_keeps_the_abi_version():
    text = open(os.path.join(ROOT, "include", "nnlm_mi355x.h")).read()
    assert re.search(r"^#define NNLM_ABI_VERSION 1\s*$", text, re.M)
    flat = re.sub(r"\s+", " ", text)
    assert "int nnlm_predict_entries(nnlm_handle *h, long long count, const int *rows, const int *cols, double *out);" in flat
    assert ("int nnlm_top_n(nnlm_handle *h, int by, int n_top, const int *lines, long long n_lines, int exclude, int *idx_out, "
            "double *score_out);") in flat
    assert "nnlm_predict_entries" in _lib.EXPORTS and "nnlm_top_n" in _lib.EXPORTS


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to open a handle is an error: the refusals below must fire before it."""
    def boom(*a, **k):
        raise AssertionError("a device call was made before the arguments were checked")
    monkeypatch.setattr(_lib, "Handle", boom)
    monkeypatch.setattr(_lib, "load", boom)


def _fit(n=6, m=5, k=2):
    rng = np.random.default_rng(1)
    return dict(W=rng.random((n, k)), H=rng.random((k, m)))


def _seen(n, m):
    return sc.Csc(sc.csc_from_pattern(np.eye(n, m, dtype=bool), np.ones((n, m))))


def test_python_refusals_fire_without_a_device(no_device):
    fit = _fit()
    stop = (api.NnlmStop, ValueError)
    with pytest.raises(stop, match="same length"):
        api.predict_entries(fit, [0, 1], [0])
    with pytest.raises(stop, match="integers"):
        api.predict_entries(fit, [0.5, 1.0], [0, 1])
    with pytest.raises(stop, match="one-dimensional"):
        api.predict_entries(fit, [[0, 1]], [[0, 1]])
    with pytest.raises(stop, match="rows .*out of range"):
        api.predict_entries(fit, [6], [0])
    with pytest.raises(stop, match="cols .*out of range"):
        api.predict_entries(fit, [0], [-1])
    with pytest.raises(stop, match="'column' or 'row'"):
        api.top_n(fit, 3, by="col")
    with pytest.raises(stop, match="integers"):
        api.top_n(fit, 3, lines=np.array([0.0, 1.0]))
    with pytest.raises(stop, match="lines .*out of range"):
        api.top_n(fit, 3, by="column", lines=[5])
    with pytest.raises(stop, match="lines .*out of range"):
        api.top_n(fit, 3, by="row", lines=[6])
    with pytest.raises(stop, match="n_top"):
        api.top_n(fit, 0)
    with pytest.raises(stop, match="n_top"):
        api.top_n(fit, 129)
    with pytest.raises(stop, match="does not match the fit"):
        api.top_n(fit, 3, seen=_seen(5, 6))
    with pytest.raises(stop, match="tocsc"):
        api.top_n(fit, 3, seen=np.zeros((6, 5)))
    with pytest.raises(stop, match="W .*and H"):
        api.top_n(dict(W=np.zeros((6, 2)), H=np.zeros((3, 5))), 3)


def test_handle_argument_checks_are_value_errors():
    with pytest.raises(ValueError, match="integers"):
        _lib.index_array(np.array([1.5]), "rows")
    with pytest.raises(ValueError, match="32 bits"):
        _lib.index_array(np.array([2 ** 40]), "rows")
    with pytest.raises(ValueError, match="'column' or 'row'"):
        _lib.by_code("both")
    assert _lib.index_array([], "rows").dtype == np.int32 and _lib.by_code("row") == 1 and _lib.by_code("column") == 0


def test_oracle_orders_ties_by_ascending_index_and_pads():
    W = np.array([[1.0], [2.0], [2.0], [0.0], [2.0]])
    H = np.array([[1.0, 0.0, 3.0]])
    idx, score = tc.topn_oracle(W, H, 3, "column")
    assert idx.tolist() == [[1, 2, 4], [0, 1, 2], [1, 2, 4]]
    assert score.tolist() == [[2.0, 2.0, 2.0], [0.0, 0.0, 0.0], [6.0, 6.0, 6.0]]
    idx, score = tc.topn_oracle(W, H, 7, "column", lines=[2])
    assert idx.tolist() == [[1, 2, 4, 0, 3, -1, -1]]
    assert score[0, :5].tolist() == [6.0, 6.0, 6.0, 3.0, 0.0] and np.isnan(score[0, 5:]).all()
    idx, score = tc.topn_oracle(W, H, 2, "row", lines=[3, 1])
    assert idx.tolist() == [[0, 1], [2, 0]] and score.tolist() == [[0.0, 0.0], [6.0, 2.0]]


def test_oracle_excludes_stored_entries_and_nan():
    W = np.array([[1.0], [2.0], [3.0], [4.0]])
    H = np.array([[1.0, 1.0]])
    P = np.array([[0, 1], [0, 1], [1, 1], [0, 1]], dtype=bool)
    seen = sc.csc_from_pattern(P, np.zeros((4, 2)))  # (stored zeros are stored)
    idx, score = tc.topn_oracle(W, H, 2, "column", seen=seen)
    assert idx.tolist() == [[3, 1], [-1, -1]] and score[0].tolist() == [4.0, 2.0] and np.isnan(score[1]).all()
    idx, _ = tc.topn_oracle(W, H, 2, "row", seen=seen)
    assert idx.tolist() == [[0, -1], [0, -1], [-1, -1], [0, -1]]
    W2 = W.copy()
    W2[3, 0] = np.nan
    idx, _ = tc.topn_oracle(W2, H, 4, "column", lines=[0])
    assert idx.tolist() == [[2, 1, 0, -1]]


@pytest.mark.parametrize("i", range(len(tc.RANDOM_SHAPES)))
def test_no_line_of_the_random_cases_is_a_near_tie(i):
    """The GPU file asks exact index equality of every line of these cases: the exemption rule (two consecutive oracle scores among the
    best N + 1 within 2 tau) must exempt none of them, with and without exclusion, both ways."""
    c = tc.random_case(i)
    for by in tc.BYS:
        for seen in (None, c["seen"]):
            ex = tc.exempt_lines(c["W"], c["H"], c["N"], by, seen)
            gap, t = tc.smallest_gap(c["W"], c["H"], c["N"], by, seen)
            print(f"case {i} by={by} seen={seen is not None}: smallest gap {gap:.3e}, largest tau {t:.3e}, exempt {int(ex.sum())}/{ex.size}")
            assert ex.mean() == 0.0
