"""Top-N scores and listed entries of a fit on the MI355X: nnlm_top_n, nnlm_predict_entries, api.top_n and
api.predict_entries against the numpy restatement of tests/topn_cases.py.  Run with `pytest -m gpu`.

Exact family: integer factors, so `idx` and `score` equal the oracle's exactly, tie order and (-1, NaN) padding included.  Random family:
scores within tau_ij = 4 k eps sum_q |w_iq h_qj| of numpy's; exact index equality on every line that the near-tie rule does not exempt
(tests/test_topn_host.py asserts from the oracle alone that it exempts none).  Geometry invariance: bit-identical results whatever lines
are asked for and however the candidates are sliced."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import topn_cases as tc  # noqa: E402
import sparse_cases as sc  # noqa: E402
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = [("f64", _lib.PREC_F64), ("f32", _lib.PREC_F32)]
MODE_IDS = [m[0] for m in MODES]
ERR_ARG, ERR_UNSUPPORTED = 1, 5
Z3 = [0.0, 0.0, 0.0]


@pytest.fixture(autouse=True)
def _default_precision(monkeypatch):
    monkeypatch.delenv("NNLM_PRECISION", raising=False)


def open_handle(prec, W, H, seen=None, missing=False):
    """A handle with the factors and `seen` (a CSC tuple; None: the empty pattern) as its sparse matrix."""
    n, m = W.shape[0], H.shape[1]
    h = nnlm_amd.Handle(0, prec)
    if seen is None:
        seen = (np.zeros(m + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), (n, m))
    (h.set_matrix_csc_missing if missing else h.set_matrix_csc)(*seen)
    h.set_factors(W.shape[1], W, H)
    return h


def assert_same(got, want, what):
    gi, gs = got
    wi, ws = want
    assert gi.dtype == np.int32 and gs.dtype == np.float64 and gi.shape == wi.shape and gs.shape == ws.shape, what
    bad = np.flatnonzero((gi != wi).any(axis=1) | ~((gs == ws) | (np.isnan(gs) & np.isnan(ws))).all(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} lines differ, first {bad[0]}: got {gi[bad[0]]} {gs[bad[0]]}, want {wi[bad[0]]} {ws[bad[0]]}"


# ---- exact family ------------------------------------------------------------------------------------------------------------------------
PATTERNS = tc.exact_patterns()


@pytest.mark.parametrize("mode,prec", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("pi", range(len(PATTERNS)), ids=[p[0] for p in PATTERNS])
def test_exact_with_patterns(mode, prec, pi):
    name, seen = PATTERNS[pi]
    n, m = seen[3]
    k = tc.EXACT_RANKS[pi % len(tc.EXACT_RANKS)]
    W, H = tc.integer_factors(n, m, k, np.random.default_rng(100 + pi))
    missing = k <= 64 and pi % 2 == 1  # (either absent semantics: the stored pattern is what is excluded)
    with open_handle(prec, W, H, seen, missing) as h:
        for by in tc.BYS:
            for n_top in tc.EXACT_NTOPS:
                assert_same(h.top_n(n_top, by=by, exclude=True), tc.topn_oracle(W, H, n_top, by, None, seen), f"{name} k={k} {by} N={n_top} excl")
            assert_same(h.top_n(10, by=by), tc.topn_oracle(W, H, 10, by), f"{name} k={k} {by} N=10")


@pytest.mark.parametrize("mode,prec", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("k", tc.EXACT_RANKS)
def test_exact_ranks(mode, prec, k):
    n, m = 257, 130
    rng = np.random.default_rng(200 + k)
    W, H = tc.integer_factors(n, m, k, rng)
    seen = sc.csc_from_pattern(rng.random((n, m)) < 0.3, np.ones((n, m)))
    with open_handle(prec, W, H, seen) as h:
        for by in tc.BYS:
            side = m if by == "column" else n
            lines = rng.choice(side, size=37, replace=False)
            for n_top, ex in ((10, False), (10, True), (128, True), (1, False)):
                s = seen if ex else None
                assert_same(h.top_n(n_top, by=by, exclude=ex), tc.topn_oracle(W, H, n_top, by, None, s), f"k={k} {by} N={n_top} ex={ex}")
                assert_same(h.top_n(n_top, by=by, lines=lines, exclude=ex), tc.topn_oracle(W, H, n_top, by, lines, s), f"k={k} {by} N={n_top} lines")


@pytest.mark.parametrize("mode,prec", MODES, ids=MODE_IDS)
def test_exact_more_wanted_than_candidates_and_nan_scores(mode, prec):
    rng = np.random.default_rng(31)
    W, H = tc.integer_factors(9, 40, 3, rng)
    W[4, :] = np.nan  # row 4 scores NaN everywhere: never selected
    with open_handle(prec, W, H) as h:
        for by, n_top in (("column", 64), ("column", 9), ("row", 64), ("row", 40), ("row", 3)):
            assert_same(h.top_n(n_top, by=by), tc.topn_oracle(W, H, n_top, by), f"{by} N={n_top}")
        idx, score = h.top_n(5, by="column", lines=np.zeros(0, dtype=np.int64))
        assert idx.shape == (0, 5) and score.shape == (0, 5)
        idx, score = h.top_n(4, by="row", lines=[4])
        assert (idx == -1).all() and np.isnan(score).all()


def test_exact_many_lines_span_several_rounds():
    """More lines than one round of the library (16384): the rounds' results are laid out one after another."""
    rng = np.random.default_rng(32)
    W, H = tc.integer_factors(40000, 90, 5, rng)
    with open_handle(_lib.PREC_F64, W, H) as h:
        assert_same(h.top_n(7, by="row"), tc.topn_oracle(W, H, 7, "row"), "40000 rows")
        lines = rng.integers(0, 90, size=20000)  # (repeated lines are legal)
        assert_same(h.top_n(3, by="column", lines=lines), tc.topn_oracle(W, H, 3, "column", lines), "20000 listed columns")


# ---- random family -----------------------------------------------------------------------------------------------------------------------
def check_random(got, W, H, n_top, by, seen):
    idx, score = got
    S, T = W @ H, tc.tau(W, H)
    P = None if seen is None else sc.pattern_of(seen)
    if by == "row":
        S, T, P = S.T, T.T, (None if P is None else P.T)
    ncand, L = S.shape
    assert idx.shape == (L, n_top) and (idx >= 0).all() and (idx < ncand).all()
    ls = np.arange(L)[:, None]
    ref, t = S[idx, ls], T[idx, ls]
    dev = np.abs(score - ref) / t
    print(f"  by={by} seen={seen is not None}: max |score - numpy| / tau = {dev.max():.3f}")
    assert (dev <= 1.0).all()
    srt = np.sort(idx, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "an index is returned twice"
    if P is not None:
        assert not P[idx, ls].any(), "a stored entry was returned"
    assert ((score[:, :-1] > score[:, 1:]) | ((score[:, :-1] == score[:, 1:]) & (idx[:, :-1] < idx[:, 1:]))).all(), "order"
    # nothing left out scores above the N-th returned score by more than tau
    left = S.copy()
    left[idx, ls] = -np.inf
    if P is not None:
        left[P] = -np.inf
    assert (left <= score[:, -1][None, :] + T).all()
    exempt = tc.exempt_lines(W, H, n_top, by, seen)
    assert exempt.mean() == 0.0  # (these cases: test_topn_host.py; other random cases may exempt at most 1 %)
    want, _ = tc.topn_oracle(W, H, n_top, by, None, seen)
    assert (idx[~exempt] == want[~exempt]).all()


@pytest.mark.parametrize("mode,prec", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("i", range(len(tc.RANDOM_SHAPES)))
def test_random(mode, prec, i):
    c = tc.random_case(i)
    W, H, N = c["W"], c["H"], c["N"]
    with open_handle(prec, W, H, c["seen"]) as h:
        for by in tc.BYS:
            check_random(h.top_n(N, by=by), W, H, N, by, None)
            check_random(h.top_n(N, by=by, exclude=True), W, H, N, by, c["seen"])


# ---- geometry invariance -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,prec", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("by", tc.BYS)
def test_result_does_not_depend_on_lines_asked_or_slicing(mode, prec, by):
    c = tc.random_case(0 if by == "column" else 2)  # (3000 candidates either way: enough for several slices)
    W, H, N = c["W"], c["H"], c["N"]
    side = c["m"] if by == "column" else c["n"]
    runs, slices = [], []
    try:
        for cus in (0, 3, 64):
            _lib.debug_set_cus(cus)
            with open_handle(prec, W, H, c["seen"]) as h:
                full = h.top_n(N, by=by, exclude=True)
                slices.append(h.get_info("topn_slices"))
                two = np.array([side - 2, 5])
                part = h.top_n(N, by=by, lines=two, exclude=True)
                slices.append(h.get_info("topn_slices"))
                assert np.array_equal(part[0], full[0][two]) and np.array_equal(part[1], full[1][two])
                runs.append(full)
    finally:
        _lib.debug_set_cus(0)
    print(f"  slices per launch (all lines, two lines) at the device's CUs, 3 and 64: {slices}")
    assert slices[2] != slices[4] or slices[3] != slices[5], "the two CU counts must slice differently"
    assert slices[1] > 1, "two lines on the whole device must be sliced"
    for r in runs[1:]:
        assert np.array_equal(r[0], runs[0][0]) and np.array_equal(r[1], runs[0][1])


# ---- predict_entries ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,prec", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("i", (1, 3))
def test_predict_entries_against_numpy_and_top_n(mode, prec, i):
    c = tc.random_case(i)
    W, H, N, n, m = c["W"], c["H"], c["N"], c["n"], c["m"]
    S, T = W @ H, tc.tau(W, H)
    rng = np.random.default_rng(400 + i)
    rows, cols = rng.integers(0, n, size=200001), rng.integers(0, m, size=200001)
    with open_handle(prec, W, H) as h:
        got = h.predict_entries(rows, cols)
        assert got.dtype == np.float64 and got.shape == rows.shape
        dev = np.abs(got - S[rows, cols]) / T[rows, cols]
        print(f"  max |predict - numpy| / tau = {dev.max():.3f}")
        assert (dev <= 1.0).all()
        assert h.predict_entries([], []).shape == (0,)
        idx, score = h.top_n(N, by="column")
        jj = np.repeat(np.arange(m), N)
        again = h.predict_entries(idx.ravel(), jj)
        assert (np.abs(again - score.ravel()) <= 2.0 * T[idx.ravel(), jj]).all()
        idx, score = h.top_n(N, by="row", lines=np.arange(0, n, 7))
        ii = np.repeat(np.arange(0, n, 7), N)
        again = h.predict_entries(ii, idx.ravel())
        assert (np.abs(again - score.ravel()) <= 2.0 * T[ii, idx.ravel()]).all()


@pytest.mark.parametrize("mode,prec", MODES, ids=MODE_IDS)
def test_predict_entries_after_a_run_reads_the_current_factors(mode, prec):
    c = sc.make_case(1, "missing", large=False)
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix_csc_missing(*c["S"])
        h.set_factors(c["k"], c["W0"], c["H0"])
        h.run(Z3, Z3, 5, -1.0, 0, False, 10, 1e-9, 1, 1)
        n, m = c["S"][3]
        rng = np.random.default_rng(9)
        rows, cols = rng.integers(0, n, size=5000), rng.integers(0, m, size=5000)
        got = h.predict_entries(rows, cols)  # (nothing re-uploaded)
        idx, score = h.top_n(5, by="column", exclude=True)
        W, H = h.get_factors()
    assert not np.array_equal(W, c["W0"])
    assert (np.abs(got - (W @ H)[rows, cols]) <= tc.tau(W, H)[rows, cols]).all()
    have = idx >= 0
    jj = np.broadcast_to(np.arange(m)[:, None], idx.shape)
    assert not sc.pattern_of(c["S"])[idx[have], jj[have]].any()
    assert (np.abs(score[have] - (W @ H)[idx[have], jj[have]]) <= tc.tau(W, H)[idx[have], jj[have]]).all()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def raises(code, match):
    class Ctx:
        def __enter__(self):
            self.cm = pytest.raises(_lib.NnlmError, match=match)
            self.info = self.cm.__enter__()
            return self

        def __exit__(self, *exc):
            out = self.cm.__exit__(*exc)
            if out:
                assert self.info.value.code == code, self.info.value
            return out
    return Ctx()


def call_top_n(h, by, n_top, lines, exclude):
    ln = None if lines is None else np.ascontiguousarray(lines, dtype=np.int32)
    L = ln.size if ln is not None else 1
    idx, score = np.zeros((max(L, h.n, h.m), 128), dtype=np.int32), np.zeros((max(L, h.n, h.m), 128))
    h._ck(h._lib.nnlm_top_n(h._h, by, n_top, _lib._ip(ln), L, exclude, _lib._ip(idx), _lib._dp(score)))


def test_refusals_by_code_and_message():
    rng = np.random.default_rng(5)
    n, m, k = 50, 30, 4
    W, H = rng.random((n, k)), rng.random((k, m))
    with open_handle(_lib.PREC_F64, W, H) as h:
        with raises(ERR_UNSUPPORTED, "n_top = 129"):
            call_top_n(h, 0, 129, None, 0)
        with raises(ERR_ARG, "n_top = 0"):
            call_top_n(h, 0, 0, None, 0)
        with raises(ERR_ARG, "by = 2"):
            call_top_n(h, 2, 5, None, 0)
        with raises(ERR_ARG, "exclude = 3"):
            call_top_n(h, 0, 5, None, 3)
        with raises(ERR_ARG, r"lines\[1\] = 30 is out of range"):
            call_top_n(h, 0, 5, [0, 30], 0)
        with raises(ERR_ARG, r"lines\[0\] = -1 is out of range"):
            call_top_n(h, 1, 5, [-1], 0)
        call_top_n(h, 1, 5, [49], 0)
        with raises(ERR_ARG, r"rows\[0\] = 50 is out of range"):
            h.predict_entries([50], [0])
        with raises(ERR_ARG, r"cols\[1\] = -2 is out of range"):
            h.predict_entries([0, 0], [0, -2])
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
        h.set_matrix(rng.random((n, m)))
        with raises(ERR_ARG, "no factors set"):
            h.top_n(5)
        with raises(ERR_ARG, "no factors set"):
            h.predict_entries([0], [0])
        h.set_factors(k, W, H)
        idx, score = h.top_n(5)  # (a dense matrix on the handle serves when nothing is excluded)
        want = tc.topn_oracle(W, H, 5)
        assert np.array_equal(idx, want[0]) and (np.abs(score - want[1]) <= tc.tau(W, H).max()).all()
        with raises(ERR_UNSUPPORTED, "exclude = 1 needs a sparse matrix"):
            h.top_n(5, exclude=True)
        h.set_factors_batch([2, 3])
        with raises(ERR_UNSUPPORTED, "batch"):
            h.top_n(5)
        with raises(ERR_UNSUPPORTED, "batch"):
            h.predict_entries([0], [0])
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
        h.set_matrix(rng.random((n, m)))
        h.comm_init(None, 0, 2)  # (a virtual rank)
        h.set_factors(k, W, H)
        with raises(ERR_UNSUPPORTED, "communicator"):
            h.top_n(5)
        with raises(ERR_UNSUPPORTED, "communicator"):
            h.predict_entries([0], [0])


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODE_IDS)
def test_end_to_end_ratings(mode, monkeypatch):
    monkeypatch.setenv("NNLM_PRECISION", mode)
    rng = np.random.default_rng(77)
    n, m, k, N = 400, 150, 4, 10
    V = (rng.random((n, k)) + 0.1) @ (rng.random((k, m)) + 0.1)
    stored = rng.random((n, m)) < 0.4
    left = np.flatnonzero(~stored.T.ravel())[::7]  # some of the entries left out, column-major flat
    S = sc.Csc(sc.csc_from_pattern(stored, V))
    fit = api.nnmf(S, k, absent="missing", max_iter=30, rel_tol=-1, verbose=0, rng=np.random.default_rng(1))
    W, H = np.asarray(fit["W"]), np.asarray(fit["H"])
    for by in tc.BYS:
        idx, score = api.top_n(fit, N, by=by, seen=S)
        P = stored if by == "column" else stored.T
        ls = np.broadcast_to(np.arange(idx.shape[0])[:, None], idx.shape)
        have = idx >= 0
        assert have.any() and not P[idx[have], ls[have]].any()
        want, _ = tc.topn_oracle(W, H, N, by, None, (S.indptr, S.indices, S.data, S.shape))
        ex = tc.exempt_lines(W, H, N, by, (S.indptr, S.indices, S.data, S.shape))
        assert ex.mean() <= 0.01 and (idx[~ex] == want[~ex]).all()
    rows, cols = left % n, left // n
    got = api.predict_entries(fit, rows, cols)
    assert (np.abs(got - (W @ H)[rows, cols]) <= tc.tau(W, H)[rows, cols]).all()
    idx2, _ = api.top_n(fit, 3, by="column", lines=[0, m - 1])
    assert np.array_equal(idx2, tc.topn_oracle(W, H, 3, "column", [0, m - 1])[0])
