"""Ranking evaluation of top-N lists against held-out entries on the MI355X: nnlm_top_n_eval, Handle.top_n_eval and
api.evaluate_top_n against eval_oracle (tests/topn_eval_cases.py), the definitions in plain numpy and Python working from index lists.
Run with `pytest -m gpu`.  The checks (check_*) are parts of one collected test, test_top_n_eval, at the end of the file.

Integers (n_evaluated, t, first, hits) compare exactly, floats at 1e-13 relative: the only differences allowed are the C library's log2
against Python's and the order in which the means are summed.  The lists the oracle reads are the ones Handle.top_n returns on the same
handle with the same arguments (consistency) or topn_cases.topn_oracle's on integer factors (numpy alone)."""
import os
import sys
import traceback

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import topn_eval_cases as ec  # noqa: E402
import topn_cases as tc  # noqa: E402
import sparse_cases as sc  # noqa: E402
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = [("f64", _lib.PREC_F64), ("f32", _lib.PREC_F32)]
MODE_IDS = [m[0] for m in MODES]
ERR_ARG, ERR_UNSUPPORTED = 1, 5
CASES = ec.consistency_cases()


@pytest.fixture(autouse=True)
def _default_precision(monkeypatch):
    monkeypatch.delenv("NNLM_PRECISION", raising=False)


def open_handle(prec, W, H, seen=None):
    """A handle with the factors and `seen` (a CSC tuple; None: the empty pattern) as its sparse matrix."""
    n, m = W.shape[0], H.shape[1]
    h = nnlm_amd.Handle(0, prec)
    if seen is None:
        seen = (np.zeros(m + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), (n, m))
    h.set_matrix_csc(*seen)
    h.set_factors(W.shape[1], W, H)
    return h


def close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    both_nan = np.isnan(got) & np.isnan(want)
    return bool(np.all(both_nan | (np.abs(got - want) <= ec.RTOL * np.abs(want))))


def worst(got, want):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(np.asarray(got) - np.asarray(want)) / np.abs(np.asarray(want))
    return float(np.nanmax(r)) if np.any(np.isfinite(r)) else 0.0


def assert_matches(out, want, what):
    """A per_line result of Handle.top_n_eval against eval_oracle's."""
    assert out["n_evaluated"] == want["n_evaluated"], what
    assert np.array_equal(out["n_heldout"], want["t"]) and np.array_equal(out["first_hit"], want["first"]), what
    assert out["hits"].dtype == np.int64 and np.array_equal(out["hits"], want["hits"]), what
    agg = np.stack([out[name] for name in ec.METRICS], axis=1)
    print(f"  {what}: evaluated {out['n_evaluated']}, worst relative difference dcg {worst(out['dcg'], want['dcg']):.1e} "
          f"apn {worst(out['apn'], want['apn']):.1e} means {worst(agg, want['agg']):.1e}")
    assert close(out["dcg"], want["dcg"]) and close(out["apn"], want["apn"]), what
    assert agg.shape == want["agg"].shape and close(agg, want["agg"]), (what, agg, want["agg"])


def evaluate(h, cutoffs, by, lines, exclude, ptr, idx, lists, what):
    """top_n_eval with records, checked against the oracle on `lists`; the call without records gives the same aggregates."""
    out = h.top_n_eval(cutoffs, by=by, lines=lines, exclude=exclude, held_ptr=ptr, held_idx=idx, per_line=True)
    assert_matches(out, ec.eval_oracle(lists, ec.held_sets(ptr, idx, lines), cutoffs), what)
    assert h.get_info("topn_eval_lines") == out["n_evaluated"]
    bare = h.top_n_eval(cutoffs, by=by, lines=lines, exclude=exclude, held_ptr=ptr, held_idx=idx)
    assert "hits" not in bare and all(np.array_equal(bare[k], out[k], equal_nan=True) for k in ec.METRICS)
    return out


# ---- (a) consistency with top_n, (b) against numpy alone -----------------------------------------------------------------------------------
def check_equals_the_oracle_on_the_lists_top_n_returns(mode, prec, ci):
    name, W, H, seen, P = CASES[ci]
    n, m = P.shape
    rng = np.random.default_rng(900 + ci)
    cutoffs = (1, 5, 10, 20)
    with open_handle(prec, W, H, seen) as h:
        for by in tc.BYS:
            side = m if by == "column" else n
            some = rng.choice(side, size=23, replace=False)
            for exclude in (False, True):
                held = ec.random_held(n, m, rng, avoid=P if exclude else None)
                ptr, idx = ec.oriented(held, by)
                for lines in (None, some):
                    lists, _ = h.top_n(20, by=by, lines=lines, exclude=exclude)
                    out = evaluate(h, cutoffs, by, lines, exclude, ptr, idx, lists, f"{name} {by} exclude={exclude} lines={lines is not None}")
                    assert out["n_evaluated"] > 0 and out["hits"].max() > 0
                    assert lines is not None or out["n_evaluated"] < lists.shape[0]  # (lines without held-out entries are among them)
                    if name.startswith("integer") and exclude:  # numpy alone: exact scores, the oracle's own lists
                        assert_matches(out, ec.eval_oracle(tc.topn_oracle(W, H, 20, by, lines, seen)[0], ec.held_sets(ptr, idx, lines), cutoffs),
                                       f"{name} {by} against topn_oracle")


def check_integer_factors_put_hits_inside_runs_of_tied_scores():
    """The integer cases are there for ties: some hit has a neighbour in its list with the same score."""
    name, W, H, seen, P = CASES[2]
    held = ec.random_held(*P.shape, np.random.default_rng(1), density=0.3)
    ptr, idx = ec.oriented(held, "column")
    with open_handle(_lib.PREC_F64, W, H, seen) as h:
        lists, scores = h.top_n(20, by="column")
        evaluate(h, (20,), "column", None, False, ptr, idx, lists, name + " ties")
    tied = 0
    for l, T in enumerate(ec.held_sets(ptr, idx, None)):
        for p in np.flatnonzero(np.isin(lists[l], T)):
            tied += int((p > 0 and scores[l, p - 1] == scores[l, p]) or (p < 19 and scores[l, p + 1] == scores[l, p]))
    assert tied > 20


# ---- (c) list and cutoff edges -----------------------------------------------------------------------------------------------------------
CUTOFF_SETS = ((1,), (64,), (65,), (128,), (1, 5, 10, 64, 65, 127, 128), (1, 2, 3, 63, 64, 65, 66, 128))
HIT_POSITIONS = ((0,), (127,), (63,), (64,), (63, 64), (70,), (0, 1, 2, 126, 127), tuple(range(128)), (5, 64, 100))


def check_cutoff_sets_with_hits_at_chosen_positions(cutoffs):
    """Column l holds out exactly the rows at positions HIT_POSITIONS[l] of its best-128 list: position 0, the last one, both sides of the
    two ballot words (63 / 64), every position at once."""
    rng = np.random.default_rng(41)
    n, m, k = 140, 12, 4
    W, H = rng.random((n, k)), rng.random((k, m))
    with open_handle(_lib.PREC_F64, W, H) as h:
        full, _ = h.top_n(128, by="column")
        held = np.zeros((n, m), dtype=bool)
        for l, pos in enumerate(HIT_POSITIONS):
            held[full[l, list(pos)], l] = True
        ptr, idx = ec.oriented(held, "column")
        lists, _ = h.top_n(cutoffs[-1], by="column")
        assert np.array_equal(lists, full[:, :cutoffs[-1]])
        out = evaluate(h, cutoffs, "column", None, False, ptr, idx, lists, f"cutoffs {cutoffs}")
        for l, pos in enumerate(HIT_POSITIONS):  # (stated without the oracle)
            inside = [p for p in pos if p < cutoffs[-1]]
            assert out["first_hit"][l] == (inside[0] if inside else -1) and out["n_heldout"][l] == len(pos)
            assert out["hits"][l].tolist() == [sum(p < c for p in pos) for c in cutoffs]
        assert out["n_evaluated"] == len(HIT_POSITIONS) and (out["n_heldout"][len(HIT_POSITIONS):] == 0).all()
        # the first hit of column 5 sits at position 70: RR is 0 at every cutoff up to 70 and 1 / 71 beyond
        one = h.top_n_eval(cutoffs, by="column", lines=[5], held_ptr=ptr, held_idx=idx)
        assert one["n_evaluated"] == 1
        for c, rr, hr in zip(cutoffs, one["mrr"], one["hit_rate"]):
            assert (rr == 0.0 and hr == 0.0) if c <= 70 else (close(rr, 1.0 / 71.0) and hr == 1.0)


def check_lines_with_fewer_candidates_than_n_top_are_padded(exclude):
    rng = np.random.default_rng(42)
    n, m = 9, 40
    W, H = tc.integer_factors(n, m, 3, rng)
    P = rng.random((n, m)) < 0.3
    P[:, 3] = True  # a column that stores everything: its list is padding alone
    seen = sc.csc_from_pattern(P, np.ones((n, m)))
    held = (rng.random((n, m)) < 0.3) & ~P
    with open_handle(_lib.PREC_F64, W, H, seen) as h:
        for by, cutoffs in (("column", (4, 16)), ("row", (64,)), ("row", (3, 39, 40, 41))):
            ptr, idx = ec.oriented(held, by)
            lists, _ = h.top_n(cutoffs[-1], by=by, exclude=exclude)
            assert (lists == -1).any()
            out = evaluate(h, cutoffs, by, None, exclude, ptr, idx, lists, f"padding {by} {cutoffs} exclude={exclude}")
            if exclude:  # nothing stored is a candidate, so every held-out entry of a short column is found
                assert np.array_equal(out["hits"][:, -1], out["n_heldout"])


# ---- (d) held-out edges ------------------------------------------------------------------------------------------------------------------
def check_held_out_counts_zero_one_sixty_five_and_beyond_n_top():
    name, W, H, seen, P = CASES[0]
    n, m = P.shape
    rng = np.random.default_rng(43)
    cutoffs = (10, 64, 128)
    c0, c1, c2, c3, c4 = cols = np.flatnonzero(P.sum(axis=0) <= 20)[:5]  # (columns that leave more than 128 + 86 rows to choose from)
    with open_handle(_lib.PREC_F64, W, H, seen) as h:
        lists, _ = h.top_n(128, by="column", exclude=True)
        assert (lists[cols] >= 0).all()
        held = ec.random_held(n, m, rng, avoid=P)                       # ordinary columns, and among them:
        held[:, cols] = False                                           # c0: t = 0
        free = {j: np.setdiff1d(np.flatnonzero(~P[:, j]), lists[j]) for j in (c2, c3)}
        held[lists[c1, 7], c1] = True                                   # t = 1, found at position 7
        held[lists[c2, 100:128], c2] = True                             # t = 65: 28 of them listed late
        held[rng.choice(free[c2], size=37, replace=False), c2] = True
        held[lists[c3, :128:2], c3] = True                              # t = 150 > n_top: 64 listed
        held[rng.choice(free[c3], size=86, replace=False), c3] = True
        held[lists[c4, :5], c4] = True                                  # t = 5, all found first: NDCG = AP = 1 from cutoff 10 on
        ptr, idx = ec.oriented(held, "column")
        assert np.diff(ptr)[cols].tolist() == [0, 1, 65, 150, 5]
        out = evaluate(h, cutoffs, "column", None, True, ptr, idx, lists, "held-out counts")
        assert out["n_heldout"][c0] == 0 and out["first_hit"][c0] == -1 and not out["hits"][c0].any() and not out["dcg"][c0].any()
        assert out["first_hit"][c1] == 7 and out["hits"][c1].tolist() == [1, 1, 1]
        assert out["hits"][c2].tolist() == [0, 0, 28] and out["hits"][c3].tolist() == [5, 32, 64]
        assert out["n_evaluated"] == int((np.diff(ptr) > 0).sum()) < m
        four = evaluate(h, cutoffs, "column", [c4], True, ptr, idx, lists[[c4]], "t = 5, a perfect list")
        assert four["precision"].tolist() == [0.5, 5 / 64, 5 / 128] and four["recall"].tolist() == [1.0] * 3
        assert close(four["ndcg"], [1.0] * 3) and close(four["map"], [1.0] * 3) and four["mrr"].tolist() == [1.0] * 3
        # the ideal DCG of c3 has min(c, t) = c terms
        three = h.top_n_eval(cutoffs, by="column", lines=[c3], exclude=True, held_ptr=ptr, held_idx=idx, per_line=True)
        ideal = [sum(ec.discount(p) for p in range(c)) for c in cutoffs]
        assert close(three["ndcg"], three["dcg"][0] / np.array(ideal))


def check_no_line_evaluated_gives_nan():
    name, W, H, seen, P = CASES[3]
    n, m = P.shape
    with open_handle(_lib.PREC_F64, W, H, seen) as h:
        for by in tc.BYS:
            side = m if by == "column" else n
            empty = (np.zeros(side + 1, dtype=np.int64), np.zeros(0, dtype=np.int32))
            out = h.top_n_eval((1, 10), by=by, exclude=True, held_ptr=empty[0], held_idx=empty[1], per_line=True)
            assert out["n_evaluated"] == 0 and all(np.isnan(out[k]).all() and out[k].shape == (2,) for k in ec.METRICS)
            assert not out["n_heldout"].any() and (out["first_hit"] == -1).all() and not out["hits"].any() and h.get_info("topn_eval_lines") == 0
            held = np.zeros((n, m), dtype=bool)
            held[:3, :3] = ~P[:3, :3]  # held-out entries only in lines that are not listed
            ptr, idx = ec.oriented(held, by)
            out = h.top_n_eval((1, 10), by=by, lines=[5, 6, 40], exclude=True, held_ptr=ptr, held_idx=idx, per_line=True)
            assert ptr[-1] > 0 and out["n_evaluated"] == 0 and np.isnan(out["ndcg"]).all() and not out["n_heldout"].any()
            out = h.top_n_eval((3,), by=by, lines=np.zeros(0, dtype=np.int32), held_ptr=ptr, held_idx=idx, per_line=True)
            assert out["n_evaluated"] == 0 and out["hits"].shape == (0, 1) and np.isnan(out["map"]).all()


# ---- (e) rounds, (f) reproducibility -----------------------------------------------------------------------------------------------------
def check_more_lines_than_one_round():
    """16400 columns are two rounds of the library (16384 lines each): the records of the second round land behind the first's, its sums
    are added to the first's, and a line's record is the same whichever call it came from."""
    rng = np.random.default_rng(44)
    n, m = 40, 16400
    W, H = rng.random((n, 2)), rng.random((2, m))
    held = ec.random_held(n, m, rng, density=0.1)
    held[:, [0, 16383, 16384, m - 1]] = False
    held[[3, 20], 0] = held[[5], 16383] = held[[0, 1, 39], 16384] = held[[7, 8], m - 1] = True
    ptr, idx = ec.oriented(held, "column")
    cutoffs = (1, 10)
    with open_handle(_lib.PREC_F64, W, H) as h:
        lists, _ = h.top_n(10, by="column")
        out = evaluate(h, cutoffs, "column", None, False, ptr, idx, lists, "16400 columns")
        assert (out["n_heldout"][:16384] > 0).any() and (out["n_heldout"][16384:] > 0).any()
        some = np.array([0, 16383, 16384, m - 1])
        part = evaluate(h, cutoffs, "column", some, False, ptr, idx, lists[some], "four scattered columns")
        assert part["n_evaluated"] == 4
        for key in ("n_heldout", "first_hit", "hits", "dcg", "apn"):
            assert np.array_equal(part[key], out[key][some]), key
        again = h.top_n_eval(cutoffs, by="column", held_ptr=ptr, held_idx=idx, per_line=True)
        assert all(np.array_equal(again[k], out[k]) for k in out)


def check_two_calls_give_identical_bits_and_records_do_not_depend_on_the_lines_asked(by):
    name, W, H, seen, P = CASES[0]
    n, m = P.shape
    rng = np.random.default_rng(45)
    held = ec.random_held(n, m, rng, avoid=P)
    ptr, idx = ec.oriented(held, by)
    cutoffs = (3, 64, 100)
    side = m if by == "column" else n
    with open_handle(_lib.PREC_F32, W, H, seen) as h:
        a = h.top_n_eval(cutoffs, by=by, exclude=True, held_ptr=ptr, held_idx=idx, per_line=True)
        b = h.top_n_eval(cutoffs, by=by, exclude=True, held_ptr=ptr, held_idx=idx, per_line=True)
        assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
        some = rng.permutation(side)[:61]  # (any order, not a multiple of the four lines of a workgroup)
        c = h.top_n_eval(cutoffs, by=by, lines=some, exclude=True, held_ptr=ptr, held_idx=idx, per_line=True)
        for key in ("n_heldout", "first_hit", "hits", "dcg", "apn"):
            assert np.asarray(c[key]).tobytes() == np.ascontiguousarray(a[key][some]).tobytes(), key


# ---- (g) refusals ------------------------------------------------------------------------------------------------------------------------
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


def check_refusals_by_code_and_message():
    rng = np.random.default_rng(5)
    n, m, k = 50, 30, 4
    W, H = rng.random((n, k)), rng.random((k, m))
    P = np.zeros((n, m), dtype=bool)
    P[3, 2] = P[9, 2] = P[4, 7] = True
    seen = sc.csc_from_pattern(P, np.ones((n, m)))
    held = np.zeros((n, m), dtype=bool)
    held[[1, 3, 9], 2] = held[4, 7] = held[0, 0] = True  # (3, 2), (9, 2) and (4, 7) are stored
    cptr, cidx = ec.oriented(held, "column")
    rptr, ridx = ec.oriented(held, "row")
    with open_handle(_lib.PREC_F64, W, H, seen) as h:
        def good():
            out = h.top_n_eval((1, 5), by="column", held_ptr=cptr, held_idx=cidx)
            assert out["n_evaluated"] == 3 and np.isfinite(out["ndcg"]).all()

        def ev(cutoffs, by="column", lines=None, exclude=False, ptr=cptr, idx=cidx):
            return h.top_n_eval(cutoffs, by=by, lines=lines, exclude=exclude, held_ptr=ptr, held_idx=idx)
        good()
        for cutoffs, code, match in (((5, 5), ERR_ARG, r"cutoffs\[1\] = 5 does not ascend"), ((10, 3), ERR_ARG, r"cutoffs\[1\] = 3 does not ascend"),
                                     ((0, 4), ERR_ARG, r"cutoffs\[0\] = 0"), ((4, 129), ERR_UNSUPPORTED, r"cutoffs\[1\] = 129, at most 128"),
                                     (tuple(range(1, 10)), ERR_ARG, "n_cut = 9"), ((), ERR_ARG, "n_cut = 0")):
            with raises(code, match):
                ev(cutoffs)
            good()
        with raises(ERR_ARG, r"lines\[1\] = 30 is out of range \(m = 30\)"):
            ev((5,), lines=[0, 30])
        with raises(ERR_ARG, r"lines\[0\] = 50 is out of range \(n = 50\)"):
            ev((5,), by="row", lines=[50], ptr=rptr, idx=ridx)
        good()
        bad = cidx.copy()
        bad[cptr[2] + 1] = 50
        with raises(ERR_ARG, r"held-out row index 50 out of range at entry 2 \(column 2\)"):
            ev((5,), idx=bad)
        good()
        bad = cidx.copy()
        bad[cptr[2]:cptr[2] + 2] = (3, 3)
        with raises(ERR_ARG, r"held-out row indices of column 2 are not strictly increasing \(entry 2\)"):
            ev((5,), idx=bad)
        bad = ridx.copy()
        bad[rptr[4]] = -1
        with raises(ERR_ARG, r"held-out column index -1 out of range at entry \d+ \(row 4\)"):
            ev((5,), by="row", ptr=rptr, idx=bad)
        bad = cptr.copy()
        bad[3] = 0
        with raises(ERR_ARG, "held_ptr decreases at column 2"):
            ev((5,), ptr=bad)
        good()
        # an overlap with the stored pattern: the first entry in (position in lines, index) order is named
        with raises(ERR_ARG, r"held-out entry \(row 3, column 2\) of lines\[2\] is stored in the resident matrix"):
            ev((5,), exclude=True)
        with raises(ERR_ARG, r"held-out entry \(row 4, column 7\) of lines\[0\] is stored in the resident matrix"):
            ev((5,), exclude=True, lines=[7, 2])
        with raises(ERR_ARG, r"held-out entry \(row 3, column 2\) of lines\[3\] is stored in the resident matrix"):
            ev((5,), by="row", exclude=True, ptr=rptr, idx=ridx)
        assert ev((5,), exclude=True, lines=[0, 1])["n_evaluated"] == 1  # (the overlap sits in lines that are not listed)
        assert ev((5,), exclude=False)["n_evaluated"] == 3               # (and without exclusion nothing is wrong with it)
        good()
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
        h.set_matrix(rng.random((n, m)))
        with raises(ERR_ARG, "no factors set"):
            h.top_n_eval((5,), held_ptr=cptr, held_idx=cidx)
        h.set_factors(k, W, H)
        with raises(ERR_UNSUPPORTED, "exclude = 1 needs a sparse matrix"):
            h.top_n_eval((5,), exclude=True, held_ptr=cptr, held_idx=cidx)
        out = h.top_n_eval((5,), held_ptr=cptr, held_idx=cidx)  # (a dense matrix on the handle serves when nothing is excluded)
        assert out["n_evaluated"] == 3
        h.set_factors_batch([2, 3])
        with raises(ERR_UNSUPPORTED, "batch"):
            h.top_n_eval((5,), held_ptr=cptr, held_idx=cidx)
        h.set_factors(k, W, H)
        assert h.top_n_eval((5,), held_ptr=cptr, held_idx=cidx)["n_evaluated"] == 3


# ---- (h) end to end ----------------------------------------------------------------------------------------------------------------------
def check_end_to_end_split_fit_evaluate(by):
    rng = np.random.default_rng(78)
    n, m, k = 400, 300, 4
    V = (rng.random((n, k)) ** 2 + 0.05) @ (rng.random((k, m)) ** 2 + 0.05)
    stored = rng.random((n, m)) < 0.1 + 0.5 * (V > np.quantile(V, 0.8))  # (what is rated is mostly what rates high: a planted signal)
    A = sc.Csc(sc.csc_from_pattern(stored, V))
    train, held = api.holdout_split(A, per_line=2, by=by, min_keep=5, rng=7)
    fit = api.nnmf(train, k, absent="missing", max_iter=30, rel_tol=-1, verbose=0, rng=np.random.default_rng(1))
    out = api.evaluate_top_n(fit, held, (1, 10), by=by, seen=train, per_line=True)
    lists, _ = api.top_n(fit, 10, by=by, seen=train)
    ptr, idx = ec.oriented(sc.pattern_of(tuple(held)), by)
    want = ec.eval_oracle(lists, ec.held_sets(ptr, idx, None), (1, 10))
    assert out["cutoffs"].tolist() == [1, 10] and out["n_evaluated"] == want["n_evaluated"] > 0
    assert np.array_equal(out["lines"], np.arange(lists.shape[0])) and np.array_equal(out["n_heldout"], want["t"])
    assert np.array_equal(out["first_hit"], want["first"]) and np.array_equal(out["hits"], want["hits"]) and close(out["dcg"], want["dcg"])
    with np.errstate(divide="ignore", invalid="ignore"):
        assert close(out["ap"], want["apn"] / np.minimum(np.array([1, 10])[None, :], want["t"][:, None]))
    agg = np.stack([out[name] for name in ec.METRICS], axis=1)
    assert close(agg, want["agg"])
    print(f"  by={by}: {out['n_evaluated']} lines, hit rate@1/10 {out['hit_rate']}, ndcg {out['ndcg']}, map {out['map']}, mrr {out['mrr']}")
    assert out["hit_rate"][1] > 0  # (a sanity check of a planted model, not a quality bar)
    short = api.evaluate_top_n(fit, held, 10, by=by, seen=train, lines=[0, 5, 7])
    assert short["cutoffs"].tolist() == [10] and "hits" not in short and short["n_evaluated"] == int((want["t"][[0, 5, 7]] > 0).sum())
    with pytest.raises(api.NnlmStop, match="heldout overlaps seen: .*is stored in the resident matrix"):
        api.evaluate_top_n(fit, A, 10, by=by, seen=train)


# ---- (i) nnlm_top_n itself did not move -----------------------------------------------------------------------------------------------------
GOLDEN = ec.golden_calls()


def check_top_n_is_bit_identical_to_the_lists_recorded_before_the_round_helper(gi):
    """tests/golden/topn_parent_lists.npz: idx and scores that topn_eval_cases.golden_run returned on the commit before nnlm_top_n's round
    loop became the helper it now shares with nnlm_top_n_eval."""
    rec = np.load(os.path.join(HERE, "golden", ec.GOLDEN_FILE))
    idx, score = ec.golden_run(GOLDEN[gi])
    want_i, want_s = rec[GOLDEN[gi][0] + "_idx"], rec[GOLDEN[gi][0] + "_score"]
    assert idx.dtype == want_i.dtype and np.array_equal(idx, want_i)
    assert score.dtype == want_s.dtype == np.float64 and score.tobytes() == want_s.tobytes()


# ---- the one collected test ---------------------------------------------------------------------------------------------------------------
def parts():
    """[(label, check, arguments)]: every check above at every argument it is meant for."""
    out = [(f"{CASES[ci][0]}-{mode}", check_equals_the_oracle_on_the_lists_top_n_returns, (mode, prec, ci))
           for ci in range(len(CASES)) for mode, prec in MODES]
    out.append(("ties", check_integer_factors_put_hits_inside_runs_of_tied_scores, ()))
    out += [("cutoffs " + "-".join(str(c) for c in cs), check_cutoff_sets_with_hits_at_chosen_positions, (cs,)) for cs in CUTOFF_SETS]
    out += [(f"padding exclude={e}", check_lines_with_fewer_candidates_than_n_top_are_padded, (e,)) for e in (False, True)]
    out.append(("held-out counts", check_held_out_counts_zero_one_sixty_five_and_beyond_n_top, ()))
    out.append(("nothing evaluated", check_no_line_evaluated_gives_nan, ()))
    out.append(("two rounds", check_more_lines_than_one_round, ()))
    out += [(f"reproducible {by}", check_two_calls_give_identical_bits_and_records_do_not_depend_on_the_lines_asked, (by,)) for by in tc.BYS]
    out.append(("refusals", check_refusals_by_code_and_message, ()))
    out += [(f"end to end {by}", check_end_to_end_split_fit_evaluate, (by,)) for by in tc.BYS]
    out += [("golden " + GOLDEN[gi][0], check_top_n_is_bit_identical_to_the_lists_recorded_before_the_round_helper, (gi,)) for gi in range(len(GOLDEN))]
    return out


def test_top_n_eval():
    """Every check of this file, as one test item (the GPU suite is some five thousand items long already; all of this takes about a
    second).  Each check runs whatever the ones before it did, and a failure is reported under its label with its traceback."""
    failed = []
    for label, check, args in parts():
        print(f"[{label}]")
        try:
            check(*args)
        except (Exception, pytest.fail.Exception):
            failed.append(f"---- {label} ----\n{traceback.format_exc()}")
    assert not failed, f"{len(failed)} of {len(parts())} checks failed:\n" + "\n".join(failed)
