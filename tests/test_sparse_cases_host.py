"""Conditions on the generators of tests/sparse_cases.py that keep tests/test_gpu_fuzz_sparse.py from hiding failures, checked with the
generators and the fp64 oracle alone (no GPU): few cases may be skipped as degenerate or compared with the loosened sweep-count
tolerance, the stopping rule must actually fire (and fire on trace strides above 1), every work-split boundary the `boundary` family is
built for must occur -- computed from the Python restatements of the kernels' work split, which the GPU file pins to the library -- and
every K-padding form and pattern family must occur among the default seeds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_cases as sc  # noqa: E402
from oracle import ref  # noqa: E402

SEED_COUNTS = [16, 150]  # the default of NNLM_FUZZ_SEEDS and the deep run


@pytest.mark.parametrize("semantics", sc.SEMANTICS)
@pytest.mark.parametrize("seeds", SEED_COUNTS)
def test_few_cases_are_degenerate_or_loosened(seeds, semantics):
    cases = [sc.make_case(seed, semantics) for seed in range(seeds)]
    deg = [c["seed"] for c in cases if sc.degenerate(c, ref)]
    loose = [c["seed"] for c in cases if sc.rank_deficient(c)]
    assert len(deg) <= seeds / 8, deg
    assert len(loose) <= seeds / 4, loose
    if semantics == "zero":
        assert not loose


@pytest.mark.parametrize("semantics", sc.SEMANTICS)
@pytest.mark.parametrize("seeds", SEED_COUNTS)
def test_the_stopping_rule_fires(seeds, semantics):
    """At least half of the non-degenerate stopping-rule cases stop by the rule before max_iter, at least a third of those with a trace
    stride above 1 (the speculative W half-step alternates with the stride)."""
    ran = ruled = strided = 0
    for seed in range(max(1, seeds // 2)):
        c = sc.make_stop_case(seed, semantics)
        if sc.degenerate(c, ref):
            continue
        o = ref.c_nnmf(sc.densify(c["S"], semantics), *sc.nnmf_args(c))
        ran += 1
        if o["n_iteration"] < c["max_iter"]:
            ruled += 1
            strided += c["trace"] > 1
    assert ran >= seeds // 2 - seeds // 16 and 2 * ruled >= ran and 3 * strided >= ruled, (ran, ruled, strided)


@pytest.mark.parametrize("semantics", sc.SEMANTICS)
def test_every_boundary_event_occurs_in_both_orientations(semantics):
    seen = {0: set(), 1: set()}  # by the half-step that reads the orientation: 0 = W over the CSR, 1 = H over the CSC
    lanes = {0: set(), 1: set()}
    for c in sc.boundary_cases(semantics):
        assert c["S"][1].size < 65536  # (below it the worker counts do not depend on the device's CU count)
        for which, ptr in ((1, c["S"][0]), (0, sc.transpose_csc(c["S"])[0])):
            ev = sc.boundary_events(ptr, c["k"], alloc_limit=c["alloc_limit"])
            seen[which] |= {e for e, cols in ev.items() if cols}
            lanes[which] |= {(e, sc.sp_lanes(sc.kp_of(c["k"]))) for e in sc.SPMM_EVENTS[:5] if ev[e]}
    for which in (0, 1):
        assert seen[which] == set(sc.SPMM_EVENTS + sc.GRAM_EVENTS), (which, set(sc.SPMM_EVENTS + sc.GRAM_EVENTS) - seen[which])
        assert lanes[which] == {(e, lw) for e in sc.SPMM_EVENTS[:5] for lw in (16, 32, 64)}, which
    used = {cnt for _, s, cols, _, _ in sc.boundary_specs() for cnt in (s,) + tuple(cols)}
    assert set(sc.COUNTS) <= used, set(sc.COUNTS) - used


def test_boundary_cases_are_what_their_specs_say():
    for (name, s, cols, k, slots), c in zip(sc.boundary_specs(), sc.boundary_cases("missing")[::2]):
        assert c["name"] == name and list(np.diff(c["S"][0])) == [s] + list(cols)
        assert np.array_equal(np.diff(sc.transpose_csc(sc.transpose_csc(c["S"]))[0]), np.diff(c["S"][0]))
        A = sc.densify(c["S"], "missing")
        assert np.array_equal(np.isfinite(A).sum(axis=0), [s] + list(cols))
        if slots:
            assert len(sc.gram_chunks(c["S"][0], sc.kp_of(k), c["alloc_limit"])) >= 2


def test_every_kp_form_family_and_corner_occurs_among_the_default_seeds():
    for semantics in sc.SEMANTICS:
        cases = [sc.make_case(seed, semantics) for seed in range(16)]
        assert {sc.kp_of(c["k"]) for c in cases} >= {16, 32, 48, 64}
        assert {c["family"] for c in cases} == set(sc.FAMILIES)
        assert {c["density"] for c in cases if c["family"] == "uniform"} == {0.05, 0.2, 0.5, 1.0}
        assert any(c["S"][3][0] == 1 for c in cases) and any(c["S"][3][1] == 1 for c in cases) and any(c["k"] == 1 for c in cases)
        assert any(c["S"][3][0] > 400 for c in cases) and any(c["Wm"] is not None for c in cases)
        assert {c["method"] for c in cases} == {1, 2} and {c["trace"] for c in cases} == {1, 2, 3}
        assert all(c["S"][1].size > 0 for c in cases)
        if semantics == "zero":
            assert any(c["k"] > 64 for c in cases)
        else:
            assert all(c["k"] <= 64 for c in cases)
    c = sc.make_cap_case("zero")
    assert c["S"][1].size > 16 * 64 * 256 and sc.sp_workers(c["S"][1].size, sc.kp_of(c["k"])) == 16 * sc.DEFAULT_CUS


def test_cases_are_deterministic_and_densify_keeps_the_pattern():
    for semantics in sc.SEMANTICS:
        a, b = sc.make_case(6, semantics), sc.make_case(6, semantics)
        assert all(np.array_equal(x, y) for x, y in zip(a["S"][:3], b["S"][:3])) and np.array_equal(a["W0"], b["W0"])
        A = sc.densify(a["S"], semantics)
        P = sc.pattern_of(a["S"])
        assert np.array_equal(A[P], sc.densify(a["S"], "zero")[P]) and (np.isnan(A[~P]).all() if semantics == "missing" else (A[~P] == 0).all())
        rows, cols = sc.line_counts(a["S"])
        assert np.array_equal(rows, P.sum(axis=1)) and np.array_equal(cols, P.sum(axis=0))
        assert (rows == 0).sum() >= 5 and (cols == 0).sum() >= 5  # (seed 6: empty_lines, runs included)


def test_restated_work_split_covers_every_non_zero_once():
    for nnz, k in ((0, 3), (1, 16), (63, 16), (64, 17), (65, 64), (4097, 20), (300000, 12), (2_000_000, 70)):
        nw = sc.sp_workers(nnz, sc.kp_of(k))
        chunk, ranges = sc.split_of(nnz, nw)
        assert nw % (64 // sc.sp_lanes(sc.kp_of(k))) == 0 and ranges[0][0] == 0 and ranges[-1][1] == nnz
        assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
        assert nw <= 16 * sc.DEFAULT_CUS * 4
    assert [sc.segments_of(v) for v in (0, 1, 2047, 2048, 2049, 4096, 4097)] == [0, 0, 0, 0, 2, 2, 3]
