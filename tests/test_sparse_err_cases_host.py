"""Conditions on the cases of tests/sparse_err_cases.py (no GPU): the groups reach all 18 forms of the sums over the stored entries; the
patterns have the empty lines; the planted entries sit on both sides of worker, wavefront and workgroup boundaries at every LW; every
quantity of the exact families is an integer within fp64 (fp32 where a kernel holds it in fp32) and the exact sum is the reference's;
and a plain fp64 numpy evaluation lies within the bars' reach of the long double reference."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import err_cases as ec  # noqa: E402
import sparse_cases as spc  # noqa: E402
import sparse_err_cases as se  # noqa: E402
import weighted_cases as wc  # noqa: E402


def test_groups_reach_every_form():
    hit = {}
    for (n, m), k in se.groups():
        for door in se.DOORS:
            if se.accepts(door, k):
                for mode in se.MODES:
                    hit.setdefault(se.form_of(mode, door, k), set()).add(k)
    assert set(hit) == se.all_forms() and len(hit) == 18
    for form, ks in hit.items():
        lo, hi = {16: (1, 16), 32: (17, 32), 64: (33, 64)}[form[2]]
        assert set(range(lo, hi + 1)) <= ks, form
    assert {k for k in hit[("sp_errors_kernel", "double", 64, False)] if k > 64} == set(se.RANKS_GENERIC)
    assert all(max(ks) <= 64 for form, ks in hit.items() if form != ("sp_errors_kernel", "double", 64, False) and form != ("sp_errors_kernel", "float", 64, False))
    assert se.form_of("f32", "weighted_zero", 17) == ("sp_errors_weighted_kernel", "float", 32)
    assert se.form_of("f64", "missing", 70) == ("sp_errors_kernel", "double", 64, True) and not se.accepts("missing", 70) and se.accepts("zero", 70)


def test_patterns_and_factors():
    for (n, m) in (se.MAIN,) + se.SHAPES_OTHER:
        for family in se.FAMILIES:
            c = se.make_case(family, n, m, 17)
            P, S = c["P"], c["S"]
            assert S[3] == (n, m) and np.array_equal(spc.pattern_of(S), P) and S[2].size == P.sum() >= 1
            if m >= 3:
                assert not P[:, 0].any() and not P[:, -1].any() and not c["H"][:, m // 2].any()
            if n >= 9:
                assert not P[7].any() and not c["W"][n // 2].any()
            if n * m > 1000:
                assert 0.25 < P.mean() < 0.33
            if family in se.EXACT:
                assert set(np.unique(c["W"])) <= {0, 1, 2, 3} and set(np.unique(c["H"])) <= {0, 1, 2, 3} and set(np.unique(c["w"])) <= set(se.EXACT_WEIGHTS)
                if n * m > 1000:
                    assert set(np.unique(c["w"])) == set(se.EXACT_WEIGHTS)


def test_planted_entries_sit_on_worker_boundaries():
    n, m = se.MAIN
    for k in (16, 17, 32, 33, 64, 70):
        c = se.make_case("planted", n, m, k)
        nnz, KP = c["S"][2].size, spc.kp_of(k)
        nw = spc.sp_workers(nnz, KP)
        _, ranges = spc.split_of(nnz, nw)
        firsts, lasts = {e0 for e0, e1 in ranges if e0 < e1}, {e1 - 1 for e0, e1 in ranges if e0 < e1}
        es = [e for e, _ in c["planted"]]
        assert len(es) == len(set(es)) >= 9 and [t for _, t in c["planted"]] == list(range(len(es)))
        assert all(e in firsts or e in lasts for e in es)
        ng = 64 // spc.sp_lanes(KP)
        last = max(w for w in range(nw) if ranges[w][0] < ranges[w][1])
        for w in {1, ng, 4 * ng, last}:   # both sides of a worker, a wavefront and a workgroup boundary, and of the last worker with entries
            assert ranges[w][0] in es and ranges[w][0] - 1 in es, (k, w)
        assert 0 in es and nnz - 1 in es
        wh = (c["W"] @ c["H"])[c["P"].T.nonzero()[::-1]]   # (CSC order)
        assert np.array_equal(np.flatnonzero(c["S"][2] != wh), np.sort(es))


def test_exact_families_are_integers_within_the_formats():
    worst64 = worst32 = 0.0
    for (n, m), k in [(se.MAIN, k) for k in (1, 17, 64, 70)] + [(s, 64) for s in se.SHAPES_OTHER]:
        for family in se.EXACT:
            c = se.make_case(family, n, m, k)
            for door in se.DOORS:
                if not se.accepts(door, k):
                    continue
                big, held32 = se.integer_bounds(c, door, family)
                worst64, worst32 = max(worst64, big), max(worst32, held32)
                assert big < 2.0 ** 53 and held32 < 2.0 ** 24, (family, n, m, k, door, big, held32)
                # the exact sum is the reference's sum: fp64 numpy on integers, the long double reference and the int agree
                A, C, obs = se.dense_of(c, door, family)
                want = se.exact_sum(c, door, family)
                r = se.ref_of(se.Case(family, n, m, k), door)
                assert float(r.s2) == float(want) and int(r.s2) == want, (family, door, want, r.s2)
                mse, _ = wc.errors(A, C, obs, c["W"].T, c["H"], r.N)
                assert mse == float(want) / r.N
                if se.ABSENT[door] == "missing" and family == "ones":
                    w = se.weights_of(c, door, family)
                    assert want == (int(w.sum()) if w is not None else c["S"][2].size)
                if se.ABSENT[door] == "missing" and family == "planted":
                    w = se.weights_of(c, door, family)
                    assert want == sum((int(w[e]) if w is not None else 1) * 4 ** t for e, t in c["planted"])
    print(f"largest fp64 integer {worst64:.3e} (2^53 = {2.0 ** 53:.3e}), largest fp32-held {worst32:.0f} (2^24 = {2 ** 24})")


def test_plain_fp64_evaluation_against_the_long_double_reference():
    """The rounding family: weighted_cases.errors (fp64 numpy) deviates from ld_errors by a few 1e-16 on the scale the bars are on -- the
    strict bar of 1e-10 (tests/test_gpu_error_block.py) is five orders above what fp64 sums of these sizes lose."""
    worst = 0.0
    for (n, m), k in [(se.MAIN, k) for k in (1, 17, 50, 64, 70)] + [(s, 17) for s in se.SHAPES_OTHER]:
        c = se.make_case("uniform", n, m, k)
        for door in se.DOORS:
            if not se.accepts(door, k):
                continue
            A, C, obs = se.dense_of(c, door, "uniform")
            r = se.ref_of(se.Case("uniform", n, m, k), door)
            mse, kl = wc.errors(A, C, obs, c["W"].T, c["H"], r.N)
            d = max(ec.dev(mse, r.s2, r.abs2, r.N), ec.dev(kl, r.kl, r.abskl, r.N))
            worst = max(worst, d)
            assert d < 1e-13, (n, m, k, door, d)
    print(f"fp64 numpy against the long double reference: {worst:.2e} at most")
