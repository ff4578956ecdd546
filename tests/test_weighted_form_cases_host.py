"""Conditions on the cases of tests/weighted_form_cases.py, from the restated dispatch and the fp64 oracle alone (no GPU): the cases reach
all 8 weighted Gram instantiations, all 8 fix-up forms (4 KP, with and without the shared Gram) and, under weighted_zero in the
fp32-operand mode, all 14 strict solver instantiations; the weights are what the module says; the wide case puts segments inside and on
worker boundaries and long columns first and last in a chunk; and the strict sweep counts of weighted_zero do not depend on whether the
Gram is one sqrt(c)-scaled sum (the reference) or G_full + sum (c - 1) y y^T (the library), outside wf.FORMULATION_DEPENDENT."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import na_solver_cases as nc  # noqa: E402
import sparse_cases as spc  # noqa: E402
import weighted_form_cases as wf  # noqa: E402
from helpers import relF  # noqa: E402
from oracle import nnlm_oracle, ref  # noqa: E402

FORM_BAR = 1e-11   # the two formulations against each other (fp64 both)


def launches():
    for k in wf.KS:
        for variant in nc.variants_of(k):
            for mode in wf.MODES:
                for door in wf.DOORS:
                    for method in (1, 2):
                        yield mode, door, method, k, variant


def test_dispatch_as_written():
    assert wf.solver_of("f32", "weighted_zero", 1, 17, True) == (("strict", 2, True, 20), 1, 20)
    assert wf.solver_of("f32", "weighted_zero", 1, 21, False) == (("strict", 2, False, 32), 1, 32)
    assert wf.solver_of("f32", "weighted_missing", 1, 17, True) == nc.solver_of("f32", 1, 17, True) == (("row", 2, True, 32), 0, 32)
    assert wf.solver_of("f32", "weighted_zero", 2, 33, False) == (("ls", 3), 2, 48)
    for mode in wf.MODES:
        for k in wf.KS:
            for masked in (False, True):
                assert wf.solver_of(mode, "weighted_zero", 1, k, masked) == nc.solver_of("f64", 1, k, masked)
                for method in (1, 2):
                    assert wf.solver_of(mode, "weighted_missing", method, k, masked) == nc.solver_of(mode, method, k, masked)
    assert wf.gram_of("f32", "weighted_zero", 33) == (("spw", "float", 3), 3, 3) and wf.gram_of("f64", "weighted_missing", 64) == (("spw", "double", 4), 3, 4)
    assert wf.info_of("f32", "weighted_zero", 1, 49, True) == (1, 52, 3, 4) and wf.info_of("f32", "weighted_missing", 1, 49, True) == (0, 50, 3, 4)
    assert wf.fixup_of("weighted_zero", 33) == ("fixup", 48, True) and wf.fixup_of("weighted_missing", 16) == ("fixup", 16, False)


def test_cases_reach_every_instantiation():
    grams, strict32, ends = {}, {}, {}
    for mode, door, method, k, variant in launches():
        masked, pen = nc.VARIANTS[variant]
        grams.setdefault(wf.gram_of(mode, door, k)[0], set()).add(k)
        if (mode, door, method) == ("f32", "weighted_zero", 1):
            s = wf.solver_of(mode, door, method, k, masked)[0]
            strict32.setdefault(s, set()).add(k)
            ends.setdefault(s, set()).add((k, pen))
    assert set(grams) == wf.all_gram_instantiations() and len(grams) == 8
    for (_, _, nt), ks in grams.items():
        assert ks == set(range(16 * nt - 15, 16 * nt + 1))
    assert set(strict32) == wf.all_strict_instantiations() and len(strict32) == 14
    for inst, ks in strict32.items():
        nkq, kr = inst[1], inst[3]
        lo = 16 * (nkq - 1) + 1 if (kr % 16 or nkq == 1) else 16 * (nkq - 1) + 5
        assert ks == set(range(lo, kr + 1)), inst
        for pen in (False, True):
            assert (lo, pen) in ends[inst] and (kr, pen) in ends[inst], inst
    # the wide case: every fix-up form, with and without the shared Gram, in the CSC and in the CSR orientation
    for ks in (wf.WIDE_KS, wf.WIDE_T_KS):
        assert {wf.fixup_of(door, k) for door in wf.DOORS for k in ks} == wf.all_fixup_instantiations()
    assert {wf.gram_of(mode, door, k)[0] for mode in wf.MODES for door in wf.DOORS for k in wf.WIDE_KS} == wf.all_gram_instantiations()


def test_weights_are_what_the_module_says():
    for k in (1, 17, 50, 64):
        for variant in nc.VARIANTS:
            c = nc.make_case(k, variant)
            S = nc.csc_of(c["A"])
            rows = c["rows_special"]
            zl = wf.line_entries(S, rows, wf.ZERO_LINE)
            assert zl.sum() >= 64
            for door in wf.DOORS:
                w = wf.weights_of(door, k, variant)
                assert w.shape == S[2].shape and np.array_equal(w, wf.weights_of(door, k, variant)) and (w >= 0).all()
                assert np.all(w[zl] == 0), (door, k, variant)
                o = w[~zl]
                if door == "weighted_zero":
                    assert 0.07 < (o == 1).mean() < 0.13 and 0.07 < ((o > 0) & (o < 1)).mean() < 0.13 and 0.03 < (o == 0).mean() < 0.07
                    assert o[(o > 0) & (o < 1)].min() >= 0.05 and o[(o > 0) & (o < 1)].max() <= 0.95 and o.max() <= 41 and (o > 1).mean() > 0.7
                else:
                    assert set(np.unique(o)) == set(wf.MISSING_WEIGHTS) and 0.2 < (o == 0).mean() < 0.3
                    # every line but the empty one and ZERO_LINE keeps at least 64 entries of positive weight: full rank at k = 64
                    P = wf.problem(door, k, variant)
                    pos_rows, pos_cols = (P["C"] > 0).sum(axis=1), (P["C"] > 0).sum(axis=0)
                    special, cross = (pos_rows, pos_cols) if rows else (pos_cols, pos_rows)
                    assert special[4] == 0 and special[wf.ZERO_LINE] == 0 and np.delete(special, [4, wf.ZERO_LINE]).min() >= 64, (k, variant)
                    assert cross.min() >= 64, (k, variant, cross.min())
    # a problem's dense parts and its CSR side say the same
    P = wf.problem("weighted_zero", 17, "masked")
    assert np.array_equal(P["A"] != 0, spc.pattern_of(P["S"])) and (P["C"][~spc.pattern_of(P["S"])] == 1).all() and P["obs"].all()
    Ct = np.ones(P["St"][3])
    Ct[P["St"][1], np.repeat(np.arange(P["St"][3][1]), np.diff(P["St"][0]))] = P["wt"]
    assert np.array_equal(Ct, P["Ct"])
    P = wf.problem("weighted_missing", 17, "plain")
    assert np.array_equal(P["obs"], np.isfinite(P["c"]["A"])) and (P["C"][~P["obs"]] == 0).all()


def test_wide_case_segments_and_chunks():
    assert sorted(wf.WIDE_ORDER) == sorted(wf.WIDE_LENS) and len(set(wf.WIDE_LENS)) == 30
    for door in wf.DOORS:
        for transposed in (False, True):
            P = wf.wide_problem(door, 16, transposed)
            ptr = P["St"][0] if transposed else P["S"][0]   # the orientation that holds the designed lines
            assert P["S"][3] == ((30, 4200) if transposed else (4200, 30))
            assert [int(v) for v in np.diff(ptr)] == list(wf.WIDE_ORDER)
            for k in wf.WIDE_T_KS:
                one = spc.boundary_events(ptr, k)
                assert one["column_of_2048"] and one["column_of_2049"] and one["segment_starts_on_boundary"], one
                many = spc.boundary_events(ptr, k, alloc_limit=wf.wide_alloc_limit(k))
                assert len(spc.gram_chunks(ptr, spc.kp_of(k), wf.wide_alloc_limit(k))) >= 3
                assert many["long_column_first_of_chunk"] and many["long_column_last_of_chunk"], many
            starts = wf.segment_starts(ptr)
            assert any(on for _, _, on in starts) and any(not on for _, _, on in starts), starts
            assert len(starts) == sum(max(spc.segments_of(L) - 1, 0) for L in wf.WIDE_ORDER) == 7
            w = P["wt"] if transposed else P["w"]
            assert (w >= 0).all() and ((w == 0).any() and (w == 1).any())
    # the reference sees what the library is given
    P = wf.wide_problem("weighted_missing", 16)
    assert np.array_equal(P["obs"].sum(axis=0), np.array(wf.WIDE_ORDER)) and P["c"]["reg"] == list(nc.REG)


def formulation_check(k, settings):
    """[(name, same)] over the variants of k, the given settings and both half-steps: sqrt(c)-scaled counts against the library's
    formulation, per column; the factors within FORM_BAR."""
    out, worst = [], 0.0
    for variant in nc.variants_of(k):
        P = wf.problem("weighted_zero", k, variant)
        for sname, setting in settings:
            cw, ch, lw, lh = [], [], None, None
            W, itw = wf.oracle_w(P, *setting, counts=cw)
            H, ith = wf.oracle_h(P, W, *setting, counts=ch)
            Wl, lw = wf.library_form_half_step(P, 0, None, *setting)
            Hl, lh = wf.library_form_half_step(P, 1, W, *setting)
            assert sum(cw) == itw and sum(ch) == ith
            worst = max(worst, relF(Wl, W), relF(Hl, H))
            assert relF(Wl, W) < FORM_BAR and relF(Hl, H) < FORM_BAR, (k, variant, sname, relF(Wl, W), relF(Hl, H))
            for side, a, b in (("w", cw, lw), ("h", ch, lh)):
                free = wf.rounding_decided_columns("weighted_zero", variant, side)
                differ = [j for j in range(len(a)) if a[j] != b[j] and j not in free]   # (free: the all-zero lines without an L1 penalty)
                out.append((wf.case_name("weighted_zero", k, variant, sname, side), not differ, a))
    return out, worst


@pytest.mark.parametrize("k", wf.KS)
def test_zero_door_counts_do_not_depend_on_the_formulation(k):
    """Every strict SCD count test_gpu_weighted_forms.py asserts under weighted_zero: equal per column in both formulations outside
    wf.FORMULATION_DEPENDENT -- but for wf.rounding_decided_columns(), the two all-zero lines where no L1 penalty clamps them,
    which the GPU test takes out of the count.  At the rank ends also (300, 1e-5), where columns of one wavefront -- four consecutive
    columns -- stop at different sweeps."""
    settings = (("tight", wf.TIGHT), ("loose", wf.LOOSE)) + ((("mid", wf.MID),) if k in wf.RANK_ENDS else ())
    res, worst = formulation_check(k, settings)
    mixed = {}
    for name, same, counts in res:
        assert same == (name not in wf.FORMULATION_DEPENDENT), name
        if "-mid-" in name:
            cnt = np.array(counts)
            waves = cnt[:cnt.size // 4 * 4].reshape(-1, 4)
            mixed[name] = int((waves.max(axis=1) != waves.min(axis=1)).sum())
            if k <= 17:
                assert cnt.max() < wf.MID[0], (name, cnt.max())
    if mixed:   # (k = 1: one coordinate is solved in two sweeps; only the masked variants' fully masked columns differ there)
        for side in "wh":
            assert max(v for name, v in mixed.items() if name.endswith(side)) >= 1, (k, mixed)
        print(f"k={k}: wavefronts with columns stopping at different sweeps at (300, 1e-5): {mixed}")
    print(f"k={k}: the two formulations differ by {worst:.2e} at most (bar {FORM_BAR:g})")


def test_formulation_dependent_cases_are_few():
    names = {wf.case_name("weighted_zero", k, v, s, side) for k in wf.KS for v in nc.variants_of(k) for s in ("tight", "loose", "mid") for side in "wh"}
    assert wf.FORMULATION_DEPENDENT <= names and len(wf.FORMULATION_DEPENDENT) <= wf.MAX_FORMULATION_DEPENDENT


@pytest.mark.parametrize("k", [1, 5, 17])
def test_c_solver_is_the_python_solver(k):
    """ref.scd_ls_update (C) is what library_form_half_step uses for speed: the same counts and bits as nnlm_oracle.scd_ls_update."""
    P = wf.problem("weighted_zero", k, "masked")
    for setting in (wf.TIGHT, wf.LOOSE):
        Wc, cc = wf.library_form_half_step(P, 0, None, *setting)
        Wp, cp = wf.library_form_half_step(P, 0, None, *setting, solver=nnlm_oracle.scd_ls_update)
        assert cc == cp and np.array_equal(Wc, Wp)


def test_missing_door_unit_weights_is_the_missing_reference():
    """Weights all 1, absent = missing: the sqrt(c)-scaled problem is nc's oracle problem."""
    c = nc.make_case(17, "masked")
    S = nc.csc_of(c["A"])
    P = wf._problem("weighted_missing", c, S, np.ones(S[2].size))
    W, it = wf.oracle_w(P, *wf.TIGHT)
    W2, it2 = nc.oracle_w(ref, c, *wf.TIGHT)
    assert np.array_equal(W, W2) and it == it2
