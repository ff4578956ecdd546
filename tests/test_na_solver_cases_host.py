"""Conditions on the cases of tests/na_solver_cases.py, from the restated dispatch and the fp64 oracle alone (no GPU): the cases reach every
one of the 47 instantiations of the per-column solvers and Gram kernels of the missing-value half-step; the oracle's strict sweep counts
do not ride on the order of the contraction where tests/test_gpu_na_forms.py compares them exactly; at the loose setting the four
columns of a colsolve_row_kernel wavefront stop at different sweeps at every rank; rounding the inputs to fp32 does not move the sweep
at which a column stops; every ordinary line observes at least 64 entries and the row-list case has every listed length on both sides
of one half."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import na_solver_cases as nc  # noqa: E402
from helpers import relF  # noqa: E402
from oracle import ref  # noqa: E402

ORDER_BAR = 1e-11   # the oracle against itself under another order of the contraction (measured: 3.2e-13 at most)


def launches():
    """(mode, door, method, k, variant) of every half-step launch test_gpu_na_forms.py's main test makes."""
    for k in nc.KS:
        for variant in nc.variants_of(k):
            for mode in nc.MODES:
                for door in nc.DOORS:
                    yield mode, door, 1, k, variant
                    yield mode, door, 2, k, variant


def test_dispatch_as_written():
    """The rules of nnlm_tu_colsolve_row, launch_colsolve_strict_m and launch_na_gram at the ranks where they switch."""
    for k, cls in ((1, (1, 16)), (16, (1, 16)), (17, (2, 32)), (32, (2, 32)), (33, (3, 48)), (47, (3, 48)), (48, (3, 48)), (49, (4, 50)), (50, (4, 50)),
                   (51, (4, 64)), (52, (4, 64)), (64, (4, 64))):
        assert nc.row_class(k) == cls, k
    short = {k: nc.solver_of("f64", 1, k, False)[2] for k in nc.KS}
    assert {k for k in nc.KS if short[k] % 16} == set(range(17, 21)) | set(range(33, 37)) | set(range(49, 53))
    assert short[20] == 20 and short[21] == 32 and short[36] == 36 and short[37] == 48 and short[52] == 52 and short[53] == 64 and short[16] == 16
    tails = {k for k in nc.KS if nc.gram_of("f64", "dense", k)[1] == nc.GRAM_CODE["lds_tail"]}
    assert tails == {17, 18, 33, 34, 49, 50}
    assert nc.gram_of("f64", "dense", 50) == (("lds", 3, True), 2, 3) and nc.gram_of("f64", "dense", 51) == (("lds", 4, False), 1, 4)
    assert nc.gram_of("f32", "dense", 50) == (("f16", 4), 0, 4) and nc.gram_of("f32", "sparse", 17) == (("sp", "float", 2), 3, 2)
    assert nc.info_of("f32", "sparse", 2, 33, True) == (2, 48, 3, 3) and nc.info_of("f64", "dense", 1, 49, True) == (1, 52, 2, 3)
    # the rank ends: both ends of every class of both SCD families, and the first rank beyond every short form
    for lo, hi in ((1, 16), (17, 32), (33, 48), (49, 50), (51, 64), (17, 20), (21, 32), (33, 36), (37, 48), (49, 52), (53, 64)):
        assert lo in nc.RANK_ENDS and hi in nc.RANK_ENDS, (lo, hi)


def test_cases_reach_every_instantiation():
    """All 47, each solver instantiation at every rank that maps to it; the masked and the unmasked form of every SCD solver with and
    without penalties at both of its rank ends."""
    want = nc.all_instantiations()
    assert len(want) == 47
    count = lambda fam: sum(1 for i in want if i[0] == fam)
    assert [count(f) for f in ("row", "strict", "ls", "lds", "f16", "sp")] == [10, 14, 4, 7, 4, 8]
    hit, ends = {}, {}
    for mode, door, method, k, variant in launches():
        masked, pen = nc.VARIANTS[variant]
        s = nc.solver_of(mode, method, k, masked)[0]
        hit.setdefault(s, set()).add(k)
        hit.setdefault(nc.gram_of(mode, door, k)[0], set()).add(k)
        if method == 1:
            ends.setdefault(s, set()).add((k, pen))
    assert set(hit) == want, sorted(want - set(hit), key=str)
    for inst, ks in hit.items():
        if inst[0] == "row":
            lo = {16: 1, 32: 17, 48: 33, 50: 49, 64: 51}[inst[3]]
            assert ks == set(range(lo, inst[3] + 1)), inst
        elif inst[0] == "strict":
            nkq, kr = inst[1], inst[3]
            lo = 16 * (nkq - 1) + 1 if (kr % 16 or nkq == 1) else 16 * (nkq - 1) + 5
            assert ks == set(range(lo, kr + 1)), inst
            for pen in (False, True):
                assert (lo, pen) in ends[inst] and (kr, pen) in ends[inst], inst
        elif inst[0] == "ls":
            assert ks == set(range(16 * inst[1] - 15, 16 * inst[1] + 1)) and {k % 8 for k in ks} == set(range(8)), inst
    for inst, kp in ends.items():
        if inst[0] == "row":
            lo = {16: 1, 32: 17, 48: 33, 50: 49, 64: 51}[inst[3]]
            for pen in (False, True):
                assert (lo, pen) in kp and (inst[3], pen) in kp, inst


def test_structure_of_the_cases():
    """The special lines, the masks, and at least 64 observed entries in every other line."""
    assert nc.N % 16 == 6 and nc.N % 4 == 2 and nc.M % 16 == 5 and nc.M % 4 == 1
    for k in (1, 2, 17, 50, 64):
        for variant in nc.VARIANTS:
            c = nc.make_case(k, variant)
            masked, pen = nc.VARIANTS[variant]
            A = c["A"]
            assert A.shape == (nc.N, nc.M) and np.nanmin(A) >= 0.1 and np.nanmax(A) <= 1.1
            miss = np.isnan(A)
            assert 0.17 < miss[5:, 5:].mean() < 0.23
            L, X = (miss, miss.T) if c["rows_special"] else (miss.T, miss)   # lines with the five; the cross lines
            assert [int(v) for v in L[:5].sum(axis=1)] == [0, 1, 7, L.shape[1] - nc.KEEP, L.shape[1]], (k, variant)
            assert [int(v) for v in X[:3].sum(axis=1)] == [1, 7, X.shape[1] - nc.KEEP], (k, variant)
            assert (~L[5:]).sum(axis=1).min() >= 64 and (~X[3:]).sum(axis=1).min() >= 64, (k, variant)
            # both sides of one half: a line that lists its missing rows and one that lists its present rows, in both orientations
            for Y in (L, X):
                assert (2 * Y.sum(axis=1) <= Y.shape[1]).any() and (2 * Y.sum(axis=1) > Y.shape[1]).any()
            assert (c["reg"] == list(nc.REG)) == pen and (c["Wm"] is not None) == masked
            assert (c["W0"] == 0).sum() > 0 and (c["H0"] == 0).sum() > 0
            if masked:
                Wm, HmT = c["Wm"], c["Hm"].T
                for Xm, line, X0 in ((Wm, nc.MASKED_LINE_W, c["W0"]), (HmT, nc.MASKED_LINE_H, c["H0"].T)):
                    assert Xm[line].all() and (X0[Xm] != 0).all()
                    assert not any(Xm[j].all() for j in range(line // 4 * 4, line // 4 * 4 + 4) if j != line), (k, variant)
                    if k >= 8:
                        assert 0.10 < np.delete(Xm, line, axis=0).mean() < 0.20
            S = nc.csc_of(A)
            assert S[0][-1] == (~miss).sum() and np.array_equal(np.diff(S[0]), (~miss).sum(axis=0))
            D = np.full(A.shape, np.nan)
            D[S[1], np.repeat(np.arange(nc.M), np.diff(S[0]))] = S[2]
            assert np.array_equal(np.isnan(D), miss) and np.array_equal(D[~miss], A[~miss])
            assert all((np.diff(S[1][S[0][j]:S[0][j + 1]]) > 0).all() for j in range(nc.M))


def test_row_list_case_has_every_length_on_both_sides_of_one_half():
    lens, n = nc.ROWLIST_LENS, nc.ROWLIST_N
    assert len(set(lens)) == len(lens) == 41
    assert set(lens) >= {0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 255, 256, 257, 288, 511, 512, 513, 600, 649, 650, 651, 700, 1299}
    assert set(lens) >= {2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17}
    assert {L for L in lens if 2 * L <= n} and max(L for L in lens if 2 * L <= n) == 650 and min(L for L in lens if 2 * L > n) == 651
    assert {n - L for L in lens if 2 * L > n} == {649, 600, 1}     # the lists of present rows
    for k in (1, 64):
        c = nc.make_rowlist_case(k)
        assert [int(v) for v in np.isnan(c["A"]).sum(axis=0)] == list(lens) and c["reg"] == list(nc.REG)
    # the ranks reach every Gram instantiation
    hit = {nc.gram_of(mode, door, k)[0] for k in nc.ROWLIST_KS for mode in nc.MODES for door in nc.DOORS}
    assert hit == {i for i in nc.all_instantiations() if i[0] in ("lds", "f16", "sp")}


def settings_of(k):
    return nc.SETTINGS + (nc.LIMIT_SETTINGS if k in nc.RANK_ENDS else ())


@pytest.mark.parametrize("k", nc.KS)
def test_oracle_counts_do_not_depend_on_the_order_of_the_contraction(k):
    """Every case whose strict sweep count the GPU file asserts (every variant and setting of the rank, SCD and -- tight -- Lee, the W
    half-step and the H half-step from the oracle's W): equal counts and solutions within 1e-11 under a permuted contraction index,
    outside nc.ORDER_DEPENDENT."""
    worst = 0.0
    for variant in nc.variants_of(k):
        c = nc.make_case(k, variant)
        rng = np.random.default_rng(k)
        pm, pn = rng.permutation(nc.M), rng.permutation(nc.N)
        for sname, setting in settings_of(k) + (("lee", nc.TIGHT),):
            method = 2 if sname == "lee" else 1
            name = nc.case_name(k, variant, sname)
            W, itw = nc.oracle_w(ref, c, *setting, method=method)
            Wp, itwp = nc.oracle_w(ref, c, *setting, method=method, perm=pm)
            H, ith = nc.oracle_h(ref, c, W, *setting, method=method)
            Hp, ithp = nc.oracle_h(ref, c, W, *setting, method=method, perm=pn)
            assert np.isfinite(W).all() and np.isfinite(H).all() and W.min() >= 0 and H.min() >= 0, name
            d = max(relF(Wp, W), relF(Hp, H))
            worst = max(worst, d)
            same = (itw, ith) == (itwp, ithp) and d < ORDER_BAR
            assert same == (name not in nc.ORDER_DEPENDENT), (name, itw, itwp, ith, ithp, d)
            if sname == "limit0":
                assert np.array_equal(W, c["W0"]) and np.array_equal(H, c["H0"]) and (itw, ith) == (0, 0)
            elif sname in ("limit1", "negtol"):  # no column stops before the limit
                assert (itw, ith) == (setting[0] * nc.live_columns(c), setting[0] * nc.live_columns_h(c)), name
    print(f"k={k}: order of the contraction moves the oracle by {worst:.2e} at most (bar {ORDER_BAR:g})")


def test_order_dependent_cases_are_few():
    names = {nc.case_name(k, v, s) for k in nc.KS for v in nc.variants_of(k) for s, _ in settings_of(k) + (("lee", None),)}
    assert nc.ORDER_DEPENDENT <= names and len(nc.ORDER_DEPENDENT) <= nc.MAX_ORDER_DEPENDENT


@pytest.mark.parametrize("cls", range(len(nc.ROW_CLASSES)))
def test_columns_of_a_wavefront_stop_at_different_sweeps_and_rounding_does_not_move_them(cls):
    """Per class of colsolve_row_kernel (k <= 16, 32, 48, 50, 64), at the loose setting, from the oracle's per-column sweep counts (one
    ref.update per column of the W half-step).  Early finishers: every rank has a variant with a wavefront -- four consecutive
    columns, 4 j .. 4 j + 3 -- whose columns stop at different sweeps, so a column that has converged keeps computing with its
    wavefront and its output must be the values of the sweep that ended it.  Input rounding: with A and the factors rounded to fp32 at
    most 3 of the 150 columns stop at another sweep than with fp64 inputs."""
    lo = 1 if cls == 0 else nc.ROW_CLASSES[cls - 1][1] + 1
    fewest, most_moved = None, 0
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    for k in range(lo, nc.ROW_CLASSES[cls][1] + 1):
        mixed = {}
        for variant in ("plain", "masked"):
            c = nc.make_case(k, variant)
            cnt = nc.column_counts_w(ref, c, *nc.LOOSE)
            assert int(cnt.sum()) == nc.oracle_w(ref, c, *nc.LOOSE)[1], (k, variant)
            waves = cnt[:nc.N // 4 * 4].reshape(-1, 4)
            mixed[variant] = int((waves.max(axis=1) != waves.min(axis=1)).sum())
            moved = int((nc.column_counts_w(ref, c, *nc.LOOSE, A=f32(c["A"]), W0=f32(c["W0"]), H0=f32(c["H0"])) != cnt).sum())
            most_moved = max(most_moved, moved)
            assert moved <= 3, (k, variant, moved)
        assert max(mixed.values()) >= 1, (k, mixed)
        fewest = max(mixed.values()) if fewest is None else min(fewest, max(mixed.values()))
    print(f"class KR={nc.ROW_CLASSES[cls][1]}: at least {fewest} wavefronts with columns stopping at different sweeps at every rank; "
          f"fp32 inputs move the stopping sweep of {most_moved} columns at most")
