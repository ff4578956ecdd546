"""Conditions on the cases of tests/scd_sweep_cases.py, from the restated launch policy and the fp64 oracle alone (no GPU): the cases reach
every one of the 144 instantiations of the four dense SCD sweep kernels (the switch tables of tu_sweepq.hip, tu_sweepqw.hip,
tu_sweepf.hip and tu_sweepr.hip) with every rank tail, and every column-group count G the persistent form can be given; they are well
posed (the oracle agrees with itself under another order of summation far inside the 1e-10 the GPU tests hold the strict kernels to, no
factor dies), and the oracle's sweep counts do not ride on the order of summation where the GPU tests compare them exactly."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scd_sweep_cases as sc  # noqa: E402
from helpers import relF  # noqa: E402
from oracle import ref  # noqa: E402

STRICT_BAR = 1e-10


def launches():
    """(prec, k, variant, cus, Form) of every W half-step launch test_gpu_scd_forms.py's main test makes at the TIGHT / LOOSE settings."""
    for k in sc.KS:
        for variant in sc.variants_of(k):
            for prec in ("f64", "f32"):
                for cus in sc.cus_of(prec, k):
                    yield prec, k, variant, cus, sc.policy(prec, k, sc.N, cus, sc.TIGHT[0])


def test_policy_on_150_columns_as_written():
    """What launch_sweep_f / launch_sweep_q give 150 columns on 1, 3, 5 and 10 compute units, and the 160 columns of the H half-step."""
    for k in sc.KS:
        NB, NT = (k + 3) // 4, (k + 15) // 16
        assert sc.policy("f32", k, 150, 1, 30) == sc.Form("f", NB, NT, 8, 2)    # 10 groups on 4 SIMDs: two per SIMD, 128 columns per workgroup
        assert sc.policy("f32", k, 150, 3, 30) == sc.Form("f", NB, NT, 4, 3)    # 10 groups on 12 SIMDs
        if k <= 50:
            assert sc.policy("f32", k, 150, 5, 30) == sc.Form("r", NB, NT, 8, 5)    # 150 <= 32 * 5: workgroups of 32 columns
            assert sc.policy("f32", k, 150, 10, 30) == sc.Form("r", NB, NT, 4, 10)  # 150 <= 16 * 10: workgroups of 16 columns
        else:
            assert sc.policy("f32", k, 150, 5, 30).family == sc.policy("f32", k, 150, 10, 30).family == "f"
        assert sc.policy("f64", k, 150, 1, 30) == sc.Form("qw", NB, NT, 5, 2)   # 10 groups on one CU: two workgroups of G = 5
        assert sc.policy("f64", k, 150, 3, 30) == sc.Form("q", NB, NT, 4, 3)
        for inner in sc.INNER_LIMITS:  # below four sweeps the persistent form is not taken
            assert sc.policy("f64", k, 150, 1, inner) == sc.Form("q", NB, NT, 4, 3)
        assert sc.policy("f64", k, 150, 1, 4).family == "qw"
        for prec in ("f64", "f32"):  # the H half-step (160 columns, ten whole groups) takes the same family and width
            for cus in sc.cus_of(prec, k):
                fw, fh = sc.policy(prec, k, sc.N, cus, 30), sc.policy(prec, k, sc.M, cus, 30)
                assert (fw.family, fw.groups) == (fh.family, fh.groups), (prec, k, cus)
    # 150 columns are ragged for every workgroup shape
    assert 150 % 16 == 6 and 150 % 64 == 22 and 150 % 128 == 22 and 150 % 32 == 22 and 150 % 80 != 0
    assert sc.masked_columns() == [3, 143, 147, 149]


def test_cases_reach_every_instantiation_with_every_rank_tail():
    """The 32 + 32 + 64 + 16 instantiations of the switch tables, each by every rank that maps to it -- so each NB with its four k % 4
    tails (1, 2, 3 coordinates in the last block, or a full one) and each row class at all of its ranks (KR = 50: k = 49 and 50)."""
    want = sc.all_instantiations()
    assert len(want) == 144
    assert sum(1 for i in want if i[0] == "q") == 32 and sum(1 for i in want if i[0] == "qw") == 32
    assert sum(1 for i in want if i[0] == "f") == 64 and sum(1 for i in want if i[0] == "r") == 16
    hit = {}
    for prec, k, variant, cus, form in launches():
        hit.setdefault(sc.instantiation(form, sc.VARIANTS[variant][0]), set()).add(k)
    assert set(hit) == want, sorted(want - set(hit))
    for inst, ks in hit.items():
        if inst[0] == "r":
            cpl, kr = inst[1], inst[2]
            assert ks == set(range(16 * (cpl - 1) + 1, kr + 1)), inst
        else:
            NB = inst[2]
            assert ks == set(range(4 * NB - 3, 4 * NB + 1)) and {k % 4 for k in ks} == {0, 1, 2, 3}, inst
    # the swapped combinations (mask without penalties, penalties without mask) sit on the rank ends of every rank padding
    assert {(k + 15) // 16 for k in sc.NT_ENDS} == {1, 2, 3, 4}
    for NT in (1, 2, 3, 4):
        assert 16 * NT in sc.NT_ENDS and 16 * (NT - 1) + 1 in sc.NT_ENDS
    # both families of the second kind: the persistent form at NB = 1, 6, 11, 15 and the plain form below its threshold
    assert [(k + 3) // 4 for k in sc.KS_FEW] == [1, 6, 11, 15]
    for k in sc.KS_FEW:
        for cus, n, G in sc.G_SHAPES:
            assert sc.policy("f64", k, n, cus, sc.TIGHT[0]) == sc.Form("qw", (k + 3) // 4, (k + 15) // 16, G, -(-((n + 15) // 16) // G)), (k, cus, n)
        for inner in sc.INNER_LIMITS:
            f = sc.policy("f64", k, sc.N, 1, inner)
            assert f.family == "q" and (sc.N + 15) // 16 > 4 * 1  # plain, more than one wavefront per SIMD


def chosen_groups(cus, ngroups, gmax):
    """launch_sweep_q's choice of G for arrays of group counts on `cus` compute units, g <= gmax fitting the LDS; 0 = the plain form."""
    simds = 4 * cus
    best = (ngroups + simds - 1) // simds * 4
    G = np.zeros_like(ngroups)
    for g in range(5, gmax + 1):
        cost = ((ngroups + g - 1) // g + cus - 1) // cus * g
        better = (cost < best) & (ngroups > simds)
        best, G = np.where(better, cost, best), np.where(better, g, G)
    return G


def test_group_counts_the_policy_can_choose():
    """Over every CU count up to 256 and every column-group count up to 16 per SIMD the persistent form is given G = 5, 6, 7 or 9 and
    nothing else: a tie keeps the smaller G (the comparison is `<`), G = 10 always ties with G = 5 in twice the rounds and G = 8 never
    beats 5 .. 7.  At k = 61 .. 64 nine groups no longer fit the LDS (the loop breaks at G = 9): 5, 6, 7.  So "G = 10" for 2500 groups
    on 256 CUs or 19 groups on two is G = 5 in two rounds of workgroups, at the same cost."""
    gmax = {k: max(g for g in range(5, sc.WRAP_MAXG + 1) if sc.sweepqw_lds_bytes(16 * ((k + 15) // 16), (k + 3) // 4, g) <= sc.LDS_LIMIT) for k in sc.KS}
    assert {k for k in sc.KS if gmax[k] < 10} == {57, 58, 59, 60, 61, 62, 63, 64} and gmax[60] == 9 and gmax[61] == 8 and gmax[56] == 10
    seen = {8: set(), 9: set(), 10: set()}
    for cus in range(1, 257):
        ng = np.arange(1, 64 * cus + 1)
        for gm in seen:
            seen[gm] |= set(np.unique(chosen_groups(cus, ng, gm)).tolist())
    assert seen[10] == seen[9] == {0, 5, 6, 7, 9} and seen[8] == {0, 5, 6, 7}
    rng = np.random.default_rng(0)
    for _ in range(2000):  # the vectorised form above is the policy
        cus, k = int(rng.integers(1, 257)), int(rng.integers(1, 65))
        ngr = int(rng.integers(1, 64 * cus + 1))
        f = sc.policy("f64", k, 16 * ngr, cus, 30)
        assert (f.groups if f.family == "qw" else 0) == int(chosen_groups(cus, np.array([ngr]), gmax[k])[0])
    assert sc.policy("f64", 50, 40000, 256, 50) == sc.Form("qw", 13, 4, 5, 500)  # two rounds of 256 workgroups
    assert sc.policy("f64", 50, 19 * 16, 2, 50) == sc.Form("qw", 13, 4, 5, 4)
    assert {G for _, _, G in sc.G_SHAPES} == {5, 6, 7, 9}
    assert all(sc.policy("f64", 7, n, cus, 9).groups == G for cus, n, G in sc.G_SHAPES)


def check_case(c, w_setting, h_setting, what):
    """The oracle's chain under both orders: agreement to the strict bar, live factors, the structure of the start.  Returns
    (deviation, counts equal under both orders)."""
    k, n = c["k"], c["n"]
    W, itw, H, ith = sc.oracle_chain(ref, k, c["variant"], w_setting, h_setting, False, n)
    Wr, itwr, Hr, ithr = sc.oracle_chain(ref, k, c["variant"], w_setting, h_setting, True, n)
    d = max(relF(Wr, W), relF(Hr, H))
    assert d < STRICT_BAR, (what, d)
    assert np.isfinite(W).all() and np.isfinite(H).all() and W.min() >= 0 and H.min() >= 0
    for nrm in ((W * W).sum(axis=0), (H * H).sum(axis=1)):  # no column of W, no row of H dies
        assert nrm.min() > 1e-2 * np.median(nrm), (what, nrm.min(), np.median(nrm))
    if c["Wm"] is not None:
        assert np.array_equal(W[c["Wm"]], c["W0"][c["Wm"]]) and np.array_equal(H[c["Hm"]], c["H0"][c["Hm"]])
    return d, (itw, ith) == (itwr, ithr), (itw, ith)


@pytest.mark.parametrize("k", sc.KS)
def test_case_is_well_posed(k):
    """Per rank, every variant at both settings: see check_case.  The start has zeros that stay zero and zeros that leave zero (k = 1:
    A > 0 and H > 0 make every free coordinate positive), the masked variants hold about 10 % masked entries with values other than zero,
    bit 0 and bit k - 1 masked in a live column and the four fully masked columns; the tight setting's counts do not depend on the order
    of summation; at the loose one columns stop at different sweeps."""
    worst = 0.0
    for variant in sc.variants_of(k):
        c = sc.make_case(k, variant)
        masked, pen = sc.VARIANTS[variant]
        assert c["A"].shape == (150, 160) and c["A"].min() > 0 and 160 >= 2.5 * k
        assert (c["reg"] == list(sc.REG)) == pen and (c["Wm"] is not None) == masked
        free = np.ones((sc.N, k), bool) if not masked else ~c["Wm"]
        live = sc.N
        if masked:
            Wm = c["Wm"]
            assert Wm[sc.masked_columns()].all() and (c["W0"][Wm] != 0).all() and (c["H0"][c["Hm"]] != 0).all()
            assert 0.06 < np.delete(Wm, sc.masked_columns(), axis=0).mean() < 0.15 and 0.05 < c["Hm"].mean() < 0.16  # about 10 %
            assert Wm[5, 0] and Wm[7, k - 1] and (k == 1 or not (Wm[5].all() or Wm[7].all()))
            live = sc.live_columns(c)
            assert live <= sc.N - 4
        for sname, setting in sc.SETTINGS:
            d, same, (itw, ith) = check_case(c, setting, None, sc.case_name(k, variant, sname))
            worst = max(worst, d)
            W = sc.oracle_chain(ref, k, variant, setting)[0]
            if sname == "tight":
                assert same, (k, variant, "tight sweep counts depend on the order of summation")
                z0 = (c["W0"] == 0) & free
                assert (z0 & (W > 0)).sum() >= 5, (k, variant)
                if k >= 2:
                    assert (z0 & (W == 0)).sum() >= 1, (k, variant)
            else:
                assert same == (sc.case_name(k, variant, sname) not in sc.LOOSE_ORDER_DEPENDENT), (k, variant, itw, ith)
                if k >= 2:  # a mix: some column stops before the budget, not every column after its first sweeps
                    assert 2 * live < itw < sc.LOOSE[0] * live, (k, variant, itw, live)
    print(f"k={k}: order of summation moves the oracle by {worst:.2e} at most (bar {STRICT_BAR:g})")


def test_order_dependent_loose_cases_are_few():
    names = [sc.case_name(k, v, "loose") for k in sc.KS for v in sc.variants_of(k)]
    assert sc.LOOSE_ORDER_DEPENDENT <= set(names) and len(sc.LOOSE_ORDER_DEPENDENT) <= 0.05 * len(names)


@pytest.mark.parametrize("k", sc.KS_FEW)
def test_second_family_is_well_posed(k):
    """The persistent form's cases at G = 5, 6, 7, 9 (150, 260, 112, 144 columns) and the inner limits 0, 1, 3 (then an H half-step at the
    tight setting); a limit of 0 leaves the factor as it is and counts no sweep."""
    worst = 0.0
    for cus, n, G in sc.G_SHAPES:
        c = sc.make_case(k, "masked", n)
        for sname, setting in sc.SETTINGS:
            d, same, _ = check_case(c, setting, None, f"k{k}-G{G}-{sname}")
            assert same, (k, G, sname)
            worst = max(worst, d)
    c = sc.make_case(k, "masked")
    for inner in sc.INNER_LIMITS:
        d, same, (itw, ith) = check_case(c, (inner, sc.TIGHT[1]), sc.TIGHT, f"k{k}-inner{inner}")
        live = sc.live_columns(c)  # (a column with one free coordinate stops after its second sweep)
        assert same and (itw == inner * live if inner <= 1 else 2 * live <= itw <= inner * live)
        worst = max(worst, d)
    W0 = sc.oracle_chain(ref, k, "masked", (0, sc.TIGHT[1]), sc.TIGHT)[0]
    assert np.array_equal(W0, c["W0"])
    print(f"k={k}: order of summation moves the oracle by {worst:.2e} at most (bar {STRICT_BAR:g})")
