"""Conditions on the error-block cases of tests/err_cases.py that need no GPU: the exact families are exact in three independent
evaluations, the oracle's _errors agrees with the long double reference on every case, and the case lists reach every instantiation of
every error kernel, with every kind of tile, at every rank."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import err_cases as ec  # noqa: E402
from oracle import nnlm_oracle  # noqa: E402

EPS = np.finfo(np.float64).eps


def oracle_errors(c):
    fin = np.isfinite(c["A"])
    return nnlm_oracle._errors(c["A"], np.ascontiguousarray(c["W"].T), c["H"], fin, not bool(fin.all()))


@pytest.fixture(scope="module")
def evaluated():
    """[(Case, exact, Ref, oracle mse, oracle kl, fp32 emulation of the sum of squares or None)] of every case below the large shape."""
    out = []
    for case in ec.all_cases():
        if (case.n, case.m) == ec.LARGE:
            continue
        c = ec.make_case(*case)
        mse, kl = oracle_errors(c)
        emu = ec.fp32_emulation_s2(c["A"], c["W"], c["H"]) if case.family in ec.EXACT else None
        out.append((case, c["exact"], ec.ref_of(case, c), mse, kl, emu))
    return out


def test_exact_families_are_exact_in_three_evaluations(evaluated):
    """"ones": the sum of squares is N; "planted": the sum of 4^t over the finite planted entries -- in the long double reference, in the
    fp32 emulation (fp32 operands, products and sums) and in the oracle.  The oracle forms mse as a mean of the finite entries (exact: an
    integer sum below 2^53, one division) when entries are missing, and as the mean of the column means otherwise: m + 1 divisions and a
    pairwise sum of m rounded quotients -- within (log2 m + 3) eps of S / N, and exactly 1 for "ones" (every column mean is 1)."""
    seen = collections.Counter()
    for case, exact, r, mse, _, emu in evaluated:
        if case.family not in ec.EXACT:
            continue
        seen[case.family] += 1
        assert exact is not None and float(r.s2) == exact and r.s2 == exact, case
        assert emu == exact, (case, emu, exact)
        want = float(exact) / r.N
        if case.family == "ones":
            assert exact == r.N and mse == 1.0, (case, mse)
        elif case.missing is not None:
            assert mse == want, (case, mse, want)
        else:
            assert abs(mse - want) <= (np.log2(case.m) + 3) * EPS * want, (case, mse, want)
            assert round(mse * r.N) == exact, (case, mse * r.N, exact)
    assert seen["ones"] > 200 and seen["planted"] > 200, seen


def test_planted_entries_sit_on_every_tile_edge():
    """Over the ranks of the main shape every listed edge row and column that exists holds a planted entry, every t = 0 .. 10 occurs, and
    the variant with a NaN beside every planted entry leaves all of them finite."""
    n, m = ec.MAIN
    rows, cols, ts = set(), set(), set()
    for k in ec.RANKS_ALL:
        pl = ec.planted_entries(n, m, k)
        assert len(pl) == 11 and len({(i, j) for i, j, _ in pl}) == 11
        rows |= {i for i, _, _ in pl}
        cols |= {j for _, j, _ in pl}
        ts |= {t for _, _, t in pl}
        c = ec.make_case("planted", n, m, k, "beside")
        fin = np.isfinite(c["A"])
        assert all(fin[i, j] for i, j, _ in pl) and (~fin).sum() == 11
        assert c["exact"] == sum(4 ** t for t in range(11)) < 2 ** 22
    assert rows == {r for r in ec.EDGE_ROWS + (n - 1,) if r < n} and cols == {c for c in ec.EDGE_COLS + (m - 1,) if c < m}
    assert ts == set(range(11))
    assert ec.planted_entries(1, 1, 5) == [(0, 0, 0)]


def test_oracle_errors_agree_with_the_reference_on_every_case(evaluated):
    """1e-13 of the mean |term| for both sums."""
    worst = [0.0, 0.0]
    for case, _, r, mse, kl, _ in evaluated:
        d2, dk = ec.dev(mse, r.s2, r.abs2, r.N), ec.dev(kl, r.kl, r.abskl, r.N)
        worst = [max(worst[0], d2), max(worst[1], dk)]
        assert d2 < 1e-13 and dk < 1e-13, (case, d2, dk)
    print(f"ERRDEV oracle against the reference: mse {worst[0]:.3e} kl {worst[1]:.3e}")


def test_large_shape_reference_is_exact_on_ones():
    n, m = ec.LARGE
    for case in ec.plain_cases(ec.LARGE, ec.LARGE_K):
        if case.family == "ones":
            c = ec.make_case(*case)
            r = ec.ref_of(case, c)
            assert r.s2 == c["exact"] == r.N and (r.N == n * m) == (case.missing is None), case


def test_zero_lines_put_zeros_under_both_kinds_of_entry():
    """wh = 0 under a > 0 and under a = 0, in an interior 64 x 64 tile (nnlm_log_tab in the strict kernel) and in the ragged last row
    tile (nnlm_log_pos)."""
    n, m = ec.MAIN
    c = ec.make_case("zero_lines", n, m, 17)
    wh = c["W"] @ c["H"]
    rows, col = ec.zero_lines_of(n, m)
    assert rows[0] < 64 <= n and rows[1] >= n - n % 64 and n % 64
    for i in rows:
        assert (wh[i] == 0).all() and (c["A"][i] > 0).any() and (c["A"][i] == 0).any()
    assert (wh[:, col] == 0).all() and (c["A"][:, col] > 0).any() and (c["A"][:, col] == 0).any()
    assert 0.25 < (c["A"] == 0).mean() < 0.35
    r = ec.ref_of(ec.Case("zero_lines", n, m, 17, None), c)
    assert np.isfinite(float(r.kl)) and np.isfinite(float(r.kl_const))


def test_case_lists_reach_every_instantiation_and_every_kind_of_tile():
    plain = collections.defaultdict(set)    # kernel -> kinds of tile
    ranks = collections.defaultdict(set)    # (mode, missing?) -> ranks
    for shape, k in ec.plain_groups():
        for case in ec.plain_cases(shape, k):
            for mode in ("f64", "f32"):
                kern = ec.kernel_of(mode, case.k, case.missing is not None)
                plain[kern] |= ec.tiles(kern, case.n, case.m)
                ranks[(mode, case.missing is not None)].add(case.k)
                if kern.startswith("errors64") and ec.strict_chunks(case.n, case.m).chunk > 1:
                    plain[kern].add("multi_tile")
    every = {"interior", "row_edge", "col_edge"}
    for miss in ("true", "false"):
        assert plain[f"errors64_kernel<{miss}>"] == every | {"multi_tile"}
        assert plain[f"errors_f32_kernel<{miss}>"] == every
    assert plain["errors_kernel<double>"] == every and plain["errors_kernel<float>"] == every
    assert len(plain) == 6
    for key in ranks:
        assert ranks[key] >= set(ec.RANKS_ALL) | set(ec.RANKS_GENERIC), key
    fused = collections.defaultdict(set)
    franks = collections.defaultdict(set)
    for shape, k in ec.fused_groups():
        for case, methods in ec.fused_cases(shape, k):
            kern = ec.kernel_of("f32", case.k, case.missing is not None, fused=True)
            fused[kern] |= ec.tiles(kern, case.n, case.m)
            franks[case.missing is not None] |= {(case.k, me) for me in methods}
    assert sorted(fused) == sorted(f"xprod16_err_kernel<{q}, {miss}>" for q in (1, 2, 3, 4) for miss in ("true", "false"))
    for kern, kinds in fused.items():
        assert kinds == every, (kern, kinds)
    for miss in (False, True):
        assert franks[miss] >= {(k, me) for k in ec.RANKS_ALL for me in (1, 2)}, miss
    assert {c.family for s, k in ec.fused_groups() for c, _ in ec.fused_cases(s, k)} == set(ec.FAMILIES)


def test_restated_geometry_of_the_named_shapes():
    """The figures the case list was chosen for, from the launch rule as restated (errors_launch, nnlm_mi355x.hip)."""
    assert ec.pads(150, 160) == (256, 256) and ec.pads(4100, 4101) == (4352, 4224)
    # small shapes: one j-tile per block
    assert ec.strict_chunks(150, 160) == ec.Chunks(4, 0, 4, 4, 1, 1)
    # the large shape: 68 i-tiles (three of them padding only), 66 j-tiles in 33 chunks of two: a block walks two tiles with the
    # double-buffered H slice, the last of them past the matrix
    g = ec.strict_chunks(*ec.LARGE)
    assert g == ec.Chunks(68, 0, 66, 33, 2, 2) and g.nit * g.nchunks == 2244
    # (1153, 130) in the fp32-operand mode: ten i-tiles in two rounds of eight block ids per j-tile -- 32 blocks, 12 of them idle
    assert ec.f32_grid(1153, 130) == (32, 20)
    # five ranks over 130 columns: two j-tiles of 128, four of 64 -- ranks without a tile in both modes
    assert [ec.shard(128, 130, r, 5)[1] for r in range(5)] == [1, 1, 0, 0, 0]
    assert [ec.shard(64, 130, r, 5)[1] for r in range(5)] == [1, 1, 1, 1, 0]
    assert [ec.shard(64, 160, r, 3) for r in range(3)] == [(0, 2), (2, 2), (4, 0)]
    assert ec.kernel_of("f32", 64, True, sharded=True, fused=True) == "errors_f32_kernel<true>"
    assert ec.kernel_of("f32", 64, False, sharded=True, fused=True) == "xprod16_err_kernel<4, false>"
    assert ec.kernel_of("f32", 65, False, fused=True) == "errors_kernel<float>" and ec.tile_of("errors_kernel<float>") == (64, 64)
    assert ec.tile_of("errors_f32_kernel<true>") == (128, 128) and ec.tile_of("xprod16_err_kernel<1, false>") == (128, 64)
