"""The conditions under which tests/test_gpu_kl_pieces.py says something, checked without a GPU: the case table of tests/kl_piece_cases.py
reaches every instantiation the KL launch plan (nnlm_kl_plan, a pure host entry built from the launchers' own helpers) can choose, its
restated dispatch is the library's, the plan is sane over every length, and the oracle alone shows that one lost boundary element of a
case moves every column by far more than the bar the GPU test holds the kernels to."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kl_piece_cases as kc  # noqa: E402
from nnlm_amd import _lib  # noqa: E402
from oracle import ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP_END = 41000
PREC = {"tile": _lib.PREC_F32, "reg64": _lib.PREC_F64}
LDS_MAX = 160 * 1024


def plan(kind, p, mask_words=0):
    return _lib.kl_plan(p, kc.K, PREC[kind], mask_words)


def key(pl):
    return (pl["kernel"], pl["pieces"], pl["cols"])


@pytest.fixture(scope="module")
def sweep():
    """{(kind, mask words): [plan of p = 1 .. SWEEP_END]} at the cases' rank."""
    return {(kind, mw): [plan(kind, p, mw) for p in range(1, SWEEP_END + 1)] for kind in ("tile", "reg64") for mw in (0, 1)}


def members(sweep):
    """Every (kind, kernel, instantiated pieces, columns per block) the plan can return."""
    return {(kind,) + key(pl) for (kind, _), plans in sweep.items() for pl in plans}


def uncovered(cases, sweep):
    """Members of the plan that fewer than three distinct H-orientation lengths of `cases` reach (the streaming kernel: fewer than one --
    it is out of this table's scope beyond the first length past each switch point)."""
    reach = {}
    for c in cases:
        if c["orient"] == "H":
            reach.setdefault((c["kind"],) + tuple(c["plan"]), set()).add(c["p"])
    return sorted(m for m in members(sweep) if len(reach.get(m, ())) < (1 if m[1] == kc.STREAM else 3))


def test_the_entry_is_declared_exported_and_refuses_bad_arguments():
    hdr = open(os.path.join(ROOT, "include", "nnlm_mi355x.h")).read()
    assert re.search(r"^int nnlm_kl_plan\(int p, int k, int precision, int mask_words, int out\[8\]\);", hdr, re.M)
    assert "#define NNLM_ABI_VERSION 1" in hdr and _lib.load().nnlm_abi_version() == 1  # (an added entry: the version stays, as before)
    assert "nnlm_kl_plan" in _lib.EXPORTS
    for k in ("kl_pieces_w", "kl_pieces_h", "kl_cols_w", "kl_cols_h"):
        assert '"%s"' % k in hdr
    for bad in ((0, 3, _lib.PREC_F32, 0), (5, 0, _lib.PREC_F32, 0), (5, 3, 7, 0), (5, 3, _lib.PREC_F64, -1)):
        with pytest.raises(_lib.NnlmError):
            _lib.kl_plan(*bad)


def test_every_case_plans_as_the_table_says():
    """The restated dispatch of kl_piece_cases (tile_plan, reg64_plan, the piece counts, the hard-coded switch points) is the library's."""
    for c in kc.CASES + kc.OWN_INIT_CASES:
        pl = plan(c["kind"], c["p"], 1 if c["masked"] else 0)
        assert key(pl) == tuple(c["plan"]) and pl["pieces_exact"] == c["pieces_exact"], (c["id"], pl)
        assert c["ncols"] == (2 * pl["cols"] + 1 if pl["cols"] else 3)
        if c["tag"] == "lo":
            assert pl["last_waves"] == (1 if pl["pieces"] == pl["pieces_exact"] else 0), (c["id"], pl)  # wavefront 0 alone owns the last piece
        if c["tag"] == "hi" and c["p"] not in (kc.TILE2_MAX_P, kc.TILE_MAX_P):
            assert pl["last_waves"] == (8 if pl["pieces"] == pl["pieces_exact"] else 0), (c["id"], pl)
        if c["tag"] == "cut-in":  # W orientation: the row ends in the lower half of a wavefront piece, the leading dimension cuts it there
            assert 0 < c["p"] % 256 <= 128 and (c["p"] + 127) // 128 % 2 == 1
        if c["tag"] == "cut-out":
            assert c["p"] % 256 == 129


def test_the_table_reaches_every_instantiation_the_plan_can_choose(sweep):
    """Every (kernel, instantiated pieces, columns per block) nnlm_kl_plan returns for p = 1 .. 41000 in either mode, with or without a
    mask word, is reached by at least three H-orientation lengths; every exact reg64 piece count 1 .. 20 by one; the W orientation by the
    subset the table promises.  An instantiation added to launch_kl_tile() / launch_kl64() without cases fails here -- and so does the
    table with any one member's cases taken out."""
    assert uncovered(kc.CASES, sweep) == []
    ms = members(sweep)
    assert len([m for m in ms if m[0] == "tile" and m[1] != kc.STREAM]) == 20 and len([m for m in ms if m[1] == kc.REG64]) == len(kc.R64_RUNGS)
    for m in ms:
        fewer = [c for c in kc.CASES if (c["kind"],) + tuple(c["plan"]) != m]
        assert m in uncovered(fewer, sweep), m
    assert {c["pieces_exact"] for c in kc.H_CASES if c["plan"][0] == kc.REG64} == set(range(1, 21))
    for e in range(1, 21):  # both methods at both ends of every exact piece count, one at its middle
        for kind in ("tile", "reg64"):
            got = sorted((c["tag"], c["method"]) for c in kc.H_CASES if c["kind"] == kind and c["pieces_exact"] == e and c["plan"][0] != kc.STREAM)
            assert [g for g in got if g[0] != "mid"] == [("hi", 3), ("hi", 4), ("lo", 3), ("lo", 4)] and len(got) == 5, (kind, e, got)
    wt = {c["plan"][1] for c in kc.W_CASES if c["kind"] == "tile"}
    assert wt >= {1, 2, 3, 5, 6, 10, 11, 15, 20}
    for e in wt:
        assert sorted(c["tag"] for c in kc.W_CASES if c["kind"] == "tile" and c["plan"][1] == e) == ["cut-in", "cut-out"]
    assert {c["plan"][1] for c in kc.W_CASES if c["kind"] == "reg64"} == set(kc.R64_RUNGS)
    assert {(c["pieces_exact"], c["method"]) for c in kc.OWN_INIT_CASES} == {(e, m) for e in range(4, 11) for m in (3, 4)}
    flags = {(c["nan_edge"], c["masked"]) for c in kc.CASES}
    assert len(flags) == 4  # weighted missing edge entries and masks, alone and together


def test_the_plan_is_sane_at_every_length(sweep):
    """Tile pieces are exact, reg64 pieces the smallest instantiated count that holds the exact one, the dynamic LDS fits 160 KiB, C x pieces
    stays within the 160 state registers the launchers assume (20 sixteen-byte slots per thread), and the kernels change hands exactly where
    the case table says: two row buffers up to 20224, streaming for 20225 .. 20480 (10 pieces fit neither form), one row buffer for
    20481 .. 40192, streaming beyond; strict mode: registers up to 20480, streaming beyond."""
    for (kind, mw), plans in sweep.items():
        for p, pl in enumerate(plans, start=1):
            assert pl["lds_bytes"] <= LDS_MAX, (kind, p, pl)
            if pl["kernel"] == kc.STREAM:
                assert key(pl) == (kc.STREAM, 0, 0) and pl["last_waves"] == 0
                continue
            assert pl["cols"] * pl["pieces"] <= 20 and pl["cols"] in (1, 2, 4, 8), (kind, p, pl)
            if kind == "tile":
                p4 = ((p + 3) // 4 + 63) // 64 * 64
                assert pl["pieces"] == pl["pieces_exact"] and (pl["pieces"] - 1) * 512 < p4 <= pl["pieces"] * 512, (p, pl)
                assert pl["kernel"] == (kc.TILE2 if pl["pieces"] <= 10 else kc.TILE1)
                assert pl["last_waves"] == min(8, (p4 - (pl["pieces"] - 1) * 512) // 64)
            else:
                p2 = (p + 1) // 2
                assert (pl["pieces_exact"] - 1) * 512 < p2 <= pl["pieces_exact"] * 512 and pl["kernel"] == kc.REG64
                assert pl["pieces"] == min(r for r in kc.R64_RUNGS if r >= pl["pieces_exact"])
        kernels = [pl["kernel"] for pl in plans]
        if kind == "tile":
            want = [kc.TILE2] * kc.TILE2_MAX_P + [kc.STREAM] * (20480 - kc.TILE2_MAX_P) + [kc.TILE1] * (kc.TILE_MAX_P - 20480)
        else:
            want = [kc.REG64] * kc.R64_MAX_P
        assert kernels == want + [kc.STREAM] * (SWEEP_END - len(want)), (kind, mw)


def test_one_lost_boundary_element_moves_every_column_far_beyond_the_bar():
    """Every H and W case: zero ONE probed edge element (p - 1; the first element of the last wavefront piece that exists; the element in
    front of the last piece) in A and in the fixed factor -- what a dropped slot, a wrong `last` predicate or a wait count off by one would
    do to it -- and the oracle's result moves in EVERY column that is not fully masked by at least 5e-3 relative, 50 times the fp32 bar of
    the GPU test.  Smallest value over all 235 cases and their probes: 9.9e-3 (tile-H-p2048-m3-hi, element 0).  (Edge rows of the same
    weight but uniformly random like the rest: 0 -- a column whose one free coordinate is clamped, or whose lost row happens to have the
    fitted ratio, does not move; hence kl_piece_cases.EDGE_RATIO and the small given values of masked coordinates.)"""
    worst = (np.inf, None, None)
    for c in kc.CASES:
        d = kc.make_data(c)
        X, _ = kc.oracle(ref, c["id"])
        live = np.ones(c["ncols"], bool) if d["mask"] is None else ~d["mask"].all(axis=0)
        probes = kc.probe_indices(c)
        assert c["p"] - 1 in probes and set(probes) <= set(d["edges"]) and (len(probes) >= 2 or c["p"] < 3), c["id"]
        assert not np.isnan(d["Ac"][probes, :]).any()  # (the weighted missing entries sit on the other edges)
        for i in probes:
            A2, Y2 = d["Ac"].copy(), d["Y"].copy()
            A2[i, :] = 0.0
            Y2[:, i] = 0.0
            X2, _ = ref.update(d["X0"], Y2, A2, d["mask"], kc.REG, kc.INNER, kc.TOL, c["method"])
            s = float(kc.col_err(X2, X)[live].min())
            worst = min(worst, (s, c["id"], i))
    print("smallest sensitivity", worst)
    assert worst[0] >= 5e-3, worst


def test_the_data_are_what_the_table_promises():
    """About 2 % missing, weighted edges never missing by chance, one weighted missing entry per column where the case says so, about 30 %
    of the solved factor masked and column 1 entirely; cases that differ in the method alone share their data."""
    for c in kc.CASES[::7] + kc.OWN_INIT_CASES[:2]:
        d = kc.make_data(c)
        p, nc = c["p"], c["ncols"]
        assert d["Ac"].shape == (p, nc) and d["Y"].shape == (kc.K, p) and d["X0"].shape == (kc.K, nc)
        nan = np.isnan(d["Ac"])
        assert nan[d["edges"], :].sum() == (nc if c["nan_edge"] and len(d["edges"]) > len(kc.probe_indices(c)) else 0)
        if p > 2000:
            assert 0.015 < nan.mean() < 0.025
        if c["masked"]:
            assert d["mask"][:, 1].all() and d["mask"].shape == (kc.K, nc)
        else:
            assert d["mask"] is None
        d2 = kc.make_data(dict(c, method=7 - c["method"]))
        assert np.array_equal(d["Ac"], d2["Ac"], equal_nan=True) and np.array_equal(d["Y"], d2["Y"])
