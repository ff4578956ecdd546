"""The launch plan of the split-fp16 cross product (xprod16_tn_kernel: 128- or 160-column blocks, split-K slabs), swept on the host
through the pure entry nnlm_xprod_plan -- no GPU.

The plan must cover every column and every contraction stage with no empty block, never ask for more LDS than a CU has, never pick the
160-column form where its ring does not fit (k > 52), and -- with 8 wavefronts forced on 256 compute units -- make the choice of slabs the
library made before it had a second block width."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from nnlm_amd import _lib  # noqa: E402

STAGES = (1, 2, 7, 8, 79, 158, 316)
CUS = (3, 7, 256)
LDS_MAX = 160 * 1024


def old_split_plan(tiles_x, stages):
    """split_plan() as it stood with `cus = 256` written into it and 128-column tiles only."""
    best_s, best = 1, 1e300
    for s in range(1, 17):
        if s > 1 and stages // s < 8:
            break
        rounds = (tiles_x * s + 255) // 256
        per_block = (stages + s - 1) // s
        cost = rounds * (per_block + 3) + 0.75 * s
        if cost < best - 1e-9:
            best, best_s = cost, s
    per = max((stages + best_s - 1) // best_s, 1)
    return max((stages + per - 1) // per, 1), per


def check(p, ldc, stages, k):
    w, S, sps, tiles = p["waves"], p["splits"], p["stages_per_split"], p["tiles"]
    assert w in (8, 10)
    assert S >= 1 and sps >= 1 and S * sps >= stages and (S - 1) * sps < stages, (p, stages)  # every stage covered, no empty block
    assert tiles * 16 * w >= ldc and (tiles - 1) * 16 * w < ldc, (p, ldc)  # the tiles cover ldc, none starts beyond it
    assert p["blocks"] == tiles * S
    assert p["pieces"] == (13 if 49 <= k <= 52 else 4 * ((k + 15) // 16))
    assert p["lds_bytes"] <= LDS_MAX, p
    assert p["lds_bytes"] >= 3 * (w * 4096 + p["pieces"] * 1024)
    if k > 52:
        assert w == 8, (p, k)


@pytest.mark.parametrize("cus", CUS)
def test_plan_sweep(cus):
    for ldc in range(128, 20224 + 1, 128):
        for stages in STAGES:
            for k in range(1, 65):
                check(_lib.xprod_plan(ldc, stages, k, cus), ldc, stages, k)


@pytest.mark.parametrize("cus", CUS)
def test_forced_widths(cus):
    for ldc in list(range(128, 2048 + 1, 128)) + [10112, 20224]:
        for stages in STAGES:
            for k in (1, 5, 16, 17, 48, 49, 50, 52, 53, 64):
                p8, p10 = _lib.xprod_plan(ldc, stages, k, cus, 8), _lib.xprod_plan(ldc, stages, k, cus, 10)
                check(p8, ldc, stages, k)
                check(p10, ldc, stages, k)
                assert p8["waves"] == 8
                assert p10["waves"] == (10 if k <= 52 else 8)


def test_eight_wavefronts_on_256_cus_reproduce_the_earlier_plan():
    for ldc in range(128, 20224 + 1, 128):
        for stages in STAGES:
            for k in (1, 50, 64):
                p = _lib.xprod_plan(ldc, stages, k, 256, 8)
                assert (p["splits"], p["stages_per_split"]) == old_split_plan(ldc // 128, stages), (ldc, stages, k, p)


def test_plan_of_the_benchmark_launches():
    """Config 2 (20000 x 10000, k = 50) on 256 compute units: both launches fill the device in one round of 160-column blocks."""
    h = _lib.xprod_plan(10112, 316, 50, 256)
    assert (h["waves"], h["splits"], h["blocks"]) == (10, 4, 256), h
    w = _lib.xprod_plan(20224, 158, 50, 256)
    assert (w["waves"], w["splits"], w["blocks"]) == (10, 2, 254), w


def test_bad_arguments_are_refused():
    for args in ((100, 10, 5, 256, 0), (128, 0, 5, 256, 0), (128, 10, 0, 256, 0), (128, 10, 65, 256, 0), (128, 10, 5, 0, 0), (128, 10, 5, 256, 9)):
        with pytest.raises(_lib.NnlmError):
            _lib.xprod_plan(*args)
