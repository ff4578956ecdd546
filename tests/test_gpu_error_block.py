"""The error block -- mse_error, mkl_error, target_error, what the stopping rule of nnlm_run reads -- against exact sums and a long
double reference, at every rank and tile edge of every kernel that forms it (cases, reference and the restated launch rule:
tests/err_cases.py; that the cases reach every instantiation: tests/test_err_cases_host.py).

a. errors() right after set_factors(): the plain kernels (errors64_kernel, errors_f32_kernel, errors_kernel<T>, penalty_kernel) on known
   factors, both modes.
b. nnlm_run on FROZEN factors: with every entry of W and H masked the half-steps return the factors to the bit, so each trace entry of a
   three-iteration run is the error of the factors set: entries 0 and 1 from xprod16_err_kernel (inside the speculative W half-step),
   entry 2 from the plain kernel.  fp32-operand mode, methods 1 (factor16_fold_err_kernel feeds the kq-contiguous copies) and 2 (the
   general routine, prepare_factor16).
c. the same fused entry once in the real flow: unmasked, against the reference on the factors a twin handle's iterate(1) returns.
d. virtual ranks: every rank sums its own j-tiles; the shares are a partition.
e. stale state: a smaller rank, a smaller matrix and a repeated call on a used handle equal a fresh handle's to the bit.
f. the six penalty sums.

Bars.  The sum of squares of the "ones" and "planted" families is an integer every kernel forms without rounding (err_cases.py), so
mse == float(S) / N to the bit in both modes and all kernels.  Everything that rounds -- the KL part everywhere, mse of the random
families, kl_const -- is held as |gpu - ref| / (sum |term| / N) below 1e-10 (strict) and 1e-5 (fp32 operands), the bars the project
already puts on these sums; n_non_missing exactly; the penalty sums to 1e-13 relative (fp64 in both modes).  Each test prints its
largest deviations (`pytest -s`, lines "ERRDEV"); the largest per kernel and family are in DESIGN.md section 4.6."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import err_cases as ec  # noqa: E402
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib  # noqa: E402
from oracle import nnlm_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = [("f64", _lib.PREC_F64, 1e-10), ("f32", _lib.PREC_F32, 1e-5)]
PEN_BAR = 1e-13
Z = [0.0, 0.0, 0.0]
ALPHA, BETA = [0.02, 0.01, 0.03], [0.03, 0.02, 0.01]   # all six terms of add_penalty
INNER = 10


@pytest.fixture(autouse=True)
def _default_precision(monkeypatch):
    monkeypatch.delenv("NNLM_PRECISION", raising=False)


def shape_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else None


class Worst(collections.defaultdict):
    """Largest deviation per (kernel, family, quantity)."""

    def __init__(self):
        super().__init__(float)

    def note(self, key, v):
        self[key] = max(self[key], v)
        return v

    def line(self, what):
        print(f"ERRDEV {what}: " + (", ".join(f"{' '.join(k)} {v:.3e}" for k, v in sorted(self.items())) or "-"))


def check_matrix_info(info, case, r, bar, worst, kern):
    assert info["n_non_missing"] == r.N, (case, info["n_non_missing"], r.N)
    assert info["any_missing"] == (case.missing is not None), case
    dc = abs(float(ec.LD(info["kl_const"]) - r.kl_const)) / float(r.abs_const)
    assert worst.note((kern, case.family, "kl_const"), dc) < bar, (case, dc)


def check_sums(mse, kl, case, exact, r, bar, worst, kern, what=""):
    """One (mse, variable KL part) pair against the reference."""
    if exact is not None:
        want = float(exact) / r.N
        worst.note((kern, case.family, "mse"), abs(mse - want) / want)
        assert mse == want, (case, kern, what, mse, want, (mse - want) * r.N)   # (last: in entries)
    else:
        d2 = worst.note((kern, case.family, "mse"), ec.dev(mse, r.s2, r.abs2, r.N))
        assert d2 < bar, (case, kern, what, d2, mse)
    dk = worst.note((kern, case.family, "kl"), ec.dev(kl, r.kl, r.abskl, r.N))
    assert dk < bar, (case, kern, what, dk, kl)


def check_pen(pen, case, r, worst):
    for i in range(6):
        want = float(r.pen[i])
        d = abs(float(ec.LD(pen[i]) - r.pen[i])) / want if want > 0 else abs(pen[i])
        assert worst.note(("penalty_kernel", case.family, "pen"), d) < PEN_BAR, (case, i, pen[i], want)


def plain(prec, c, k):
    """(errors(), matrix_info()) of a fresh handle."""
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix(c["A"])
        h.set_factors(k, c["W"], c["H"])
        e = h.errors()
        assert h.get_info("xprod_splits_err") == 0   # (no fused launch on this handle)
        return e, h.matrix_info()


# ---- a. the plain kernels on known factors --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,bar", MODES)
@pytest.mark.parametrize("shape,k", ec.plain_groups(), ids=shape_id)
def test_plain_kernels_on_known_factors(shape, k, pname, prec, bar):
    """Every case of (shape, k): n_non_missing, kl_const, mse, the KL part and the six penalty sums of errors() on a fresh handle."""
    worst = Worst()
    for case in ec.plain_cases(shape, k):
        c = ec.make_case(*case)
        r = ec.ref_of(case, c)
        kern = ec.kernel_of(pname, case.k, case.missing is not None)
        (mse, kl, pen), info = plain(prec, c, case.k)
        check_matrix_info(info, case, r, bar, worst, kern)
        check_sums(mse, kl, case, c["exact"], r, bar, worst, kern)
        check_pen(pen, case, r, worst)
    worst.line(f"plain {shape_id(shape)} k={k} {pname}")


# ---- b. the fused kernel on frozen factors --------------------------------------------------------------------------------------------------
def frozen_run(c, k, method, alpha=Z, beta=Z, want_splits=None):
    """Three iterations with every entry of both factors masked: (traces, errors() after the run, matrix_info())."""
    n, m = c["A"].shape
    with nnlm_amd.Handle(0, _lib.PREC_F32) as h:
        h.set_matrix(c["A"])
        h.set_factors(k, c["W"], c["H"], np.ones((n, k), dtype=bool), np.ones((k, m), dtype=bool))
        assert h.get_info("xprod_splits_err") == 0
        t = h.run(alpha, beta, 3, -1.0, 0, False, INNER, 1e-9, method, 1)
        splits = int(h.get_info("xprod_splits_err"))
        assert splits >= 1, (splits, "the fused kernel did not run")
        if want_splits is not None:
            assert splits == want_splits, (splits, want_splits)
        W, H = h.get_factors()
        assert np.array_equal(W, c["W"]) and np.array_equal(H, c["H"]), "masked factors moved"
        assert t["n_iteration"] == 3 and len(t["mse_error"]) == len(t["mkl_error"]) == len(t["target_error"]) == 3, t
        return t, h.errors(), h.matrix_info()


def check_frozen(case, c, method, worst, alpha=Z, beta=Z, want_splits=None):
    r = ec.ref_of(case, c)
    miss = case.missing is not None
    fused, last = ec.kernel_of("f32", case.k, miss, fused=True), ec.kernel_of("f32", case.k, miss)
    t, after, info = frozen_run(c, case.k, method, alpha, beta, want_splits)
    what = f"method {method}"
    for i in range(3):
        kern = fused if i < 2 else last
        # mkl_error = kl_const + the variable part: the variable part, at the bar of the sum it is
        check_sums(t["mse_error"][i], t["mkl_error"][i] - info["kl_const"], case, c["exact"], r, 1e-5, worst, kern, f"{what} entry {i}")
        dm = abs(float(ec.LD(t["mkl_error"][i]) - (r.kl_const + r.kl / r.N))) / float(r.abs_const + r.abskl / r.N)
        assert worst.note((kern, case.family, "mkl"), dm) < 1e-5, (case, what, i, dm)
        if alpha is Z:
            assert t["target_error"][i] == 0.5 * t["mse_error"][i], (case, what, i)
        else:  # 0.5 mse + the penalty terms of the fp64 sums (1e-13 each): against the oracle's add_penalty on this mse
            want = nnlm_oracle.add_penalty(0.5 * t["mse_error"][i], c["W"].T, c["H"], r.N, alpha, beta)
            dt = abs(t["target_error"][i] - want) / want
            assert worst.note((kern, case.family, "target"), dt) < 1e-12, (case, what, i, dt)
    assert t["mse_error"][0] == t["mse_error"][1] and t["mkl_error"][0] == t["mkl_error"][1], (case, what, t)   # (the same launch twice)
    # entry 2 is the plain kernel's: the same launch as errors() on the same state
    assert t["mse_error"][2] == after[0] and t["mkl_error"][2] == info["kl_const"] + after[1], (case, what, t, after)


@pytest.mark.parametrize("shape,k", ec.fused_groups(), ids=shape_id)
def test_fused_kernel_on_frozen_factors(shape, k):
    """Every case of (shape, k), see b. in the module docstring."""
    worst = Worst()
    for case, methods in ec.fused_cases(shape, k):
        c = ec.make_case(*case)
        for method in methods:
            check_frozen(case, c, method, worst)
    worst.line(f"frozen {shape_id(shape)} k={k}")


@pytest.mark.parametrize("k", ec.RANKS_ENDS)
def test_fused_target_error_with_penalties(k):
    """target_error = 0.5 mse + the six penalty terms on frozen factors (the masks hold them against the penalties too)."""
    worst = Worst()
    n, m = ec.MAIN
    for family, missing in (("ones", None), ("uniform", "nan10")):
        case = ec.Case(family, n, m, k, missing)
        c = ec.make_case(*case)
        for method in (1, 2):
            check_frozen(case, c, method, worst, ALPHA, BETA)
    worst.line(f"frozen with penalties k={k}")


def fused_plan(n, m, k, cus):
    npad, mpad = ec.pads(n, m)
    return _lib.xprod_plan(npad, mpad // 64, k, cus, 8)   # (the fused kernel keeps 128-column blocks)


def test_fused_kernel_with_one_stage_of_columns_one_slab_and_several_slabs():
    """m = 64: one stage with entries (the second is padding); a shape the plan gives one slab, and the first of a list it gives
    several: the partial pairs of all slabs are reduced.  The plan is nnlm_xprod_plan's, the value that ran xprod_splits_err's."""
    worst = Worst()
    with nnlm_amd.Handle(0, _lib.PREC_F32) as h:
        cus = int(h.get_info("cus"))
    shapes = [(150, 64), ec.MAIN]
    assert all(fused_plan(n, m, 17, cus)["splits"] == 1 for n, m in shapes)
    several = [(n, m) for n, m in ((64, 1100), (64, 2100), (64, 4200), (64, 8300)) if fused_plan(n, m, 17, cus)["splits"] > 1]
    assert several, "no candidate shape is planned with more than one slab"
    for n, m in shapes + several[:1]:
        splits = fused_plan(n, m, 17, cus)["splits"]
        for family, missing in (("ones", None), ("ones", "word"), ("planted", "beside"), ("uniform", "nan10")):
            case = ec.Case(family, n, m, 17, missing)
            c = ec.make_case(*case)
            check_frozen(case, c, 1 if missing is None else 2, worst, want_splits=splits)
        print(f"ERRDEV {n}x{m}: xprod_splits_err {splits}")
    worst.line("frozen, stages and slabs")


# ---- c. the real flow once ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("k", [5, 50])
@pytest.mark.parametrize("missing", [None, "nan10"])
def test_fused_entry_of_a_real_run(missing, k, method):
    """Unmasked: trace entry 0 of run(max_iter = 2) is the fused kernel's value for the factors after one iteration -- the factors a twin
    handle's iterate(1) returns (asserted: run(max_iter = 1) and iterate(1) agree to the bit)."""
    n, m = ec.MAIN
    case = ec.Case("uniform", n, m, k, missing)
    c = ec.make_case(*case)

    def handle():
        h = nnlm_amd.Handle(0, _lib.PREC_F32)
        h.set_matrix(c["A"])
        h.set_factors(k, c["W"], c["H"])
        return h

    with handle() as h:
        h.iterate(1, Z, Z, INNER, 1e-9, method)
        W1, H1 = h.get_factors()
    with handle() as h:
        t1 = h.run(Z, Z, 1, -1.0, 0, False, INNER, 1e-9, method, 1)
        Wr, Hr = h.get_factors()
        assert h.get_info("xprod_splits_err") == 0 and len(t1["mse_error"]) == 1
    assert np.array_equal(Wr, W1) and np.array_equal(Hr, H1)
    with handle() as h:
        t2 = h.run(Z, Z, 2, -1.0, 0, False, INNER, 1e-9, method, 1)
        assert h.get_info("xprod_splits_err") >= 1 and len(t2["mse_error"]) == 2
        info = h.matrix_info()
    r = ec.err_ref(c["A"], W1, H1)
    worst = Worst()
    fused, last = ec.kernel_of("f32", k, missing is not None, fused=True), ec.kernel_of("f32", k, missing is not None)
    check_sums(t2["mse_error"][0], t2["mkl_error"][0] - info["kl_const"], case, None, r, 1e-5, worst, fused)
    check_sums(t1["mse_error"][0], t1["mkl_error"][0] - info["kl_const"], case, None, r, 1e-5, worst, last)
    worst.line(f"real run k={k} method {method} {missing}")


# ---- d. virtual ranks -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,bar", MODES)
@pytest.mark.parametrize("world,shape,k", [(2, ec.MAIN, 17), (3, ec.MAIN, 50), (3, ec.MAIN, 70), (5, (1153, 130), 17), (5, (1153, 130), 64)],
                         ids=shape_id)
def test_virtual_ranks_partition_the_error_sums(world, shape, k, pname, prec, bar):
    """"ones" without and with missing entries: a rank's mse is the number of finite entries in the columns of its j-tiles over N (one
    division: exact), a rank without a tile reports exactly 0 on its first call, and the shares add up to 1 within 1e-14."""
    n, m = shape
    for missing in (None, "nan10"):
        case = ec.Case("ones", n, m, k, missing)
        c = ec.make_case(*case)
        r = ec.ref_of(case, c)
        fin = np.isfinite(c["A"])
        tile = ec.tile_of(ec.kernel_of(pname, k, missing is not None, sharded=True))[1]
        shares, kls, empty = [], [], 0
        for rk in range(world):
            with nnlm_amd.Handle(0, prec) as h:
                h.comm_init(None, rk, world, form="cols")
                h.set_matrix(c["A"])
                h.set_factors(k, c["W"], c["H"])
                mse, kl, _ = h.errors()
            jt0, jcnt = ec.shard(tile, m, rk, world)
            count = int(fin[:, jt0 * tile:(jt0 + jcnt) * tile].sum())
            empty += jcnt == 0
            assert mse == count / r.N and (jcnt > 0 or (mse == 0.0 and kl == 0.0)), (case, world, rk, mse, count, r.N)
            shares.append(mse)
            kls.append(kl)
        assert abs(sum(shares) - 1.0) < 1e-14, (case, shares)
        assert empty > 0 or world < 5, (world, empty)   # (five ranks over 130 columns leave ranks without a j-tile in both modes)
        dk = ec.dev(sum(kls), r.kl, r.abskl, r.N)
        print(f"ERRDEV ranks {world} {shape_id(shape)} k={k} {pname} {missing}: shares {shares} kl {dk:.3e}")
        assert dk < bar, (case, dk)


# ---- e. stale state -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,bar", MODES)
@pytest.mark.parametrize("missing", [None, "nan10"])
def test_used_handle_equals_a_fresh_one(missing, pname, prec, bar):
    """Rank 64, then rank 5 on the same handle: rows 5 .. 63 of every operand copy are gone; then a smaller matrix on the same handle;
    errors() twice: all equal a fresh handle's values to the bit."""
    n, m = ec.MAIN
    big, small = ec.make_case("uniform", n, m, 64, missing), ec.make_case("uniform", n, m, 5, missing)
    tiny = ec.make_case("ones", 63, 65, 5, missing)

    def same(a, b):
        return a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])

    fresh_small, _ = plain(prec, small, 5)
    fresh_tiny, info_tiny = plain(prec, tiny, 5)
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix(big["A"])
        h.set_factors(64, big["W"], big["H"])
        first = h.errors()
        assert same(first, h.errors())
        h.set_matrix(small["A"])   # (the same shape, other entries)
        h.set_factors(5, small["W"], small["H"])
        got = h.errors()
        assert same(got, fresh_small) and same(got, h.errors()), (got, fresh_small)
        h.set_matrix(tiny["A"])    # (a smaller matrix: a second set_matrix is permitted)
        h.set_factors(5, tiny["W"], tiny["H"])
        got = h.errors()
        assert same(got, fresh_tiny) and h.matrix_info() == info_tiny, (got, fresh_tiny)
        assert got[0] == 1.0
    # the rank alone: the same matrix stays resident
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix(small["A"])
        h.set_factors(64, big["W"], big["H"])
        h.errors()
        h.set_factors(5, small["W"], small["H"])
        assert same(h.errors(), fresh_small)
    print(f"ERRDEV used handle {pname} {missing}: 0 (mse, KL part and penalty sums bit-identical to a fresh handle's: {fresh_small[0]!r}, {fresh_small[1]!r})")


# ---- f. the penalty sums --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,k", [(ec.MAIN, 17), (ec.MAIN, 70), ((1153, 130), 64)], ids=shape_id)
def test_penalty_sums(shape, k):
    """errors()[2] against the reference at 1e-13: one block and several blocks of 256 columns per factor, a rank beyond 64, factors of
    three magnitudes.  (The large shape's -- 17 blocks per factor -- are held by test_plain_kernels_on_known_factors, which checks the
    penalty sums of every case.)"""
    worst = Worst()
    n, m = shape
    for family in ("uniform", "scaled_up", "scaled_down", "zero_lines"):
        case = ec.Case(family, n, m, k, None)
        c = ec.make_case(*case)
        r = ec.ref_of(case, c)
        for pname, prec, _ in MODES:
            (_, _, pen), _ = plain(prec, c, k)
            check_pen(pen, case, r, worst)
    worst.line(f"penalty sums {shape_id(shape)} k={k}")
