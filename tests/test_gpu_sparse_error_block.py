"""The error block of a sparse A -- Handle.errors() through set_matrix_csc, set_matrix_csc_missing and both weighted doors -- against
exact sums and a long double reference at every rank 1 .. 64 (65 and 70 where the door takes them), in both modes (cases, reference and
the restated forms: tests/sparse_err_cases.py; that they reach all 18 forms of the sums over the stored entries and the conditions
relied on here: tests/test_sparse_err_cases_host.py).

Before a number is compared the handle says which door it is ("sparse_weighted", "matrix_absent_missing") and how many workers the sums
are split over ("sp_workers", against the restated nnlm_sp_workers: with the rank's KP it fixes LW).

Bars.  The sum of squares of "ones" and "planted" is an integer every kernel forms without rounding, and nnlm_errors divides it ONCE by
n_non_missing: mse == float(S) / N TO THE BIT in both modes and through all four doors.  What rounds -- the KL part everywhere, mse of
"uniform" -- is held as |gpu - ref| / (sum |term| / N) below 1e-10 (strict) and 1e-5 (fp32 operands), the bars of
tests/test_gpu_error_block.py.  Two calls of errors() give identical bits.  Each test prints its largest deviations (`pytest -s`, lines
"SPERRDEV"); the largest per door and mode are in DESIGN.md 4.23."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import err_cases as ec  # noqa: E402
import sparse_cases as spc  # noqa: E402
import sparse_err_cases as se  # noqa: E402
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = [("f64", _lib.PREC_F64, 1e-10), ("f32", _lib.PREC_F32, 1e-5)]


@pytest.fixture(autouse=True)
def _default_precision(monkeypatch):
    monkeypatch.delenv("NNLM_PRECISION", raising=False)


def shape_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else None


def errors_of(prec, door, c, k, w):
    """(mse, KL part) of errors() on a fresh handle, called twice."""
    S = c["S"]
    with nnlm_amd.Handle(0, prec) as h:
        if se.WEIGHTED[door]:
            h.set_matrix_csc_weighted(S[0], S[1], S[2], w, S[3], absent_missing=se.ABSENT[door] == "missing")
        elif door == "missing":
            h.set_matrix_csc_missing(*S)
        else:
            h.set_matrix_csc(*S)
        h.set_factors(k, c["W"], c["H"])
        assert h.get_info("sparse_weighted") == float(se.WEIGHTED[door]) and h.get_info("matrix_absent_missing") == float(se.ABSENT[door] == "missing")
        assert int(h.get_info("sp_workers")) == spc.sp_workers(S[2].size, spc.kp_of(k), int(h.get_info("cus"))), (door, k)
        assert h.matrix_info()["n_non_missing"] == se.n_observed(c, door)
        first, again = h.errors(), h.errors()
        assert first[0] == again[0] and first[1] == again[1] and np.array_equal(first[2], again[2]), (door, k, first, again)
    return first[0], first[1]


@pytest.mark.parametrize("pname,prec,bar", MODES)
@pytest.mark.parametrize("shape,k", se.groups(), ids=shape_id)
def test_sparse_error_block_on_known_factors(shape, k, pname, prec, bar):
    worst = collections.defaultdict(float)
    n, m = shape
    for family in se.FAMILIES:
        case = se.Case(family, n, m, k)
        c = se.make_case(*case)
        for door in se.DOORS:
            if not se.accepts(door, k):
                continue
            r = se.ref_of(case, door)
            mse, kl = errors_of(prec, door, c, k, se.weights_of(c, door, family))
            form = se.form_of(pname, door, k)
            if family in se.EXACT:
                want = float(se.exact_sum(c, door, family)) / r.N
                print(f"SPERRDEV {family} {n}x{m} k={k} {pname} {door}: mse {mse!r} want {want!r}")
                assert mse == want, (case, door, form, mse, want, (mse - want) * r.N)   # (last: in units of the sum)
            else:
                d2 = ec.dev(mse, r.s2, r.abs2, r.N)
                worst[(door, "mse")] = max(worst[(door, "mse")], d2)
                assert d2 < bar, (case, door, form, d2, mse)
            dk = ec.dev(kl, r.kl, r.abskl, r.N)
            key = (door, "kl " + ("exact" if family in se.EXACT else family))
            worst[key] = max(worst[key], dk)
            assert dk < bar, (case, door, form, dk, kl)
    print(f"SPERRDEV worst {shape_id(shape)} k={k} {pname}: " + ", ".join(f"{' '.join(key)} {v:.3e}" for key, v in sorted(worst.items())))
