"""A sparse matrix AND its per-entry weights that already live in device memory (nnlm_set_matrix_sparse_device_weighted,
k_sparse_ingest.h) on the MI355X.  The yardstick is what nnlm_set_matrix_csc_weighted leaves resident for the fp64 widening of the same
values and weights: the ten arrays are compared with np.array_equal -- against the host entry's own arrays on a second handle and against
numpy's restatement (stable argsort; c a formed in fp64, then rounded to the mode's type) --, and fits from the same explicit init are
compared BIT FOR BIT in both arithmetic modes.  Every test calls the new entry.  Run with `pytest -m gpu`.

Bounds: kl_const differs from the host's by summation order and the device's log only: 1e-12 relative, the allowance this quantity has on
the unweighted device route (test_gpu_sparse_device.py); the mkl trace carries kl_const and inherits it.  rel_tol = -1 in every fit: the
stopping rule cannot fire.  With no stored entry and absent = missing both routes give 0 / 0 = NaN for kl_const, which counts as equal."""
import ctypes
import os
from itertools import product
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nnlm_amd  # noqa: E402
import sparse_device_cases as sdc  # noqa: E402
import sparse_device_weighted_cases as swc  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MODES = [("f64", _lib.PREC_F64), ("f32", _lib.PREC_F32)]
ERR_ARG, ERR_UNSUPPORTED = 1, 5
WHO = "nnlm_set_matrix_sparse_device_weighted"
HOST = "nnlm_set_matrix_csc_weighted"
INFO_KEYS = ("matrix_nnz", "matrix_bytes", "matrix_absent_missing", "sparse_weighted")
_const = {}
_cases = {}


@pytest.fixture(autouse=True)
def _default_precision(monkeypatch):
    monkeypatch.delenv("NNLM_PRECISION", raising=False)


def constants():
    if not _const:
        with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
            _const["v"] = (int(h.get_info("sp_ingest_check_share")), int(h.get_info("sp_ingest_sort_tile")))
        assert _const["v"] == sdc.header_constants()
    return _const["v"]


def case(name):
    """(S, weights) of a case: built once, shared, never written."""
    if name not in _cases:
        S = sdc.build(name, *constants())
        w = swc.weights(name, S[1].size)
        for a in (*S[:3], w):
            a.setflags(write=False)
        _cases[name] = (S, w)
    return _cases[name]


def dev():
    return torch.device("cuda", 0)


def put(a, dtype):
    return torch.from_numpy(np.array(a)).to(getattr(torch, dtype)).to(dev())  # (a copy: the shared cases are read-only)


def widened(t):
    return t.to(torch.float64).cpu().numpy()


def given(S, w, layout):
    """(ptr, idx, val, weights, shape) of the matrix of the CSC S in `layout`, the weights in that layout's order."""
    if layout == "csc":
        return S[0], S[1], S[2], w, S[3]
    rptr, cidx, rval = sdc.other_side(S)
    return rptr, cidx, rval, w[swc.order_of_other_side(S)], S[3]


def ingest(h, S, w, layout="csc", absent="missing", pt="int64", it="int64", vt="float64", wt="float64", pattern=None, stream=None):
    """The device entry; pattern = (ptr dtype, idx dtype): the weights come as a sparse matrix of their own.  -> the fp64 widening of the
    weights as the device saw them, in CSC order."""
    ptr, idx, val, wl, shape = given(S, w, layout)
    tw = put(wl, wt)
    weights = tw if pattern is None else (put(ptr, pattern[0]), put(idx, pattern[1]), tw)
    h.set_matrix_sparse_device_weighted(put(ptr, pt), put(idx, it), put(val, vt), weights, shape, layout, absent=absent, stream=stream)
    w64 = widened(tw)
    if layout == "csr":
        back = np.empty_like(w64)
        back[swc.order_of_other_side(S)] = w64
        w64 = back
    return w64


def host_ingest(h, S, w, absent):
    h.set_matrix_csc_weighted(S[0], S[1], S[2], w, S[3], absent_missing=absent == "missing")


def all_resident(h):
    return [h.debug_sparse_resident(side) + h.debug_sparse_resident_weighted(side) for side in (0, 1)]


def same_arrays(got, want, tag):
    for side in (0, 1):
        for g, w, what in zip(got[side], want[side], ("ptr", "idx", "val", "weights", "weights * val")):
            assert g.dtype == w.dtype and np.array_equal(g, w), (tag, side, what)


def same_number(a, b, rtol):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= rtol * abs(b)


def check_resident(name, layout, absent, prec, tag, **kw):
    """Device ingest against numpy and against the host entry: the ten arrays, the matrix facts, the info keys."""
    S, w = case(name)
    n, m = S[3]
    with nnlm_amd.Handle(0, prec) as hd, nnlm_amd.Handle(0, prec) as hh:
        w64 = ingest(hd, S, w, layout, absent, **kw)
        host_ingest(hh, S, w64, absent)
        got = all_resident(hd)
        same_arrays(got, swc.resident(S, w64, prec == _lib.PREC_F64), (tag, "numpy"))
        same_arrays(got, all_resident(hh), (tag, "host"))
        id_, ih = hd.matrix_info(), hh.matrix_info()
        assert id_["n_non_missing"] == ih["n_non_missing"] and id_["any_missing"] == ih["any_missing"], tag
        assert same_number(id_["kl_const"], ih["kl_const"], 1e-12), (tag, id_["kl_const"], ih["kl_const"])
        for key in INFO_KEYS:
            assert hd.get_info(key) == hh.get_info(key), (tag, key)
        assert hd.get_info("sparse_weighted") == 1
        want_min = (int(np.diff(S[0]).min()), int(np.diff(sdc.other_side(S)[0]).min())) if absent == "missing" else (n, m)
        assert (hd.get_info("matrix_min_col_observed"), hd.get_info("matrix_min_row_observed")) == want_min, tag


def names(big):
    return [c for c in swc.case_names(*sdc.header_constants()) if sdc.big(c) == big and c != "fit_heavy_long"]


# ---- 1. resident arrays -------------------------------------------------------------------------------------------------------------------
# (One test per property, the cases in loops inside it: every case is a few milliseconds of GPU work, and the failing case is named by the
# tag of the assertion.  The suite's list of tests grows by a dozen entries, not by one per case.)
def test_resident_arrays():
    """Every case of the table x both absent semantics x both layouts.  The many-line cases are the two- and three-pass sorts with three
    payloads (as CSR the given side is the long one and the sort has one pass; as CSC the built side is the long one)."""
    for (mode, prec), absent, layout in product(MODES, swc.ABSENT, sdc.LAYOUTS):
        for name in names(False) + ["fit_heavy_long"]:
            check_resident(name, layout, absent, prec, (name, layout, mode, absent))
        for name in names(True):
            check_resident(name, layout, absent, prec, (name, layout, mode, absent), it="int32", vt="float32", wt="float32")


# ---- 2. every dtype and layout combination ------------------------------------------------------------------------------------------------
def test_every_layout_dtype_combination():
    for (mode, prec), layout, pt, it, vt, wt in product(MODES, sdc.LAYOUTS, sdc.INT_DTYPES, sdc.INT_DTYPES, sdc.VAL_DTYPES, swc.WEIGHT_DTYPES):
        check_resident("small", layout, "missing", prec, (layout, pt, it, vt, wt, mode), pt=pt, it=it, vt=vt, wt=wt)


def test_csr_equals_csc():
    for name, absent in [(c, a) for c in ("small", "powerlaw", "dominant_line", "lines_257") for a in swc.ABSENT]:
        S, w = case(name)
        with nnlm_amd.Handle(0, _lib.PREC_F32) as ha, nnlm_amd.Handle(0, _lib.PREC_F32) as hb:
            ingest(ha, S, w, "csc", absent, wt="float32")
            ingest(hb, S, w, "csr", absent, pt="int32", it="int32", vt="float16", wt="float32")
            same_arrays(all_resident(ha), all_resident(hb), (name, absent))
            assert ha.get_info("matrix_bytes") == hb.get_info("matrix_bytes")


# ---- 3. weights as a sparse matrix ----------------------------------------------------------------------------------------------------------
def test_weights_as_a_sparse_matrix():
    for layout in sdc.LAYOUTS:
        _weights_as_a_sparse_matrix(layout)
        _weights_of_another_pattern_are_refused(layout)


def _weights_as_a_sparse_matrix(layout):
    S, w = case("powerlaw")
    with nnlm_amd.Handle(0, _lib.PREC_F32) as ha:
        ingest(ha, S, w, layout, "zero", pt="int64", it="int64")
        want = all_resident(ha)
        info = [ha.get_info(k) for k in INFO_KEYS]
    for pattern in (("int32", "int32"), ("int64", "int32"), ("int32", "int64")):
        with nnlm_amd.Handle(0, _lib.PREC_F32) as hb:
            ingest(hb, S, w, layout, "zero", pt="int64", it="int64", pattern=pattern, wt="float32")
            got = all_resident(hb)
            w32 = w.astype(np.float32).astype(np.float64)  # (fp32 weights: the arrays of the aligned form for those values)
            same_arrays(got, swc.resident(S, w32, False), (layout, pattern, "numpy"))
            assert [hb.get_info(k) for k in INFO_KEYS] == info
    with nnlm_amd.Handle(0, _lib.PREC_F32) as hb:  # the same dtypes throughout: equal to the aligned form
        ingest(hb, S, w, layout, "zero", pt="int64", it="int64", pattern=("int64", "int64"))
        same_arrays(all_resident(hb), want, (layout, "aligned"))


def _weights_of_another_pattern_are_refused(layout):
    S, w = case("powerlaw")
    keep, wk = case("small")
    G = S if layout == "csc" else sdc.transposed(S)  # (the arrays given; as CSR they describe the same matrix by rows)
    ptr, idx, val, _ = G
    shape = S[3]
    line = "column" if layout == "csc" else "row"
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
        ingest(h, keep, wk)
        before = all_resident(h)
        tp, ti, tv = put(ptr, "int64"), put(idx, "int32"), put(val, "float64")
        for what, ((p2, i2), nnz2, first) in swc.pattern_changes(G).items():
            wts = (put(p2, "int32"), put(i2, "int64"), put(np.ones(nnz2), "float32"))
            with pytest.raises(_lib.NnlmError) as e:
                h.set_matrix_sparse_device_weighted(tp, ti, tv, wts, shape, layout)
            assert e.value.code == ERR_ARG, what
            assert str(e.value).endswith("%s: the stored pattern of weights differs from the matrix's (first in %s %d)" % (WHO, line, first)), (what, e.value)
            assert h.matrix_info()["n_non_missing"] == keep[1].size and h.get_info("matrix_nnz") == keep[1].size, what
            same_arrays(all_resident(h), before, (what, "the earlier matrix"))


# ---- 4. fits --------------------------------------------------------------------------------------------------------------------------------
def start(n, m, k, seed):
    rng = np.random.default_rng(seed)
    return 0.01 * rng.random((n, k)) + 0.01, 0.01 * rng.random((k, m)) + 0.01


def fit(h, n, m, method, k, iters=3):
    z = [0, 0, 0]
    W0, H0 = start(n, m, k, 5)
    h.set_factors(k, W0, H0)
    t = h.run(z, z, iters, -1.0, 0, False, 10, 1e-9, method, 1)
    return h.get_factors(), t


def same_fit(a, b, tag):
    ((Wa, Ha), x), ((Wb, Hb), y) = a, b
    assert np.array_equal(Wa, Wb) and np.array_equal(Ha, Hb), tag
    assert x["n_iteration"] == y["n_iteration"] and np.array_equal(x["mse_error"], y["mse_error"]), tag
    assert np.array_equal(x["average_epoch"], y["average_epoch"]) and np.array_equal(x["target_error"], y["target_error"]), tag
    np.testing.assert_allclose(x["mkl_error"], y["mkl_error"], rtol=1e-12, atol=0, err_msg=str(tag))  # (carries kl_const)


def test_fits_bit_for_bit():
    for (method, name, k), absent, (mode, prec) in product([(1, "fit_heavy", 3), (2, "fit_heavy", 17), (1, "fit_heavy_long", 5), (2, "small", 3)],
                                                           swc.ABSENT, MODES):
        _fit_bit_for_bit(method, name, k, absent, mode, prec)


def _fit_bit_for_bit(method, name, k, absent, mode, prec):
    S, w = case(name)
    n, m = S[3]
    layout = "csr" if method == 2 else "csc"
    with nnlm_amd.Handle(0, prec) as hd, nnlm_amd.Handle(0, prec) as hh:
        w64 = ingest(hd, S, w, layout, absent, it="int32", vt="float32", wt="float32")
        host_ingest(hh, S, w64, absent)
        same_fit(fit(hd, n, m, method, k), fit(hh, n, m, method, k), (method, name, absent, mode))


def test_unit_weights_equal_the_unweighted_missing_door():
    for (method, name), (mode, prec) in product([(1, "fit_heavy"), (2, "fit_heavy_long")], MODES):
        _unit_weights_equal_the_unweighted_missing_door(method, name, mode, prec)


def _unit_weights_equal_the_unweighted_missing_door(method, name, mode, prec):
    S, _ = case(name)
    n, m = S[3]
    with nnlm_amd.Handle(0, prec) as hw, nnlm_amd.Handle(0, prec) as hu:
        ingest(hw, S, np.ones(S[1].size), "csc", "missing", wt="bfloat16")
        hu.set_matrix_sparse_device(put(S[0], "int64"), put(S[1], "int64"), put(S[2], "float64"), S[3], "csc", absent="missing")
        same_fit(fit(hw, n, m, method, 4), fit(hu, n, m, method, 4), (method, name, mode))


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------
def swap_words(msg):
    return re.sub(r"\b(row|column|colptr)\b", lambda w: {"row": "column", "column": "row", "colptr": "rowptr"}[w.group(1)], msg)


def swap_entry(msg):
    """The weight message names the entry's own row and column: the same arrays given as CSR trade the two numbers."""
    return re.sub(r"\(row (\d+), column (\d+)\)", r"(row \2, column \1)", msg)


def error_of(fn):
    with pytest.raises(_lib.NnlmError) as e:
        fn()
    return e.value.code, str(e.value)


def test_refusals_of_weights():
    for (mode, prec), layout in product(MODES, sdc.LAYOUTS):
        _refusals_of_weights(mode, prec, layout)


def _refusals_of_weights(mode, prec, layout):
    """The arrays of the base case are given as CSC of the (n, m) matrix or, unchanged, as CSR of the (m, n) one: the entry numbers are the
    same, so the host entry's message for the CSC is the yardstick for both."""
    share, _ = constants()
    (ptr, idx, val, shape), w = case("nnz_%d" % (2 * share + 1))
    keep, wk = case("small")
    dshape = shape if layout == "csc" else shape[::-1]
    with nnlm_amd.Handle(0, prec) as hd, nnlm_amd.Handle(0, prec) as hh:
        ingest(hd, keep, wk)
        before = all_resident(hd)
        tp, ti, tv = put(ptr, "int64"), put(idx, "int32"), put(val, "float64")

        def both(v, wbad, tv_=None):
            tvv = tv if tv_ is None else tv_
            code, msg = error_of(lambda: hd.set_matrix_sparse_device_weighted(tp, ti, tvv, put(wbad, "float64"), dshape, layout))
            hcode, hmsg = error_of(lambda: hh.set_matrix_csc_weighted(ptr, idx, v, wbad, shape))
            return code, msg, hcode, hmsg.replace(HOST, WHO)

        for where, e in swc.offence_positions(idx.size, share).items():
            for what, value in swc.OFFENCES.items():
                code, msg, hcode, hmsg = both(val, swc.with_weight(w, e, value))
                assert code == hcode == ERR_ARG, (where, what, msg)
                assert "weight" in msg and "entry %d " % e in msg, msg
                assert msg == (hmsg if layout == "csc" else swap_entry(hmsg)), (where, what, msg, hmsg)
                same_arrays(all_resident(hd), before, (where, what, "the earlier matrix"))
            for what, value in swc.LEGAL.items():
                with nnlm_amd.Handle(0, prec) as h2:
                    h2.set_matrix_sparse_device_weighted(tp, ti, tv, put(swc.with_weight(w, e, value), "float64"), dshape, layout)
                    assert h2.get_info("sparse_weighted") == 1
        # two weight offences in different blocks: the earlier one is named
        two = swc.with_weight(swc.with_weight(w, share + 9, -1.0), 40, np.inf)
        code, msg, hcode, hmsg = both(val, two)
        assert "entry 40 " in msg and msg == (hmsg if layout == "csc" else swap_entry(hmsg)), msg
        # an offence of A at a later entry outranks a weight offence at an earlier one
        vbad = val.copy()
        vbad[idx.size - 2] = np.nan
        code, msg, hcode, hmsg = both(vbad, swc.with_weight(w, 3, np.nan), put(vbad, "float64"))
        assert code == hcode == ERR_ARG and "is not finite" in msg and "entry %d " % (idx.size - 2) in msg, msg
        assert msg == (hmsg if layout == "csc" else swap_words(hmsg)), (msg, hmsg)
        same_arrays(all_resident(hd), before, "the earlier matrix")


def test_refusals_of_the_fp32_range_rules():
    S, w = case("small")
    ptr, idx, _, shape = S
    for what, (v, c, text) in swc.range_rule_inputs(S).items():
        with nnlm_amd.Handle(0, _lib.PREC_F32) as hd, nnlm_amd.Handle(0, _lib.PREC_F32) as hh:
            ingest(hd, S, w)
            before = all_resident(hd)
            code, msg = error_of(lambda: hd.set_matrix_sparse_device_weighted(put(ptr, "int64"), put(idx, "int64"), put(v, "float64"),
                                                                              put(c, "float64"), shape))
            hcode, hmsg = error_of(lambda: hh.set_matrix_csc_weighted(ptr, idx, v, c, shape))
            assert code == hcode == ERR_UNSUPPORTED and msg == hmsg and text in msg, (what, msg, hmsg)
            same_arrays(all_resident(hd), before, (what, "kept"))
        with nnlm_amd.Handle(0, _lib.PREC_F64) as hd:  # (the strict mode takes all three)
            hd.set_matrix_sparse_device_weighted(put(ptr, "int64"), put(idx, "int64"), put(v, "float64"), put(c, "float64"), shape)
            assert np.array_equal(hd.debug_sparse_resident_weighted(0)[1], c * v), what


def test_refusals_of_arguments():
    S, w = case("small")
    ptr, idx, val, (n, m) = S
    tp, ti, tv, tw = put(ptr, "int64"), put(idx, "int32"), put(val, "float64"), put(w, "float64")
    lib = _lib.load()

    def call(h, a, wt):
        h._ck(lib.nnlm_set_matrix_sparse_device_weighted(h._h, ctypes.byref(a), None if wt is None else ctypes.byref(wt), n, m, 1, None))

    def desc(**kw):
        f = dict(ptr=tp.data_ptr(), idx=ti.data_ptr(), val=tv.data_ptr(), ptr_dtype=_lib.IT_I64, idx_dtype=_lib.IT_I32, val_dtype=_lib.DT_F64,
                 layout=_lib.SP_CSC, nnz=idx.size)
        f.update(kw)
        return _lib.DevSparse(**f)

    def wdesc(**kw):  # the aligned form unless ptr and idx are given
        f = dict(ptr=None, idx=None, val=tw.data_ptr())
        f.update(kw)
        return desc(**f)

    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
        ingest(h, S, w)
        before = all_resident(h)
        own = int(h.get_info("debug_sparse_values_address"))
        assert own > 0
        for wt, word in ((None, "Wt is NULL"), (wdesc(val=None), "Wt.val is NULL"), (wdesc(ptr=tp.data_ptr()), "both be NULL"),
                         (wdesc(idx=ti.data_ptr()), "both be NULL"), (wdesc(ptr=tp.data_ptr(), idx=ti.data_ptr(), layout=_lib.SP_CSR), "Wt.layout"),
                         (wdesc(nnz=idx.size - 1), "Wt.nnz"), (wdesc(nnz=-1), "negative"), (wdesc(val_dtype=4), "Wt.val_dtype"),
                         (wdesc(ptr=tp.data_ptr(), idx=ti.data_ptr(), ptr_dtype=2), "Wt.ptr_dtype"),
                         (wdesc(val=w.ctypes.data), "Wt.val is not device"),
                         (wdesc(ptr=ptr.ctypes.data, idx=ti.data_ptr()), "Wt.ptr is not device"),
                         (wdesc(val=own), "Wt.val aliases a buffer of the handle itself"),
                         (wdesc(nnz=idx.size + 10 ** 7, ptr=tp.data_ptr(), idx=ti.data_ptr()), "past the end of its allocation")):
            code, msg = error_of(lambda: call(h, desc(), wt))
            assert code == ERR_ARG and word in msg and WHO in msg, (word, msg)
        code, msg = error_of(lambda: call(h, desc(val_dtype=7), wdesc()))  # (A's own descriptor: the unweighted entry's refusals)
        assert code == ERR_ARG and "A.val_dtype" in msg and WHO in msg
        same_arrays(all_resident(h), before, "kept")
        for bad, match in ((torch.from_numpy(np.array(w)), "host memory"), (tw[:-1], "weights has %d entries, val has %d" % (idx.size - 1, idx.size)),
                           (put(np.arange(idx.size), "int64"), "float64, float32"), (tw.reshape(1, -1), "1-D"),
                           ((tp, ti), "triple")):
            with pytest.raises(ValueError, match=match):
                h.set_matrix_sparse_device_weighted(tp, ti, tv, bad, (n, m))
        same_arrays(all_resident(h), before, "kept")
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:  # the hook on handles without weights
        assert error_of(lambda: h.debug_sparse_resident_weighted(0))[0] == ERR_ARG
        h.set_matrix_csc(ptr, idx, val, (n, m))
        code, msg = error_of(lambda: h.debug_sparse_resident_weighted(0))
        assert code == ERR_ARG and "per-entry weights" in msg
    with nnlm_amd.Handle(0, _lib.PREC_F64) as hd, nnlm_amd.Handle(0, _lib.PREC_F64) as hh:  # a sharded handle: the host entry's refusal
        for h in (hd, hh):
            h.comm_init(None, 0, 2)
        code, msg = error_of(lambda: ingest(hd, S, w))
        hcode, hmsg = error_of(lambda: host_ingest(hh, S, w, "missing"))
        assert code == hcode == ERR_UNSUPPORTED and msg == hmsg.replace(HOST, WHO), (msg, hmsg)


# ---- 6. stream order --------------------------------------------------------------------------------------------------------------------------
def test_weights_produced_on_another_stream():
    S, w = case("nnz_%d" % (2 * constants()[0] + 1))
    ptr, idx, val, shape = S
    hp, hi, hv, hw = (torch.from_numpy(np.array(a)).pin_memory() for a in (ptr, idx.astype(np.int64), val, w))
    s = torch.cuda.Stream(device=dev())
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
        with torch.cuda.stream(s):
            busy = torch.ones((2048, 2048), device=dev())
            for _ in range(20):  # work queued ahead of the copies: the weights do not exist yet when the ingest is called
                busy = busy @ busy * 1e-4
            tp, ti, tv, tw = (a.to(dev(), non_blocking=True) for a in (hp, hi, hv, hw))
            tw = tw * 2.0
            h.set_matrix_sparse_device_weighted(tp, ti, tv, tw, shape, "csc", stream=s)
        same_arrays(all_resident(h), swc.resident(S, 2.0 * w, True), "stream")
        with torch.cuda.stream(s):  # the current stream of the tensors' device is taken when none is named
            tw2 = tw * 0.5
            h.set_matrix_sparse_device_weighted(tp, ti, tv, (tp, ti, tw2), shape, "csc")
        same_arrays(all_resident(h), swc.resident(S, w, True), "current stream")
    torch.cuda.synchronize()


# ---- 7. api -------------------------------------------------------------------------------------------------------------------------------------
class Csc:
    """numpy-only duck-typed host sparse matrix (canonical CSC given directly)."""

    def __init__(self, S):
        self.indptr, self.indices, self.data, self.shape = S

    def tocsc(self):
        return self


def sparse_tensor(S, w, layout, it="int64", vt="float64"):
    """The sparse tensor of S in `layout`, the aligned weights (1-D tensor) and the weights as a sparse tensor of the same pattern."""
    ptr, idx, val, wl, shape = given(S, w, layout)
    make = torch.sparse_csc_tensor if layout == "csc" else torch.sparse_csr_tensor
    A = make(put(ptr, it), put(idx, it), put(val, vt), size=shape, device=dev())
    Wt = make(put(ptr, "int32"), put(idx, "int32"), put(wl, "float64"), size=shape, device=dev())
    return A, put(wl, "float64"), Wt


@pytest.mark.filterwarnings("ignore")
def test_api_nnmf():
    for form, absent, layout in product(["aligned", "sparse"], swc.ABSENT, sdc.LAYOUTS):
        _api_nnmf(form, absent, layout)


def _api_nnmf(form, absent, layout):
    S, w = case("powerlaw")
    A, w1, Wt = sparse_tensor(S, w, layout, "int32" if layout == "csr" else "int64", "float32")
    opts = dict(k=3, max_iter=6, rel_tol=-1.0, check_k=False, absent=absent)
    rd = api.nnmf(A, rng=np.random.default_rng(11), weights=w1 if form == "aligned" else Wt, **opts)
    rh = api.nnmf(Csc(S), rng=np.random.default_rng(11), weights=np.array(w), **opts)
    assert isinstance(rd["W"], torch.Tensor) and rd["W"].device == A.device and rd["W"].dtype == torch.float64
    assert isinstance(rd["H"], torch.Tensor) and rd["H"].device == A.device
    assert np.array_equal(rd["W"].cpu().numpy(), rh["W"]) and np.array_equal(rd["H"].cpu().numpy(), rh["H"])
    assert np.array_equal(rd["mse"], rh["mse"]) and rd["n_iteration"] == rh["n_iteration"]
    np.testing.assert_allclose(rd["mkl"], rh["mkl"], rtol=1e-12, atol=0)
    assert rd["options"]["absent"] == rh["options"]["absent"] == absent
    if form == "aligned" and layout == "csc":  # scores from the fit: the host entries take the factors as host arrays
        fitted = {"W": rd["W"].cpu().numpy(), "H": rd["H"].cpu().numpy()}
        i1, s1 = api.top_n(fitted, 4, seen=Csc(S))
        i2, s2 = api.top_n(rh, 4, seen=Csc(S))
        assert np.array_equal(i1, i2) and np.array_equal(s1, s2)
        rows, cols = S[1][:20], np.repeat(np.arange(S[3][1]), np.diff(S[0]))[:20]
        assert np.array_equal(api.predict_entries(fitted, rows, cols), api.predict_entries(rh, rows, cols))


@pytest.mark.filterwarnings("ignore")
def test_api_nnmf_refusals():
    S, w = case("small")
    A, w1, Wt = sparse_tensor(S, w, "csc")
    Ar, w1r, Wtr = sparse_tensor(S, w, "csr")
    ok = api.nnmf(A, 2, weights=w1, max_iter=2, rel_tol=-1.0, rng=np.random.default_rng(1))
    assert ok["W"].shape == (S[3][0], 2)
    fitted = api.nnmf(Csc(S), 2, weights=np.array(w), max_iter=2, rel_tol=-1.0, rng=np.random.default_rng(1))  # (a fit with host factors)
    assert np.array_equal(ok["W"].cpu().numpy(), fitted["W"])
    # new refusals
    with pytest.raises(api.NnlmStop, match="weights live in device memory, but A is a host matrix"):
        api.nnmf(Csc(S), 2, weights=w1)
    with pytest.raises(api.NnlmStop, match="weights live in device memory, but A is a host matrix"):
        api.nnmf(Csc(S), 2, weights=Wt)
    with pytest.raises(api.NnlmStop, match="weights is a sparse CSR tensor, the matrix a sparse CSC tensor"):
        api.nnmf(A, 2, weights=Wtr)
    T = sdc.transposed(S)
    with pytest.raises(api.NnlmStop, match=r"weights is %d x %d, the matrix %d x %d" % (T[3] + S[3])):
        api.nnmf(A, 2, weights=sparse_tensor(T, np.ones(T[1].size), "csc")[2])
    with pytest.raises(api.NnlmStop, match=r"weights: a device tensor of layout torch.sparse_coo"):
        api.nnmf(A, 2, weights=Wt.to_sparse_coo())
    with pytest.raises(api.NnlmStop, match="weights has %d entries, val has %d" % (w.size - 1, w.size)):
        api.nnmf(A, 2, weights=w1[:-1])
    # kept refusals
    with pytest.raises(api.NnlmStop, match="weights cannot be combined with a A in device memory"):
        api.nnmf(A, 2, weights=np.array(w))
    with pytest.raises(api.NnlmStop, match="weights cannot be combined with a A in device memory"):
        api.nnmf(put(np.ones(S[3]), "float64"), 2, weights=w1)
    with pytest.raises(api.NnlmStop, match="weights cannot be combined with a y in device memory"):
        api.nnlm(np.ones((S[3][0], 2)), A, weights=w1)
    with pytest.raises(api.NnlmStop, match="loss = 'mse' only"):
        api.nnmf(A, 2, weights=w1, loss="mkl")
    with pytest.raises(api.NnlmStop, match="loss = 'mse' only"):
        api.nnmf(A, 2, weights=w1, sparse_kl=True)
    with pytest.raises(api.NnlmStop, match="cannot be combined with init = 'nndsvd'"):
        api.nnmf(A, 2, weights=w1, init="nndsvd")
    for fn, who in ((lambda: api.nnmf_cv(A, [2]), "nnmf_cv: A"), (lambda: api.predict_nnmf(fitted, A, which="H"), "predict_nnmf: newdata"),
                    (lambda: api.top_n(fitted, 2, seen=A), "top_n: seen")):
        with pytest.raises(api.NnlmStop, match=who + " is a sparse tensor in device memory"):
            fn()
    with pytest.raises((api.NnlmStop, _lib.NnlmError, TypeError)):  # (the batch has no weights argument of its own)
        api.nnmf_batch(A, [2], sparse_batch=True, weights=w1)
    # the library's own refusals come through with its message
    with pytest.raises(_lib.NnlmError, match="is not a finite number >= 0"):
        api.nnmf(A, 2, weights=put(swc.with_weight(w, 3, -1.0), "float64"))
    changed = swc.pattern_changes(S)["index_changed"]
    other = torch.sparse_csc_tensor(put(changed[0][0], "int64"), put(changed[0][1], "int64"), put(w, "float64"), size=S[3], device=dev())
    with pytest.raises(_lib.NnlmError, match=r"the stored pattern of weights differs from the matrix's \(first in column %d\)" % changed[2]):
        api.nnmf(A, 2, weights=other)
