"""Sparse matrices that already live in device memory (nnlm_set_matrix_sparse_device, k_sparse_ingest.h) on the MI355X.  The yardstick
is what the matching host entry leaves resident for the fp64 widening of the same values: the six arrays are compared with
np.array_equal -- against numpy's stable-argsort transposition and against the host entry's own resident arrays --, and fits from the same
explicit init are compared BIT FOR BIT in both arithmetic modes.  Run with `pytest -m gpu`.

Bounds: kl_const differs from the host's by summation order only (per-block partial sums instead of one running sum): 1e-12 relative, the
project's bound for this quantity on such a route (test_gpu_device_io.py); the traces that carry kl_const (mkl; the target of the KL
methods) inherit it.  rel_tol = -1 in every fit: the stopping rule cannot fire, so that 1e-12 cannot move a stop.

matrix_min_row_observed / matrix_min_col_observed: a handle loaded from host arrays answers -1 (as it always has); the handle loaded
here answers from its host copies of the pointers, and is checked against numpy's counts."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nnlm_amd  # noqa: E402
import sparse_device_cases as sdc  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MODES = [("f64", _lib.PREC_F64), ("f32", _lib.PREC_F32)]
ERR_ARG, ERR_UNSUPPORTED = 1, 5
WHO = "nnlm_set_matrix_sparse_device"
_const = {}


@pytest.fixture(autouse=True)
def _default_precision(monkeypatch):
    monkeypatch.delenv("NNLM_PRECISION", raising=False)


def constants():
    """(share, tile): entries per workgroup of the entry check and of a radix pass, from the library."""
    if not _const:
        with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
            _const["v"] = (int(h.get_info("sp_ingest_check_share")), int(h.get_info("sp_ingest_sort_tile")))
        assert _const["v"] == sdc.header_constants()
    return _const["v"]


def case(name):
    return sdc.build(name, *constants())


def dev():
    return torch.device("cuda", 0)


def put(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(getattr(torch, dtype)).to(dev())


def given(S, layout):
    """(ptr, idx, val, shape) of the matrix of the CSC S in `layout`."""
    if layout == "csc":
        return S
    rptr, cidx, rval = sdc.other_side(S)
    return rptr, cidx, rval, S[3]


def ingest(h, S, layout="csc", door="plain", pt="int64", it="int64", vt="float64", stream=None):
    ptr, idx, val, shape = given(S, layout)
    absent, kl, batch = sdc.DOORS[door]
    h.set_matrix_sparse_device(put(ptr, pt), put(idx, it), put(val, vt), shape, layout, absent=absent, kl=kl, batch=batch, stream=stream)


def host_ingest(h, S, door="plain"):
    getattr(h, sdc.HOST_ENTRY[door])(S[0], S[1], S[2], S[3])


def mode_values(val, prec):
    return val if prec == _lib.PREC_F64 else val.astype(np.float32).astype(np.float64)


def same_arrays(got, want, tag):
    for g, w, what in zip(got, want, ("ptr", "idx", "val")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (tag, what)


INFO_KEYS = ("matrix_nnz", "matrix_bytes", "matrix_absent_missing", "sparse_kl", "sparse_batch", "sparse_kl_batch")


def check_resident(S, layout, door, prec, tag, **dtypes):
    """Device ingest against numpy and against the host entry: both sides, the matrix facts, the info keys."""
    ptr, idx, val, (n, m) = S
    rptr, cidx, rval = sdc.other_side(S)
    with nnlm_amd.Handle(0, prec) as hd, nnlm_amd.Handle(0, prec) as hh:
        ingest(hd, S, layout, door, **dtypes)
        host_ingest(hh, S, door)
        for side, want in ((0, (ptr, idx, mode_values(val, prec))), (1, (rptr, cidx, mode_values(rval, prec)))):
            got = hd.debug_sparse_resident(side)
            same_arrays(got, want, (tag, "numpy", side))
            same_arrays(got, hh.debug_sparse_resident(side), (tag, "host", side))
        id_, ih = hd.matrix_info(), hh.matrix_info()
        assert id_["n_non_missing"] == ih["n_non_missing"] and id_["any_missing"] == ih["any_missing"], tag
        assert abs(id_["kl_const"] - ih["kl_const"]) <= 1e-12 * abs(ih["kl_const"]), (tag, id_["kl_const"], ih["kl_const"])
        for key in INFO_KEYS:
            assert hd.get_info(key) == hh.get_info(key), (tag, key)
        if sdc.DOORS[door][0] == "missing":
            want_min = (int(np.diff(ptr).min()), int(np.diff(rptr).min()))
        else:
            want_min = (n, m)
        assert (hd.get_info("matrix_min_col_observed"), hd.get_info("matrix_min_row_observed")) == want_min, tag
        assert hh.get_info("matrix_min_col_observed") == -1  # (the host entry's handle: as before)


def small_names():
    return [c for c in sdc.case_names(*sdc.header_constants()) if not sdc.big(c) and c != "fit_heavy_long"]


# ---- 1. resident arrays -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,prec", MODES)
@pytest.mark.parametrize("name", small_names())
def test_resident_arrays(name, mode, prec):
    S = case(name)
    for layout in sdc.LAYOUTS:
        check_resident(S, layout, "plain", prec, (name, layout, mode))


@pytest.mark.parametrize("layout", sdc.LAYOUTS)
@pytest.mark.parametrize("name", [c for c in sdc.case_names(*sdc.header_constants()) if sdc.big(c)])
def test_resident_arrays_many_lines(name, layout):
    """The two-, three- and four-pass sorts: once per layout (as CSR the transposed matrix is given, so the built side is the long one)."""
    S = case(name)
    if layout == "csr":
        S = sdc.transposed(S)
    check_resident(S, layout, "plain", _lib.PREC_F64, (name, layout))


@pytest.mark.parametrize("mode,prec", MODES)
def test_every_layout_dtype_combination(mode, prec):
    S = case("small")
    for layout in sdc.LAYOUTS:
        for pt in sdc.INT_DTYPES:
            for it in sdc.INT_DTYPES:
                for vt in sdc.VAL_DTYPES:
                    check_resident(S, layout, "plain", prec, (layout, pt, it, vt, mode), pt=pt, it=it, vt=vt)


@pytest.mark.parametrize("mode,prec", MODES)
@pytest.mark.parametrize("door", list(sdc.DOORS))
def test_every_door(door, mode, prec):
    for name, layout, pt, it in (("small", "csc", "int64", "int32"), ("empty_lines", "csr", "int32", "int64"), ("fit_heavy", "csc", "int64", "int64")):
        check_resident(case(name), layout, door, prec, (name, door, mode), pt=pt, it=it, vt="float32")


# ---- 2. fits --------------------------------------------------------------------------------------------------------------------------------
def start(n, m, k, seed):
    rng = np.random.default_rng(seed)
    return 0.01 * rng.random((n, k)) + 0.01, 0.01 * rng.random((k, m)) + 0.01


def fit(h, n, m, door, method, seed=5, iters=4):
    """A fixed number of iterations from an explicit init; the stopping rule cannot fire (rel_tol = -1)."""
    z = [0, 0, 0]
    inner = 10 if method < 3 else 2
    if sdc.DOORS[door][2]:
        ks = [2, 3]
        starts = [start(n, m, k, seed + b) for b, k in enumerate(ks)]
        h.set_factors_batch(ks, [s[0] for s in starts], [s[1] for s in starts])
        traces = h.run_batch(z, z, iters, -1.0, 0, False, inner, 1e-9, method, 1)
        return h.get_factors_batch(), traces
    W0, H0 = start(n, m, 3, seed)
    h.set_factors(3, W0, H0)
    t = h.run(z, z, iters, -1.0, 0, False, inner, 1e-9, method, 1)
    return [h.get_factors()], [t]


def same_fit(a, b, tag, kl_target):
    (fa, ta), (fb, tb) = a, b
    for (Wa, Ha), (Wb, Hb) in zip(fa, fb):
        assert np.array_equal(Wa, Wb) and np.array_equal(Ha, Hb), tag
    for x, y in zip(ta, tb):
        assert x["n_iteration"] == y["n_iteration"] and np.array_equal(x["mse_error"], y["mse_error"]), tag
        assert np.array_equal(x["average_epoch"], y["average_epoch"]), tag
        np.testing.assert_allclose(x["mkl_error"], y["mkl_error"], rtol=1e-12, atol=0, err_msg=str(tag))  # (carries kl_const)
        if kl_target:
            np.testing.assert_allclose(x["target_error"], y["target_error"], rtol=1e-12, atol=0, err_msg=str(tag))
        else:
            assert np.array_equal(x["target_error"], y["target_error"]), tag


FITS = [("plain", 1, "fit_heavy"), ("plain", 2, "fit_heavy"), ("kl", 3, "fit_heavy"), ("kl", 4, "fit_heavy"), ("missing", 1, "fit_heavy_long"),
        ("batch", 1, "fit_heavy"), ("kl_batch", 3, "fit_heavy"), ("kl_batch", 4, "fit_heavy"), ("missing_batch", 1, "fit_heavy_long"),
        ("plain", 1, "small"), ("missing", 1, "small"), ("kl", 3, "small")]


@pytest.mark.parametrize("mode,prec", MODES)
@pytest.mark.parametrize("door,method,name", FITS)
def test_fits_bit_for_bit(door, method, name, mode, prec):
    S = case(name)
    n, m = S[3]
    layout = "csr" if method in (2, 4) else "csc"
    with nnlm_amd.Handle(0, prec) as hd, nnlm_amd.Handle(0, prec) as hh:
        ingest(hd, S, layout, door, it="int32", vt="float32")
        host_ingest(hh, S, door)
        same_fit(fit(hd, n, m, door, method), fit(hh, n, m, door, method), (door, method, name, mode), method >= 3)


# ---- 3. CSR == CSC ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "powerlaw", "dominant_line", "lines_257"])
def test_csr_equals_csc(name):
    S = case(name)
    for door in ("plain", "missing", "kl"):
        with nnlm_amd.Handle(0, _lib.PREC_F32) as ha, nnlm_amd.Handle(0, _lib.PREC_F32) as hb:
            ingest(ha, S, "csc", door)
            ingest(hb, S, "csr", door, pt="int32", it="int32", vt="float16")
            for side in (0, 1):
                same_arrays(ha.debug_sparse_resident(side), hb.debug_sparse_resident(side), (name, door, side))
            assert ha.get_info("matrix_bytes") == hb.get_info("matrix_bytes")


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------------------
def swap_words(msg):
    """The host entry's message for the transposed arrays -> the message for the same arrays given as CSR."""
    return re.sub(r"\b(row|column|colptr)\b", lambda w: {"row": "column", "column": "row", "colptr": "rowptr"}[w.group(1)], msg)


def error_of(fn):
    with pytest.raises(_lib.NnlmError) as e:
        fn()
    return e.value.code, str(e.value)


def malformed(S, share):
    """name -> (ptr, idx, val, shape, door): one offence each, placed by entry number; the base case spans three check blocks."""
    ptr, idx, val, shape = S
    nnz, n = idx.size, shape[0]
    assert nnz > 2 * share
    lens = np.diff(ptr)
    col_of = np.repeat(np.arange(shape[1]), lens)

    def second_of_a_line(lo):  # an entry >= lo that is not the first of its column
        e = lo
        while e == ptr[col_of[e]]:
            e += 1
        return e

    out = {}

    def add(name, door="plain", p=None, i=None, v=None, shp=None):
        out[name] = (ptr if p is None else p, idx if i is None else i, val if v is None else v, shape if shp is None else shp, door)

    p = ptr.copy()
    p[0] = 1
    add("ptr0", p=p)
    j = int(np.flatnonzero(lens[:-1] > 0)[3])
    p = ptr.copy()
    p[j] = ptr[j + 1] + 1  # column j starts beyond the start of column j + 1
    add("ptr_decreases", p=p)
    add("nnz_beyond_nm", p=np.array([0, 3, 5], dtype=np.int64), i=np.array([0, 1, 1, 0, 1], dtype=np.int32), v=np.ones(5), shp=(2, 2))

    def at(e, what, door="plain", base=None):
        i, v = (idx.copy(), val.copy()) if base is None else (base[0].copy(), base[1].copy())
        if what == "range":
            i[e] = n
        elif what == "negative_index":
            i[e] = -1
        elif what == "order":
            i[e] = i[e - 1]
        elif what == "nan":
            v[e] = np.nan
        elif what == "inf":
            v[e] = np.inf
        elif what == "negative":
            v[e] = -0.5
        return i, v

    e_mid = second_of_a_line(share + 7)
    for what in ("range", "negative_index", "order", "nan", "inf"):
        i, v = at(e_mid, what)
        add(what, i=i, v=v)
    i, v = at(e_mid, "nan")
    add("nan_missing", "missing", i=i, v=v)
    i, v = at(e_mid, "negative")
    add("negative_kl", "kl", i=i, v=v)
    add("negative_plain_is_fine", "plain", i=i, v=v)
    # two offenders of different kinds in different blocks: the earlier one is named
    a = at(100, "nan")
    i, v = at(share + 5, "range", base=a)
    add("nan_then_range", i=i, v=v)
    a = at(50, "range")
    i, v = at(nnz - 2, "nan", base=a)
    add("range_then_nan", i=i, v=v)
    a = at(second_of_a_line(nnz - 6), "order")
    i, v = at(second_of_a_line(share - 9), "negative", base=a)
    add("negative_then_order", "kl_batch", i=i, v=v)
    # the very first and the very last entry
    i, v = at(0, "nan")
    add("first_entry", i=i, v=v)
    i, v = at(nnz - 1, "range")
    add("last_entry", i=i, v=v)
    i, v = at(0, "range")
    add("first_entry_range", "missing_batch", i=i, v=v)
    i, v = at(nnz - 1, "inf")
    add("last_entry_inf", "batch", i=i, v=v)
    return out


def reference_fit(S, prec):
    with nnlm_amd.Handle(0, prec) as h:
        ingest(h, S)
        return fit(h, *S[3], "plain", 1)


@pytest.mark.parametrize("layout", sdc.LAYOUTS)
@pytest.mark.parametrize("mode,prec", MODES)
def test_refusals(mode, prec, layout):
    share, tile = constants()
    base = case("nnz_%d" % (2 * share + 1))
    keep = case("small")
    ref = reference_fit(keep, prec)
    with nnlm_amd.Handle(0, prec) as hd, nnlm_amd.Handle(0, prec) as hh:
        ingest(hd, keep)
        for name, (ptr, idx, val, shape, door) in malformed(base, share).items():
            absent, kl, batch = sdc.DOORS[door]
            dshape = shape if layout == "csc" else shape[::-1]  # (the same arrays as CSR describe the transposed matrix)

            def device():
                hd.set_matrix_sparse_device(put(ptr, "int64"), put(idx, "int32"), put(val, "float64"), dshape, layout, absent=absent, kl=kl,
                                            batch=batch)

            if name == "negative_plain_is_fine":
                with nnlm_amd.Handle(0, prec) as h2:
                    h2.set_matrix_sparse_device(put(ptr, "int64"), put(idx, "int32"), put(val, "float64"), dshape, layout)
                continue
            code, msg = error_of(device)
            hcode, hmsg = error_of(lambda: getattr(hh, sdc.HOST_ENTRY[door])(ptr, idx, val, shape))
            hmsg = hmsg.replace("nnlm_" + sdc.HOST_ENTRY[door], WHO)
            assert code == hcode == ERR_ARG, (name, msg, hmsg)
            assert msg == (hmsg if layout == "csc" else swap_words(hmsg)), (name, msg, hmsg)
            same_fit(fit(hd, *keep[3], "plain", 1), ref, (name, "the earlier matrix"), False)
            ingest_ok = hd.debug_sparse_resident(0)
            same_arrays(ingest_ok, (keep[0], keep[1], mode_values(keep[2], prec)), name)
        # ptr[last] != nnz: the caller states nnz here (the host entries read it from the array)
        ptr, idx, val, shape = base
        code, msg = error_of(lambda: hd.set_matrix_sparse_device(put(ptr, "int64"), put(np.append(idx, 0), "int32"), put(np.append(val, 1.0), "float64"),
                                                                 shape if layout == "csc" else shape[::-1], layout))
        lines = shape[1]
        pname = "colptr" if layout == "csc" else "rowptr"
        assert code == ERR_ARG and msg.endswith("%s: %s[%d] = %d, but A.nnz = %d" % (WHO, pname, lines, idx.size, idx.size + 1)), msg
        same_fit(fit(hd, *keep[3], "plain", 1), ref, "ptr[last]", False)


def test_refusals_of_the_fp32_range_rules():
    S = case("small")
    ptr, idx, val, shape = S
    big, tiny = val.copy(), np.full(val.size, 1e-35)
    big[val.size // 2] = 1e39
    for v in (big, tiny):
        with nnlm_amd.Handle(0, _lib.PREC_F32) as hd, nnlm_amd.Handle(0, _lib.PREC_F32) as hh:
            ingest(hd, S)
            code, msg = error_of(lambda: hd.set_matrix_sparse_device(put(ptr, "int64"), put(idx, "int64"), put(v, "float64"), shape, "csc"))
            hcode, hmsg = error_of(lambda: hh.set_matrix_csc(ptr, idx, v, shape))
            assert code == hcode == ERR_UNSUPPORTED and msg == hmsg, (msg, hmsg)
            same_arrays(hd.debug_sparse_resident(0), (ptr, idx, mode_values(val, _lib.PREC_F32)), "kept")
        with nnlm_amd.Handle(0, _lib.PREC_F64) as hd:  # (the strict mode takes both)
            hd.set_matrix_sparse_device(put(ptr, "int64"), put(idx, "int64"), put(v, "float64"), shape, "csc")
            assert np.array_equal(hd.debug_sparse_resident(0)[2], v)


def test_refusals_of_arguments():
    S = case("small")
    ptr, idx, val, (n, m) = S
    tp, ti, tv = put(ptr, "int64"), put(idx, "int32"), put(val, "float64")
    lib = _lib.load()

    def call(h, d, n_=n, m_=m, door=0):
        h._ck(lib.nnlm_set_matrix_sparse_device(h._h, ctypes.byref(d), n_, m_, door, None))

    def desc(**kw):
        f = dict(ptr=tp.data_ptr(), idx=ti.data_ptr(), val=tv.data_ptr(), ptr_dtype=_lib.IT_I64, idx_dtype=_lib.IT_I32, val_dtype=_lib.DT_F64,
                 layout=_lib.SP_CSC, nnz=idx.size)
        f.update(kw)
        return _lib.DevSparse(**f)

    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
        ingest(h, S)
        for d, kw, word in ((desc(ptr_dtype=2), {}, "ptr_dtype"), (desc(idx_dtype=-1), {}, "idx_dtype"), (desc(val_dtype=4), {}, "val_dtype"),
                            (desc(layout=2), {}, "layout"), (desc(), dict(door=8), "door"), (desc(), dict(door=3), "NNLM_SP_ABSENT_MISSING | NNLM_SP_KL"),
                            (desc(), dict(n_=0), "non-empty"), (desc(nnz=-1), {}, "negative"), (desc(idx=None), {}, "NULL"),
                            (desc(ptr=ptr.ctypes.data), {}, "A.ptr is not device"), (desc(val=val.ctypes.data), {}, "A.val is not device"),
                            (desc(nnz=idx.size + 10 ** 7), {}, "past the end of its allocation")):
            code, msg = error_of(lambda: call(h, d, **kw))
            assert code == ERR_ARG and word in msg and WHO in msg, (word, msg)
        same_arrays(h.debug_sparse_resident(0), (ptr, idx, val), "kept")
        with pytest.raises(ValueError, match="host memory"):
            h.set_matrix_sparse_device(torch.from_numpy(ptr), ti, tv, (n, m))
        assert h.debug_sparse_resident(1)[0].shape == (n + 1,)
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
        code, msg = error_of(lambda: h._ck(lib.nnlm_debug_sparse_resident(h._h, 0, None, None, None)))
        assert code == ERR_ARG and "no sparse matrix" in msg
        assert error_of(lambda: h.debug_sparse_resident(0))[0] == ERR_ARG
        h.set_matrix(np.ones((3, 2)))
        code, msg = error_of(lambda: h._ck(lib.nnlm_debug_sparse_resident(h._h, 0, None, None, None)))
        assert code == ERR_ARG
    with nnlm_amd.Handle(0, _lib.PREC_F64) as hd, nnlm_amd.Handle(0, _lib.PREC_F64) as hh:  # a sharded handle: the host entry's refusal
        for h in (hd, hh):
            h.comm_init(None, 0, 2)
        code, msg = error_of(lambda: ingest(hd, S))
        hcode, hmsg = error_of(lambda: host_ingest(hh, S))
        assert code == hcode == ERR_UNSUPPORTED and msg == hmsg.replace("nnlm_set_matrix_csc", WHO), (msg, hmsg)


# ---- 5. stream order --------------------------------------------------------------------------------------------------------------------------
def test_arrays_produced_on_another_stream():
    S = case("nnz_%d" % (2 * constants()[0] + 1))
    ptr, idx, val, shape = S
    hp, hi, hv = (torch.from_numpy(a).pin_memory() for a in (ptr, idx.astype(np.int64), val))
    s = torch.cuda.Stream(device=dev())
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
        with torch.cuda.stream(s):
            busy = torch.ones((2048, 2048), device=dev())
            for _ in range(20):  # work queued ahead of the copies: the arrays do not exist yet when the ingest is called
                busy = busy @ busy * 1e-4
            tp, ti, tv = (a.to(dev(), non_blocking=True) for a in (hp, hi, hv))
            tv = tv * 2.0
            h.set_matrix_sparse_device(tp, ti, tv, shape, "csc", stream=s)
        same_arrays(h.debug_sparse_resident(0), (ptr, idx, 2.0 * val), "stream")
        rptr, cidx, rval = sdc.other_side(S)
        same_arrays(h.debug_sparse_resident(1), (rptr, cidx, 2.0 * rval), "stream")
        with torch.cuda.stream(s):  # the current stream of the tensors' device is taken when none is named
            tv2 = tv * 0.5
            h.set_matrix_sparse_device(tp, ti, tv2, shape, "csc")
        same_arrays(h.debug_sparse_resident(0), (ptr, idx, val), "current stream")
    torch.cuda.synchronize()


# ---- 6. api -------------------------------------------------------------------------------------------------------------------------------------
class Csc:
    """numpy-only duck-typed host sparse matrix (canonical CSC given directly)."""

    def __init__(self, S):
        self.indptr, self.indices, self.data, self.shape = S

    def tocsc(self):
        return self


def sparse_tensor(S, layout, it="int64", vt="float64"):
    ptr, idx, val, shape = given(S, layout)
    make = torch.sparse_csc_tensor if layout == "csc" else torch.sparse_csr_tensor
    return make(put(ptr, it), put(idx, it), put(val, vt), size=shape, device=dev())


@pytest.mark.filterwarnings("ignore")
@pytest.mark.parametrize("layout", sdc.LAYOUTS)
@pytest.mark.parametrize("kw", [dict(absent="zero"), dict(absent="missing"), dict(sparse_kl=True, loss="mkl"), dict(absent="zero", method="lee")])
def test_api_nnmf(kw, layout):
    S = case("powerlaw")
    A = sparse_tensor(S, layout, "int32" if layout == "csr" else "int64", "float32")
    opts = dict(k=3, max_iter=6, rel_tol=-1.0, check_k=False, **kw)
    rd = api.nnmf(A, rng=np.random.default_rng(11), **opts)
    rh = api.nnmf(Csc(S), rng=np.random.default_rng(11), **opts)
    assert isinstance(rd["W"], torch.Tensor) and rd["W"].device == A.device and rd["W"].dtype == torch.float64
    assert isinstance(rd["H"], torch.Tensor) and rd["H"].device == A.device
    assert np.array_equal(rd["W"].cpu().numpy(), rh["W"]) and np.array_equal(rd["H"].cpu().numpy(), rh["H"])
    assert np.array_equal(rd["mse"], rh["mse"]) and rd["n_iteration"] == rh["n_iteration"]
    np.testing.assert_allclose(rd["mkl"], rh["mkl"], rtol=1e-12, atol=0)
    assert rd["options"]["absent"] == rh["options"]["absent"]


@pytest.mark.filterwarnings("ignore")
def test_api_nnmf_refusals_and_check_k():
    S = case("small")
    A = sparse_tensor(S, "csc")
    with pytest.raises(api.NnlmStop, match="loss = 'mse' only"):
        api.nnmf(A, 2, loss="mkl")
    with pytest.raises(api.NnlmStop, match="cannot be combined"):
        api.nnmf(A, 2, sparse_kl=True, absent="missing")
    with pytest.raises(api.NnlmStop, match=r"to_sparse_csc\(\)"):
        api.nnmf(A.to_sparse_coo(), 2)
    low = min(int(np.diff(S[0]).min()), int(np.diff(sdc.other_side(S)[0]).min()))
    with pytest.raises(api.NnlmStop, match="k larger than %d is not recommended" % low):  # the fewest stored entries of a line
        api.nnmf(A, low + 1, absent="missing")
    bad = S[2].copy()
    bad[3] = np.nan
    with pytest.raises(_lib.NnlmError, match="is not finite"):  # (a refusal that depends on the values: the library's message)
        api.nnmf(sparse_tensor((S[0], S[1], bad, S[3]), "csc"), 2)
    fitted = api.nnmf(Csc(S), 2, max_iter=2, rel_tol=-1.0, rng=np.random.default_rng(1))
    for fn, who in ((lambda: api.nnmf_cv(A, [2]), "nnmf_cv: A"), (lambda: api.nnlm(A, np.ones((37, 2))), "nnlm: x"),
                    (lambda: api.nnlm(np.ones((37, 2)), A), "nnlm: y"), (lambda: api.predict_nnmf(fitted, A, which="H"), "predict_nnmf: newdata"),
                    (lambda: api.top_n(fitted, 2, seen=A), "top_n: seen")):
        with pytest.raises(api.NnlmStop, match=who + " is a sparse tensor in device memory"):
            fn()


@pytest.mark.filterwarnings("ignore")
@pytest.mark.parametrize("layout", sdc.LAYOUTS)
@pytest.mark.parametrize("door,kw", [(True, {}), ("missing", {}), ("kl", dict(loss="mkl"))])
def test_api_nnmf_batch(door, kw, layout):
    S = case("powerlaw")
    A = sparse_tensor(S, layout)
    opts = dict(k=[2, 3], nrun=2, sparse_batch=door, max_iter=5, rel_tol=-1.0, check_k=False, **kw)
    rd, bd = api.nnmf_batch(A, rng=np.random.default_rng(3), **opts)
    rh, bh = api.nnmf_batch(Csc(S), rng=np.random.default_rng(3), **opts)
    assert bd == bh and len(rd) == len(rh) == 4
    for d, h in zip(rd, rh):
        assert isinstance(d["W"], torch.Tensor) and d["W"].device == A.device
        assert np.array_equal(d["W"].cpu().numpy(), h["W"]) and np.array_equal(d["H"].cpu().numpy(), h["H"])
        assert np.array_equal(d["mse"], h["mse"])
        assert d["options"]["absent"] == h["options"]["absent"]
