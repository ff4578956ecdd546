"""Host-side checks of the weighted sparse device ingest (no GPU): the exports, the descriptor of the weights on duck-typed fakes (every
ValueError before a device call), which (A, weights) pairs api.nnmf sends where and which it refuses with which text, and the case table
of sparse_device_weighted_cases.py."""
import os
import re
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_device_cases as sdc  # noqa: E402
import sparse_device_weighted_cases as swc  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SHARE, TILE = sdc.header_constants()
CASES = swc.case_names(SHARE, TILE)


def test_exports_declared_and_listed():
    header = open(os.path.join(ROOT, "include", "nnlm_mi355x.h")).read()
    for sym in ("nnlm_set_matrix_sparse_device_weighted", "nnlm_debug_sparse_resident_weighted"):
        assert re.search(r"\bint %s\(" % sym, header), sym
        assert sym in _lib.EXPORTS
    for name in ("set_matrix_sparse_device_weighted", "debug_sparse_resident_weighted"):
        assert callable(getattr(_lib.Handle, name))
    # the unweighted entry and its descriptor are declared as before
    assert "int nnlm_set_matrix_sparse_device(nnlm_handle *h, const nnlm_dev_sparse *A, int n, int m, int door, void *stream);" in header
    assert ("typedef struct { const void *ptr, *idx, *val; int ptr_dtype, idx_dtype, val_dtype, layout; long long nnz; } nnlm_dev_sparse;"
            in header)


class Fake:
    """A tensor-like object as dev_sparse sees one."""

    def __init__(self, length, dtype, device="cuda", index=0, stride=1, shape=None, ptr=0x7F0000001000):
        self.shape = (length,) if shape is None else shape
        self.dtype = "torch." + dtype
        self.device = types.SimpleNamespace(type=device, index=index)
        self._stride, self._ptr = stride, ptr

    def stride(self):
        return (self._stride,) * len(self.shape)

    def data_ptr(self):
        return self._ptr


def test_weights_descriptor():
    d, keep, stream = _lib.dev_sparse_weights(Fake(7, "bfloat16", ptr=0x7F0000003000), 7, (5, 4), "csr", device=0)
    assert (d.ptr, d.idx, d.val, d.val_dtype, d.layout, d.nnz) == (None, None, 0x7F0000003000, _lib.DT_BF16, _lib.SP_CSR, 7) and stream is None
    triple = (Fake(5, "int32"), Fake(7, "int64"), Fake(7, "float16"))
    d, keep, stream = _lib.dev_sparse_weights(triple, 7, (5, 4), "csc", device=0)
    assert (d.ptr_dtype, d.idx_dtype, d.val_dtype, d.layout, d.nnz) == (_lib.IT_I32, _lib.IT_I64, _lib.DT_F16, _lib.SP_CSC, 7)
    assert d.ptr == triple[0].data_ptr() and keep == triple
    # a pattern of another nnz is the library's to name (first differing line): the descriptor carries it
    d = _lib.dev_sparse_weights((Fake(5, "int32"), Fake(6, "int32"), Fake(6, "float32")), 7, (5, 4), "csc")[0]
    assert d.nnz == 6


WEIGHT_REFUSALS = [
    (Fake(6, "float64"), "weights has 6 entries, val has 7"),                      # wrong length
    (Fake(7, "float64", device="cpu"), "weights lives in host memory"),            # a host tensor
    (Fake(7, "float64", index=1), "device 1, the handle on device 0"),             # another device
    (Fake(7, "int32"), "float64, float32"),                                        # an integer dtype
    (Fake(7, "float32", stride=2), "contiguous"),
    (Fake(7, "float32", shape=(7, 1)), "1-D"),
    (np.ones(7), "neither a tensor"),
    ((Fake(5, "int64"), Fake(7, "int32")), "triple"),
    ((Fake(4, "int64"), Fake(7, "int32"), Fake(7, "float32")), "needs 5"),
    ((Fake(5, "int64"), Fake(7, "float32"), Fake(7, "float32")), "int32 or int64"),
    ((Fake(5, "int64"), Fake(7, "int32"), Fake(6, "float32")), "idx has 7 entries, val has 6"),
    ((Fake(5, "int64", device="cpu"), Fake(7, "int32"), Fake(7, "float32")), "host memory"),
]


def test_weights_descriptor_refusals():
    for weights, match in WEIGHT_REFUSALS:
        with pytest.raises(ValueError, match=match):
            _lib.dev_sparse_weights(weights, 7, (5, 4), "csc", device=0)


def test_every_value_error_comes_before_a_device_call(monkeypatch):
    """The Handle method builds both descriptors first: with a library that fails on any call, the ValueErrors still arrive."""
    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError("device call %s" % name)

    h = object.__new__(_lib.Handle)
    h._lib, h._h, h.device = NoDevice(), None, 0
    good = [Fake(5, "int64"), Fake(7, "int32"), Fake(7, "float32")]
    for weights, match in ((Fake(6, "float64"), "weights has 6 entries"), (Fake(7, "float64", device="cpu"), "host memory"),
                           (Fake(7, "float64", index=1), "device 1"), (Fake(7, "int64"), "float64, float32")):
        with pytest.raises(ValueError, match=match):
            h.set_matrix_sparse_device_weighted(*good, weights, (5, 4))
    with pytest.raises(ValueError, match="absent"):
        h.set_matrix_sparse_device_weighted(*good, Fake(7, "float64"), (5, 4), absent="na")
    with pytest.raises(ValueError, match="needs 5"):  # the matrix's own descriptor, as in dev_sparse
        h.set_matrix_sparse_device_weighted(Fake(4, "int64"), *good[1:], Fake(7, "float64"), (5, 4))
    with pytest.raises(AssertionError, match="device call nnlm_set_matrix_sparse_device_weighted"):
        h.set_matrix_sparse_device_weighted(*good, Fake(7, "float64"), (5, 4))


# ---- the dispatch of api.nnmf(A, weights=) ----------------------------------------------------------------------------------------------------
class DenseOnDevice:
    shape, dtype, layout = (6, 5), "torch.float64", "torch.strided"
    device = types.SimpleNamespace(type="cuda", index=0)

    def data_ptr(self):
        return 0

    def stride(self):
        return (5, 1)


class SparseOnDevice(DenseOnDevice):
    layout = "torch.sparse_csc"


class VectorOnDevice(DenseOnDevice):
    shape = (7,)

    def stride(self):
        return (1,)


class Cai:
    __cuda_array_interface__ = dict(shape=(7,), typestr="<f8", data=(0x7F0000002000, False), version=3, strides=None)


class HostCsc:
    def __init__(self):
        self.indptr = np.array([0, 2, 3, 3, 5, 7], dtype=np.int64)
        self.indices = np.array([0, 4, 2, 1, 5, 0, 3], dtype=np.int32)
        self.data = np.arange(1.0, 8.0)
        self.shape = (6, 5)

    def tocsc(self):
        return self


HOST_W, DEV_W, DEV_SPARSE_W = np.ones(7), VectorOnDevice(), SparseOnDevice()
TO_DEVICE_DOOR = "device door"
DISPATCH = [  # (A, weights) -> the device door, or the text of the refusal
    (SparseOnDevice(), DEV_W, TO_DEVICE_DOOR),
    (SparseOnDevice(), Cai(), TO_DEVICE_DOOR),
    (SparseOnDevice(), DEV_SPARSE_W, TO_DEVICE_DOOR),
    (SparseOnDevice(), HOST_W, "weights cannot be combined with a A in device memory"),
    (SparseOnDevice(), HostCsc(), "weights cannot be combined with a A in device memory"),
    (DenseOnDevice(), HOST_W, "weights cannot be combined with a A in device memory"),
    (DenseOnDevice(), DEV_W, "weights cannot be combined with a A in device memory"),
    (DenseOnDevice(), DEV_SPARSE_W, "weights cannot be combined with a A in device memory"),
    (HostCsc(), DEV_W, "weights live in device memory, but A is a host matrix"),
    (HostCsc(), Cai(), "weights live in device memory, but A is a host matrix"),
    (HostCsc(), DEV_SPARSE_W, "weights live in device memory, but A is a host matrix"),
    (np.ones((6, 5)), DEV_W, "weights live in device memory, but A is a host matrix"),
    (np.ones((6, 5)), HOST_W, "weights need a sparse A"),
]


def test_api_dispatch_table():
    for A, weights, where in DISPATCH:
        _dispatch(A, weights, where)


def _dispatch(A, weights, where):
    if where == TO_DEVICE_DOOR:
        assert api._weights_refusals("nnmf", "A", A, "mse", False, None, weights, device_door=True) is True
        # an entry without that door (nnlm) keeps its refusal
        with pytest.raises(api.NnlmStop, match="weights cannot be combined with a y in device memory"):
            api._weights_refusals("nnlm", "y", A, "mse", False, None, weights)
        for kw, text in ((dict(loss="mkl"), "loss = 'mse' only"), (dict(sparse_kl=True), "loss = 'mse' only"),
                         (dict(init="nndsvd"), "cannot be combined with init = 'nndsvd'")):
            with pytest.raises(api.NnlmStop, match=text):
                api.nnmf(A, 2, weights=weights, **kw)
    else:
        with pytest.raises(api.NnlmStop, match=where):
            api.nnmf(A, 2, weights=weights)


def test_host_pairs_still_take_the_host_route():
    assert api._weights_refusals("nnmf", "A", HostCsc(), "mse", False, None, HOST_W, device_door=True) is False
    assert api._weights_refusals("nnmf", "A", HostCsc(), "mse", False, None, HostCsc(), device_door=True) is False


def test_sparse_weights_of_another_layout_or_shape_are_refused_by_name():
    parts = ("p", "i", "v", (6, 5), "csc")

    class W:
        device = types.SimpleNamespace(type="cuda", index=0)

        def __init__(self, layout, shape):
            self.layout, self.shape = layout, shape

        def ccol_indices(self):
            return "wp"

        crow_indices = ccol_indices

        def row_indices(self):
            return "wi"

        col_indices = row_indices

        def values(self):
            return "wv"

    assert api._device_weights_arg(W("torch.sparse_csc", (6, 5)), parts, "nnmf") == ("wp", "wi", "wv")
    dense = VectorOnDevice()
    assert api._device_weights_arg(dense, parts, "nnmf") is dense
    with pytest.raises(api.NnlmStop, match="nnmf: weights is a sparse CSR tensor, the matrix a sparse CSC tensor"):
        api._device_weights_arg(W("torch.sparse_csr", (6, 5)), parts, "nnmf")
    with pytest.raises(api.NnlmStop, match="nnmf: weights is 5 x 6, the matrix 6 x 5"):
        api._device_weights_arg(W("torch.sparse_csc", (5, 6)), parts, "nnmf")
    with pytest.raises(api.NnlmStop, match=r"nnmf: weights: a device tensor of layout torch.sparse_coo"):
        api._device_weights_arg(W("torch.sparse_coo", (6, 5)), parts, "nnmf")


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_every_family():
    for c in (0, 1, 63, 64, 65, SHARE - 1, SHARE, SHARE + 1, TILE - 1, TILE, TILE + 1, 2 * SHARE + 1, 2 * TILE + 1):
        assert "nnz_%d" % c in CASES
    for name in ("powerlaw", "dominant_line", "empty_lines", "lines_257", "lines_65535", "lines_65536", "lines_65537", "fit_heavy",
                 "fit_heavy_long", "small"):
        assert name in CASES
    assert sum(sdc.big(c) for c in CASES) == 3


def test_offence_positions_sit_on_both_sides_of_a_boundary():
    nnz = 2 * SHARE + 1
    pos = swc.offence_positions(nnz, SHARE)
    assert pos["first"] == 0 and pos["last"] == nnz - 1
    assert pos["below_share"] // SHARE == 0 and pos["at_share"] // SHARE == 1 and pos["at_share"] - pos["below_share"] == 1
    assert pos["last"] // SHARE == 2
    for v in swc.OFFENCES.values():
        assert not (np.isfinite(v) and v >= 0)
    z = swc.LEGAL["minus_zero"]
    assert np.signbit(z) and np.isfinite(z) and not z < 0.0  # (the host's rule: finite and not below zero)


def test_case_weights():
    for name in CASES:
        _case_weights(name)


def _case_weights(name):
    S = sdc.build(name, SHARE, TILE)
    nnz = S[1].size
    w = swc.weights(name, nnz)
    assert w.shape == (nnz,) and w.dtype == np.float64 and np.all(np.isfinite(w)) and np.all(w >= 0)
    assert np.array_equal(w, swc.weights(name, nnz))  # seeded from the name
    if nnz >= 64:
        wa = w * S[2]
        assert np.any(w == 1.0) and np.any(w == 0.0)
        assert np.any(w.astype(np.float32).astype(np.float64) != w) and np.any(wa.astype(np.float32).astype(np.float64) != wa)
        exact = w == np.round(w * 8) / 8
        assert np.any(exact & (w != 0) & (w != 1))
    # the restatement: the other side is the stable transposition, with the product formed before the rounding
    (ptr, idx, val, wt, wa), (rptr, cidx, rval, rwt, rwa) = swc.resident(S, w, False)
    o = swc.order_of_other_side(S)
    assert np.array_equal(rval, val[o]) and np.array_equal(rwt, wt[o]) and np.array_equal(rwa, wa[o])
    assert np.array_equal(wa, (w * S[2]).astype(np.float32).astype(np.float64))
    back = np.empty_like(o)
    back[o] = np.arange(nnz)
    T = sdc.transposed(S)
    assert np.array_equal(swc.order_of_other_side(T), back)  # transposing twice restores the order of the weights


def test_loop_statistics_agree_with_a_direct_evaluation():
    for name in ("small", "powerlaw", "nnz_65", "empty_lines"):
        _loop_statistics(name)


def _loop_statistics(name):
    S = sdc.build(name, SHARE, TILE)
    w = swc.weights(name, S[1].size)
    for val, c in [(S[2], w)] + [(v, c) for v, c, _ in swc.range_rule_inputs(S).values()]:
        a, b = swc.loop_statistics(val, c), swc.direct_statistics(val, c)
        assert a[:3] == b[:3], (a, b)
        assert abs(a[3] - b[3]) <= 1e-12 * max(abs(b[3]), 1e-300), (a, b)


def test_range_rule_inputs_trip_one_rule_each():
    S = sdc.build("small", SHARE, TILE)
    r = swc.range_rule_inputs(S)
    for name in ("c_alone", "ca_alone"):
        v, c, _ = r[name]
        over, mx, wmx, _ = swc.loop_statistics(v, c)
        assert over == 1.0 and np.all(np.abs(v) <= swc.FP32_MAX) and mx >= swc.FP32_FLOOR
    v, c, _ = r["c_alone"]
    assert np.all(np.abs(c * v) <= swc.FP32_MAX) and c.max() > swc.FP32_MAX
    v, c, _ = r["ca_alone"]
    assert c.max() <= swc.FP32_MAX and np.abs(c * v).max() > swc.FP32_MAX
    v, c, _ = r["wmx_floor"]
    over, mx, wmx, _ = swc.loop_statistics(v, c)
    assert over == 0.0 and mx >= swc.FP32_FLOOR and 0.0 < wmx < swc.FP32_FLOOR


def test_pattern_changes_name_their_first_line():
    for G in (sdc.build("powerlaw", SHARE, TILE), sdc.transposed(sdc.build("powerlaw", SHARE, TILE))):
        ptr, idx = G[0], G[1]
        for what, ((p2, i2), nnz2, first) in swc.pattern_changes(G).items():
            assert p2.shape == ptr.shape and i2.size == nnz2 == p2[-1]
            assert (nnz2 == idx.size) == (what != "other_nnz")
            lines = [j for j in range(ptr.size - 1)
                     if not np.array_equal(idx[ptr[j]:ptr[j + 1]], i2[p2[j]:p2[j + 1]])]
            assert lines and lines[0] == first, (what, lines[:3], first)
