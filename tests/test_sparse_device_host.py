"""Host-side checks of the sparse device ingest (no GPU): the exports, the descriptor builder on duck-typed fakes, sparse_tensor_parts on
CPU torch sparse tensors, and the case table of sparse_device_cases.py (well posed from numpy alone, every stage edge present)."""
import os
import re
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_device_cases as sdc  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SHARE, TILE = sdc.header_constants()


def test_exports_declared_and_listed():
    header = open(os.path.join(ROOT, "include", "nnlm_mi355x.h")).read()
    for sym in ("nnlm_set_matrix_sparse_device", "nnlm_debug_sparse_resident"):
        assert re.search(r"\bint %s\(" % sym, header), sym
        assert sym in _lib.EXPORTS
    for name in ("NNLM_IT_I32 = 0", "NNLM_IT_I64 = 1", "NNLM_SP_CSC = 0", "NNLM_SP_CSR = 1", "NNLM_SP_ABSENT_MISSING = 1", "NNLM_SP_KL = 2",
                 "NNLM_SP_BATCH = 4"):
        assert name in header, name
    assert (_lib.IT_I32, _lib.IT_I64, _lib.SP_CSC, _lib.SP_CSR, _lib.SP_ABSENT_MISSING, _lib.SP_KL, _lib.SP_BATCH) == (0, 1, 0, 1, 1, 2, 4)
    # the descriptor's fields in the header's order
    m = re.search(r"typedef struct \{([^}]*)\} nnlm_dev_sparse;", header)
    names = re.findall(r"[*\s](\w+)\s*[,;]", m.group(1))
    assert names == [f[0] for f in _lib.DevSparse._fields_], names


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


def parts(n=5, m=4, nnz=7, pt="int64", it="int32", vt="float32"):
    return [Fake(m + 1, pt), Fake(nnz, it), Fake(nnz, vt)]


def test_dev_sparse_descriptor():
    p = parts()
    d, keep, shape, stream = _lib.dev_sparse(*p, (5, 4), "csc", device=0)
    assert (d.ptr_dtype, d.idx_dtype, d.val_dtype, d.layout, d.nnz) == (_lib.IT_I64, _lib.IT_I32, _lib.DT_F32, _lib.SP_CSC, 7)
    assert shape == (5, 4) and stream is None and d.ptr == p[0].data_ptr()
    p = [Fake(6, "int32"), Fake(7, "int64"), Fake(7, "bfloat16")]
    d = _lib.dev_sparse(*p, (5, 4), "csr")[0]
    assert (d.ptr_dtype, d.idx_dtype, d.val_dtype, d.layout) == (_lib.IT_I32, _lib.IT_I64, _lib.DT_BF16, _lib.SP_CSR)

    class Cai:  # a __cuda_array_interface__ producer
        def __init__(self, length, typestr, strides=None, stream=None):
            self.__cuda_array_interface__ = dict(shape=(length,), typestr=typestr, data=(0x7F0000002000, False), version=3, strides=strides,
                                                 stream=stream)

    d, _, _, stream = _lib.dev_sparse(Cai(5, "<i8"), Cai(7, "<i4", stream=77), Cai(7, "<f2", strides=(2,)), (5, 4), "csc")
    assert (d.ptr_dtype, d.idx_dtype, d.val_dtype, d.nnz, stream) == (_lib.IT_I64, _lib.IT_I32, _lib.DT_F16, 7, 77)
    with pytest.raises(ValueError, match="contiguous"):
        _lib.dev_sparse(Cai(5, "<i8"), Cai(7, "<i4", strides=(8,)), Cai(7, "<f8"), (5, 4), "csc")
    with pytest.raises(ValueError, match="typestr"):
        _lib.dev_sparse(Cai(5, "<f8"), Cai(7, "<i4"), Cai(7, "<f8"), (5, 4), "csc")


@pytest.mark.parametrize("which,change,match", [
    (1, dict(shape=(7, 1)), "1-D"),                   # a non-1-D array
    (2, dict(stride=2), "contiguous"),                # a non-unit stride
    (0, dict(length=4), "needs 5"),                   # len(ptr) != lines + 1
    (1, dict(length=6), "idx has 6 entries, val has 7"),
    (0, dict(dtype="int16"), "int32 or int64"),
    (1, dict(dtype="float32"), "int32 or int64"),     # an index dtype other than int32 / int64
    (2, dict(dtype="int32"), "float64, float32"),     # a value dtype outside the four
    (2, dict(dtype="complex64"), "float64, float32"),
    (0, dict(device="cpu"), "host memory"),           # a host tensor
    (2, dict(index=1), "device 1, the handle on device 0"),
])
def test_dev_sparse_refusals(which, change, match):
    spec = [dict(length=5, dtype="int64"), dict(length=7, dtype="int32"), dict(length=7, dtype="float64")]
    spec[which].update(change)
    with pytest.raises(ValueError, match=match):
        _lib.dev_sparse(*[Fake(**s) for s in spec], (5, 4), "csc", device=0)


def test_dev_sparse_layout_and_shape():
    with pytest.raises(ValueError, match="layout"):
        _lib.dev_sparse(*parts(), (5, 4), "coo")
    with pytest.raises(ValueError, match="needs 6"):  # the same arrays as CSR of a 5 x 4 matrix: n + 1 pointers
        _lib.dev_sparse(*parts(), (5, 4), "csr")
    with pytest.raises(ValueError, match="neither a tensor"):
        _lib.dev_sparse(np.zeros(5, dtype=np.int64), *parts()[1:], (5, 4), "csc")


def test_sparse_tensor_parts_on_cpu_tensors():
    torch = pytest.importorskip("torch")
    a = torch.tensor([[0.0, 1.5, 0.0], [2.0, 0.0, 0.25]], dtype=torch.float64)
    for t in (a.to_sparse_csc(), a.to_sparse_csr(), a.to_sparse(), a, a.numpy(), None, 3):
        assert _lib.sparse_tensor_parts(t) is None  # (host memory, or not a sparse tensor: not this route's)
    assert _lib.is_host_sparse_tensor(a.to_sparse_csc()) and _lib.is_host_sparse_tensor(a.to_sparse()) and not _lib.is_host_sparse_tensor(a)

    class OnDevice:  # a CPU sparse tensor presented as one of the GPU: the accessors are the real ones
        def __init__(self, t):
            self._t = t
            self.layout, self.shape = t.layout, t.shape
            self.device = types.SimpleNamespace(type="cuda", index=0)

        def __getattr__(self, name):
            return getattr(self._t, name)

    ptr, idx, val, shape, layout = _lib.sparse_tensor_parts(OnDevice(a.to_sparse_csc()))
    assert layout == "csc" and shape == (2, 3)
    assert ptr.tolist() == [0, 1, 2, 3] and idx.tolist() == [1, 0, 1] and val.tolist() == [2.0, 1.5, 0.25]
    ptr, idx, val, shape, layout = _lib.sparse_tensor_parts(OnDevice(a.to_sparse_csr()))
    assert layout == "csr" and ptr.tolist() == [0, 1, 3] and idx.tolist() == [1, 0, 2] and val.tolist() == [1.5, 2.0, 0.25]
    for other in (a.to_sparse(), a.to_sparse_bsr((1, 1)), a.to_sparse_bsc((1, 1))):
        with pytest.raises(ValueError, match=r"to_sparse_csc\(\)"):
            _lib.sparse_tensor_parts(OnDevice(other))
    assert not re.search(r"^\s*(import|from) torch", open(_lib.__file__).read(), flags=re.M)  # (_lib imports no tensor library)


def test_api_refuses_host_sparse_tensor_by_name():
    torch = pytest.importorskip("torch")
    a = torch.tensor([[0.0, 1.5, 0.0], [2.0, 0.0, 0.25]], dtype=torch.float64)
    for t in (a.to_sparse_csc(), a.to_sparse_csr(), a.to_sparse()):
        with pytest.raises(api.NnlmStop, match="nnmf: A is a sparse tensor in host memory"):
            api.nnmf(t, 1)
        with pytest.raises(api.NnlmStop, match="nnmf_batch: A is a sparse tensor in host memory"):
            api.nnmf_batch(t, 1, sparse_batch=True)
        with pytest.raises(api.NnlmStop, match="nnmf_cv: A is a sparse tensor in host memory"):
            api.nnmf_cv(t, [1])


def test_constants_come_from_the_header():
    assert SHARE >= 64 and TILE >= 64 and SHARE % 64 == 0 and TILE % 64 == 0


CASES = sdc.case_names(SHARE, TILE)


def test_case_table_covers_every_stage_edge():
    for c in (0, 1, 63, 64, 65, SHARE - 1, SHARE, SHARE + 1, TILE - 1, TILE, TILE + 1):
        assert "nnz_%d" % c in CASES
    for L in (1, 255, 256, 257, 65535, 65536, 65537, (1 << 24) + 1):
        assert "lines_%d" % L in CASES
    for name in ("one_row", "one_col", "full_column", "row_everywhere", "dominant_line", "empty_lines", "powerlaw", "small", "fit_heavy",
                 "fit_heavy_long"):
        assert name in CASES
    assert set(sdc.DOORS) == set(sdc.HOST_ENTRY) and len(sdc.DOORS) == 6


@pytest.mark.parametrize("name", [c for c in CASES if c != "lines_16777217"])
def test_case_is_well_posed(name):
    ptr, idx, val, (n, m) = sdc.build(name, SHARE, TILE)
    assert ptr.dtype == np.int64 and idx.dtype == np.int32 and val.dtype == np.float64
    assert ptr.shape == (m + 1,) and ptr[0] == 0 and ptr[-1] == idx.size == val.size and np.all(np.diff(ptr) >= 0)
    if idx.size:
        assert idx.min() >= 0 and idx.max() < n
    cols = np.repeat(np.arange(m), np.diff(ptr))
    same = cols[1:] == cols[:-1]
    assert np.all(idx[1:][same] > idx[:-1][same])  # strictly increasing in every line: no index repeats
    assert np.all(val == np.round(val * 64) / 64) and np.all((val >= 0) & (val < 4))
    for dt in ("float32", "float16"):
        assert np.array_equal(val.astype(dt).astype(np.float64), val)  # exact in the narrow types
    if name.startswith("nnz_"):
        assert idx.size == int(name[4:])
    if name.startswith("lines_"):
        assert n == int(name[6:])
    # the other side, by a stable argsort, is canonical too and transposes back
    rptr, cidx, rval = sdc.other_side((ptr, idx, val, (n, m)))
    rows = np.repeat(np.arange(n), np.diff(rptr))
    rs = rows[1:] == rows[:-1]
    assert rptr[-1] == idx.size and np.all(cidx[1:][rs] > cidx[:-1][rs])
    back = sdc.other_side((rptr, cidx, rval, (m, n)))
    assert np.array_equal(back[0], ptr) and np.array_equal(back[1], idx) and np.array_equal(back[2], val)
    if name == "dominant_line":
        assert np.diff(ptr).max() * 2 > idx.size
    if name == "empty_lines":
        d, r = np.diff(ptr), np.diff(rptr)
        assert d[0] == 0 and d[-1] == 0 and r[0] == 0 and r[-1] == 0 and np.any((d[1:-1] == 0) & (d[2:] == 0))
    if name == "row_everywhere":
        assert np.diff(rptr).max() == m
    if name == "full_column":
        assert np.diff(ptr).max() == n and np.count_nonzero(np.diff(ptr)) == 1
    if name == "fit_heavy":
        lim = 256  # lines the sparse KL solvers take in their long form are longer than this
        assert np.diff(ptr).max() > lim > np.diff(ptr).min() and np.diff(rptr).max() > lim > np.diff(rptr).min()
    if name == "fit_heavy_long":
        assert np.diff(ptr).max() > 2048 > np.diff(ptr).min() and np.diff(rptr).max() > 2048 > np.diff(rptr).min()
