"""Matrices and factors in device memory (nnlm_set_matrix_device / nnlm_set_factors_device / nnlm_get_factors_device), the part that
needs no GPU: the C-ABI surface, the descriptor _lib.dev_matrix builds from fake producers (objects exposing
__cuda_array_interface__ and a tensor-like class -- no tensor library is imported), its refusals, and the refusals of the entries that
stage their matrix on the host."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nnlm_set_matrix_device", "nnlm_set_factors_device", "nnlm_get_factors_device")
BASE = 0x7F0000001000  # a made-up device address: nothing here dereferences it


class Cai:
    """A fake __cuda_array_interface__ producer: the view `arr` (a numpy array, used for its shape / strides / dtype only) at BASE."""

    def __init__(self, arr, version=3, strides="auto", typestr=None, stream=None):
        s = arr.strides if strides == "auto" else strides
        if strides == "auto" and arr.flags.c_contiguous and version == 3:
            s = None  # what a producer reports for a C-contiguous array
        self.__cuda_array_interface__ = dict(shape=arr.shape, typestr=typestr or arr.dtype.str, data=(BASE, False), version=version, strides=s)
        if stream is not None:
            self.__cuda_array_interface__["stream"] = stream


class FakeDevice:
    def __init__(self, type_, index):
        self.type, self.index = type_, index


class FakeTensor:
    """A tensor-like class: data_ptr(), stride() in elements, shape, dtype (its str() ends in the type's name), device."""

    def __init__(self, shape, stride, dtype="fake.float32", device=("cuda", 0)):
        self.shape, self._stride, self.dtype, self.device = tuple(shape), tuple(stride), dtype, FakeDevice(*device)

    def data_ptr(self):
        return BASE

    def stride(self):
        return self._stride


def fields(d):
    return d.ptr, d.dtype, d.row_stride, d.col_stride


def test_entries_are_declared_exported_and_fail_on_a_null_handle():
    header = open(os.path.join(ROOT, "include", "nnlm_mi355x.h")).read()
    declared = set(re.findall(r"\b(nnlm_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "nnlm_dev_matrix" in header and "NNLM_DT_BF16 = 3" in header
    assert lib.nnlm_abi_version() == 1
    d = _lib.DevMatrix(BASE, _lib.DT_F64, 1, 4)
    assert lib.nnlm_set_matrix_device(None, ctypes.byref(d), 4, 4, None) == _lib.ERR_ARG
    assert lib.nnlm_set_factors_device(None, 2, None, None, None, None, None) == _lib.ERR_ARG
    assert lib.nnlm_get_factors_device(None, None, None, None) == _lib.ERR_ARG
    assert ctypes.sizeof(_lib.DevMatrix) == 32  # {void *, int, long long, long long} on LP64


def test_descriptor_from_cuda_array_interface():
    a = np.zeros((6, 4), dtype=np.float64)
    d, keep, shape, stream = _lib.dev_matrix(Cai(a))  # C order, strides None
    assert fields(d) == (BASE, _lib.DT_F64, 4, 1) and shape == (6, 4) and stream is None and keep is not None
    d, _, shape, _ = _lib.dev_matrix(Cai(a, version=2))  # C order, explicit byte strides
    assert fields(d) == (BASE, _lib.DT_F64, 4, 1)
    f = np.zeros((6, 4), dtype=np.float32, order="F")
    d, _, shape, _ = _lib.dev_matrix(Cai(f))
    assert fields(d) == (BASE, _lib.DT_F32, 1, 6) and shape == (6, 4)
    t = np.zeros((4, 6), dtype=np.float16).T  # transposed view of a C-contiguous 4 x 6
    d, _, shape, _ = _lib.dev_matrix(Cai(t))
    assert fields(d) == (BASE, _lib.DT_F16, 1, 6) and shape == (6, 4)
    s = np.zeros((12, 12), dtype=np.float64)[::2, 1::3]  # strided slice
    d, _, shape, _ = _lib.dev_matrix(Cai(s))
    assert fields(d) == (BASE, _lib.DT_F64, 24, 3) and shape == (6, 4)
    assert _lib.dev_matrix(Cai(a, stream=1))[3] is None and _lib.dev_matrix(Cai(a, stream=77))[3] == 77


def test_descriptor_from_a_tensor_like_object():
    for name, dt in (("float64", _lib.DT_F64), ("float32", _lib.DT_F32), ("float16", _lib.DT_F16), ("bfloat16", _lib.DT_BF16)):
        d, _, shape, _ = _lib.dev_matrix(FakeTensor((5, 3), (3, 1), "fake." + name), device=0)
        assert fields(d) == (BASE, dt, 3, 1) and shape == (5, 3)
    assert fields(_lib.dev_matrix(FakeTensor((5, 3), (1, 5)))[0]) == (BASE, _lib.DT_F32, 1, 5)       # F order / .t() view
    assert fields(_lib.dev_matrix(FakeTensor((5, 3), (20, 2)))[0]) == (BASE, _lib.DT_F32, 20, 2)     # strided slice
    assert _lib.is_device_array(FakeTensor((5, 3), (3, 1))) and _lib.is_device_array(Cai(np.zeros((2, 2))))
    assert not _lib.is_device_array(FakeTensor((5, 3), (3, 1), device=("cpu", None)))
    assert not _lib.is_device_array(np.zeros((2, 2))) and not _lib.is_device_array(None) and not _lib.is_device_array([[1.0]])


def test_descriptor_refusals_come_before_the_library_is_touched(monkeypatch):
    def no_load():
        raise AssertionError("dev_matrix must refuse before any device call")
    monkeypatch.setattr(_lib, "load", no_load)
    bad = [
        (Cai(np.zeros(5)), "2-D"),
        (Cai(np.zeros((2, 3, 4))), "2-D"),
        (FakeTensor((5,), (1,)), "2-D"),
        (Cai(np.zeros((3, 3), dtype=np.int32)), "integer"),
        (Cai(np.zeros((3, 3), dtype=np.bool_)), "bool"),
        (Cai(np.zeros((3, 3), dtype=np.complex128)), "complex"),
        (FakeTensor((3, 3), (3, 1), "fake.int64"), "integer"),
        (FakeTensor((3, 3), (3, 1), "fake.bool"), "bool"),
        (FakeTensor((3, 3), (3, 1), "fake.complex64"), "complex"),
        (FakeTensor((3, 3), (0, 1)), "zero"),                       # expand()
        (Cai(np.zeros((3, 3)), strides=(0, 8)), "zero"),
        (Cai(np.zeros((3, 3))[::-1]), "negative"),
        (FakeTensor((3, 3), (3, -1)), "negative"),
        (FakeTensor((3, 3), (3, 1), device=("cpu", None)), "host memory"),
        (FakeTensor((3, 3), (3, 1), device=("cuda", 1)), "device 1"),
    ]
    for x, word in bad:
        with pytest.raises(ValueError, match=word):
            _lib.dev_matrix(x, device=0)
    with pytest.raises(ValueError, match="neither"):
        _lib.dev_matrix(object(), device=0)


def test_host_staged_entries_refuse_device_memory_by_name():
    dev = FakeTensor((8, 6), (6, 1), "fake.float64")
    host = np.random.default_rng(0).random((8, 6))
    with pytest.raises(api.NnlmStop, match=r"nnmf_cv: A lives in device memory"):
        api.nnmf_cv(dev, 2)
    with pytest.raises(api.NnlmStop, match=r"nnlm: y lives in device memory"):
        api.nnlm(host, dev)
    with pytest.raises(api.NnlmStop, match=r"nnlm: x lives in device memory"):
        api.nnlm(dev, host[:, 0])
    model = dict(W=host[:, :2], H=host[:2, :], options=dict(method="scd", loss="mse"))
    with pytest.raises(api.NnlmStop, match=r"predict_nnmf: newdata lives in device memory"):
        api.predict_nnmf(model, dev, which="H")


def test_device_entries_fail_loudly_without_gpu(gpu_available):
    if gpu_available:
        pytest.skip("GPU present")
    dev = FakeTensor((20, 10), (10, 1), "fake.float64")
    with pytest.raises(nnlm_amd.NnlmError, match="no HIP device"):
        api.nnmf(dev, 2)
    with pytest.raises(nnlm_amd.NnlmError, match="no HIP device"):
        api.nnmf_batch(dev, 2, nrun=2)


def test_importing_the_package_does_not_import_torch():
    code = "import sys; import nnlm_amd; from nnlm_amd import api, _lib; assert 'torch' not in sys.modules, 'torch imported'"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
