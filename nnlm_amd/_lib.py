"""ctypes binding of libnnlm_mi355x.so (include/nnlm_mi355x.h).

This is the Python stand-in for the R-side ``.Call`` stub (pkg/src/r_glue.c): it passes
plain pointers and sizes across the C ABI, nothing else.  There is deliberately NO fallback: if
the shared library is missing or no gfx950 device is present, every entry raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libnnlm_mi355x.so")

NNLM_OK = 0
ERR_ARG = 1
ERR_UNSUPPORTED = 5
BATCH_MAX = 64  # members of one batched factorisation, and the largest sum of their ranks
PREC_F32 = 0
PREC_F64 = 1
COMM_ID_BYTES = 128
FORM_COLS = 0    # column-sharded half-steps, one all-gather each (default)
FORM_REDUCE = 1  # dense square loss: contraction-sharded [G | C] + all-reduce, then sweep + all-gather
FORMS = {"cols": FORM_COLS, "reduce": FORM_REDUCE}

# every symbol include/nnlm_mi355x.h declares (tests check the .so exports all of them)
EXPORTS = [
    "nnlm_trace_capacity", "nnlm_c_nnmf", "nnlm_c_nnlm", "nnlm_create", "nnlm_destroy", "nnlm_last_error",
    "nnlm_abi_version", "nnlm_set_matrix", "nnlm_matrix_info", "nnlm_set_factors", "nnlm_get_factors",
    "nnlm_half_step", "nnlm_iterate", "nnlm_run", "nnlm_take_sweeps", "nnlm_errors", "nnlm_sync", "nnlm_profile_enable",
    "nnlm_profile_get", "nnlm_profile_reset", "nnlm_comm_unique_id", "nnlm_comm_init", "nnlm_comm_info",
    "nnlm_shard_range", "nnlm_shard_cols", "nnlm_debug_partial", "nnlm_debug_phase", "nnlm_debug_exchange",
    "nnlm_comm_set_form", "nnlm_debug_set_cus", "nnlm_debug_set_xprod_waves", "nnlm_debug_set_a_stream", "nnlm_xprod_plan", "nnlm_kl_plan", "nnlm_get_info", "nnlm_debug_alloc_limit", "nnlm_debug_poison_workspaces", "nnlm_release_caches",
    "nnlm_set_matrix_csc", "nnlm_c_nnmf_csc", "nnlm_c_nnlm_csc",
    "nnlm_set_matrix_csc_missing", "nnlm_c_nnmf_csc_missing", "nnlm_c_nnlm_csc_missing",
    "nnlm_set_matrix_csc_kl", "nnlm_c_nnmf_csc_kl", "nnlm_c_nnlm_csc_kl",
    "nnlm_set_factors_batch", "nnlm_get_factors_batch", "nnlm_run_batch", "nnlm_c_nnmf_batch",
    "nnlm_set_matrix_holdout", "nnlm_holdout_errors", "nnlm_c_nnmf_holdout_batch",
    "nnlm_set_matrix_device", "nnlm_set_factors_device", "nnlm_get_factors_device",
    "nnlm_predict_entries", "nnlm_top_n", "nnlm_top_n_eval",
    "nnlm_set_matrix_csc_batch", "nnlm_c_nnmf_csc_batch",
    "nnlm_set_matrix_csc_kl_batch", "nnlm_c_nnmf_csc_kl_batch",
    "nnlm_set_matrix_csc_missing_batch", "nnlm_c_nnmf_csc_missing_batch",
    "nnlm_set_matrix_sparse_device", "nnlm_debug_sparse_resident",
    "nnlm_set_matrix_csc_weighted", "nnlm_c_nnmf_csc_weighted", "nnlm_c_nnlm_csc_weighted",
    "nnlm_set_matrix_sparse_device_weighted", "nnlm_debug_sparse_resident_weighted",
    "nnlm_svd", "nnlm_get_svd", "nnlm_set_factors_nndsvd", "nnlm_set_factors_nndsvd_batch", "nnlm_debug_set_svd_rotate",
]
NNDSVD_VARIANTS = {"nndsvd": 0, "nndsvda": 1}
TOPN_MAX = 128  # largest n_top of nnlm_top_n
TOPN_EVAL_MAX_CUT = 8  # cutoffs per nnlm_top_n_eval call
BY = {"column": 0, "row": 1}


class NnlmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libnnlm_mi355x error {code}: {msg}")
        self.code = code


class DevMatrix(C.Structure):
    """nnlm_dev_matrix: element (i, j) at ptr[i * row_stride + j * col_stride], strides in elements."""
    _fields_ = [("ptr", C.c_void_p), ("dtype", C.c_int), ("row_stride", C.c_longlong), ("col_stride", C.c_longlong)]


class DevSparse(C.Structure):
    """nnlm_dev_sparse: a CSC / CSR matrix in device memory (three contiguous 1-D arrays)."""
    _fields_ = [("ptr", C.c_void_p), ("idx", C.c_void_p), ("val", C.c_void_p), ("ptr_dtype", C.c_int), ("idx_dtype", C.c_int),
                ("val_dtype", C.c_int), ("layout", C.c_int), ("nnz", C.c_longlong)]


DT_F64, DT_F32, DT_F16, DT_BF16 = 0, 1, 2, 3
IT_I32, IT_I64 = 0, 1
SP_CSC, SP_CSR = 0, 1
SP_ABSENT_MISSING, SP_KL, SP_BATCH = 1, 2, 4  # `door` bits of nnlm_set_matrix_sparse_device
SP_LAYOUTS = {"csc": SP_CSC, "csr": SP_CSR}
_IT_NAMES = {"int32": IT_I32, "int64": IT_I64, "int": IT_I32, "long": IT_I64}
_IT_TYPESTR = {"i4": IT_I32, "i8": IT_I64}
_DT_SIZE = {DT_F64: 8, DT_F32: 4, DT_F16: 2, DT_BF16: 2}
_DT_NAMES = {"float64": DT_F64, "float32": DT_F32, "float16": DT_F16, "bfloat16": DT_BF16, "double": DT_F64, "float": DT_F32, "half": DT_F16}
_DT_TYPESTR = {"f8": DT_F64, "f4": DT_F32, "f2": DT_F16}


class Callbacks(C.Structure):
    _fields_ = [
        ("ctx", C.c_void_p),
        ("check_interrupt", C.CFUNCTYPE(C.c_int, C.c_void_p)),
        ("progress", C.CFUNCTYPE(None, C.c_void_p, C.c_uint, C.c_uint)),
        ("print", C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)),
        ("warning", C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)),
        ("unif_rand", C.CFUNCTYPE(C.c_double, C.c_void_p)),
    ]


_lib = None


def load():
    """Load the shared library (raises if it has not been built: there is no CPU path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NnlmError(-1, f"{LIB_PATH} not found: build it with `python -m nnlm_amd.build` (hipcc, gfx950)")
    lib = C.CDLL(LIB_PATH)
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
    lib.nnlm_abi_version.restype = C.c_int
    lib.nnlm_last_error.restype = C.c_char_p
    lib.nnlm_last_error.argtypes = [vp]
    lib.nnlm_trace_capacity.restype = C.c_uint
    lib.nnlm_trace_capacity.argtypes = [C.c_uint, C.c_uint]
    lib.nnlm_c_nnmf.restype = C.c_int
    lib.nnlm_c_nnmf.argtypes = [dp, C.c_int, C.c_int, C.c_uint, dp, dp, ip, ip, dp, dp, C.c_uint, C.c_double, C.c_int,
                                C.c_int, C.c_int, C.c_uint, C.c_double, C.c_int, C.c_uint, dp, dp, dp, dp, dp, dp, ip,
                                C.POINTER(C.c_uint), ip, C.POINTER(Callbacks)]
    lp = C.POINTER(C.c_longlong)
    lib.nnlm_c_nnmf_csc.restype = C.c_int
    lib.nnlm_c_nnmf_csc.argtypes = [C.c_int, C.c_int, lp, ip, dp] + lib.nnlm_c_nnmf.argtypes[3:]
    lib.nnlm_c_nnlm.restype = C.c_int
    lib.nnlm_c_nnlm.argtypes = [dp, dp, C.c_int, C.c_int, C.c_int, dp, ip, dp, C.c_uint, C.c_double, C.c_int, C.c_int,
                                dp, ip, C.POINTER(Callbacks)]
    lib.nnlm_c_nnlm_csc.restype = C.c_int
    lib.nnlm_c_nnlm_csc.argtypes = [dp, C.c_int, C.c_int, C.c_int, lp, ip, dp] + lib.nnlm_c_nnlm.argtypes[5:]
    lib.nnlm_set_matrix_csc.restype = C.c_int
    lib.nnlm_set_matrix_csc.argtypes = [vp, C.c_int, C.c_int, lp, ip, dp]
    for name in ("nnlm_c_nnmf_csc", "nnlm_c_nnlm_csc", "nnlm_set_matrix_csc"):  # absent entries missing: the same arguments
        getattr(lib, name + "_missing").restype = C.c_int
        getattr(lib, name + "_missing").argtypes = getattr(lib, name).argtypes
        getattr(lib, name + "_kl").restype = C.c_int  # (absent entries zeros, KL loss too: the same arguments)
        getattr(lib, name + "_kl").argtypes = getattr(lib, name).argtypes
    # per-entry weights: weight, absent_missing behind x / yx
    lib.nnlm_set_matrix_csc_weighted.restype = C.c_int
    lib.nnlm_set_matrix_csc_weighted.argtypes = lib.nnlm_set_matrix_csc.argtypes + [dp, C.c_int]
    lib.nnlm_c_nnmf_csc_weighted.restype = C.c_int
    lib.nnlm_c_nnmf_csc_weighted.argtypes = lib.nnlm_c_nnmf_csc.argtypes[:5] + [dp, C.c_int] + lib.nnlm_c_nnmf_csc.argtypes[5:]
    lib.nnlm_c_nnlm_csc_weighted.restype = C.c_int
    lib.nnlm_c_nnlm_csc_weighted.argtypes = lib.nnlm_c_nnlm_csc.argtypes[:7] + [dp, C.c_int] + lib.nnlm_c_nnlm_csc.argtypes[7:]
    lib.nnlm_create.restype = C.c_int
    lib.nnlm_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int]
    lib.nnlm_destroy.restype = None
    lib.nnlm_destroy.argtypes = [vp]
    lib.nnlm_set_matrix.restype = C.c_int
    lib.nnlm_set_matrix.argtypes = [vp, dp, C.c_int, C.c_int]
    lib.nnlm_matrix_info.restype = C.c_int
    lib.nnlm_matrix_info.argtypes = [vp, dp, ip, dp]
    lib.nnlm_set_factors.restype = C.c_int
    lib.nnlm_set_factors.argtypes = [vp, C.c_uint, dp, dp, ip, ip]
    lib.nnlm_get_factors.restype = C.c_int
    lib.nnlm_get_factors.argtypes = [vp, dp, dp]
    lib.nnlm_half_step.restype = C.c_int
    lib.nnlm_half_step.argtypes = [vp, C.c_int, dp, C.c_uint, C.c_double, C.c_int]
    lib.nnlm_iterate.restype = C.c_int
    lib.nnlm_iterate.argtypes = [vp, C.c_uint, dp, dp, C.c_uint, C.c_double, C.c_int]
    lib.nnlm_run.restype = C.c_int
    lib.nnlm_run.argtypes = [vp, dp, dp, C.c_uint, C.c_double, C.c_int, C.c_int, C.c_uint, C.c_double, C.c_int, C.c_uint,
                             dp, dp, dp, dp, ip, C.POINTER(C.c_uint), ip, C.POINTER(Callbacks)]
    lib.nnlm_take_sweeps.restype = C.c_int
    lib.nnlm_take_sweeps.argtypes = [vp, C.POINTER(C.c_longlong), C.c_int]
    lib.nnlm_errors.restype = C.c_int
    lib.nnlm_errors.argtypes = [vp, dp, dp, dp]
    lib.nnlm_sync.restype = C.c_int
    lib.nnlm_sync.argtypes = [vp]
    lib.nnlm_profile_enable.restype = C.c_int
    lib.nnlm_profile_enable.argtypes = [vp, C.c_int]
    lib.nnlm_profile_reset.restype = C.c_int
    lib.nnlm_profile_reset.argtypes = [vp]
    lib.nnlm_profile_get.restype = C.c_int
    lib.nnlm_profile_get.argtypes = [vp, C.c_char_p, dp, C.POINTER(C.c_longlong)]
    lib.nnlm_comm_unique_id.restype = C.c_int
    lib.nnlm_comm_unique_id.argtypes = [C.c_char_p]
    lib.nnlm_comm_init.restype = C.c_int
    lib.nnlm_comm_init.argtypes = [vp, C.c_char_p, C.c_int, C.c_int]
    lib.nnlm_comm_info.restype = C.c_int
    lib.nnlm_comm_info.argtypes = [vp, ip, ip]
    lib.nnlm_shard_range.restype = C.c_int
    lib.nnlm_shard_range.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, ip, ip]
    lib.nnlm_shard_cols.restype = C.c_int
    lib.nnlm_shard_cols.argtypes = [C.c_int, C.c_int, C.c_int, ip, ip, ip]
    lib.nnlm_debug_partial.restype = C.c_int
    lib.nnlm_debug_partial.argtypes = [vp, C.c_int, dp, dp]
    lib.nnlm_debug_phase.restype = C.c_int
    lib.nnlm_debug_phase.argtypes = [vp, C.c_int, C.c_int, dp, C.c_uint, C.c_double, C.c_int]
    lib.nnlm_debug_exchange.restype = C.c_int
    lib.nnlm_debug_exchange.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int]
    lib.nnlm_comm_set_form.restype = C.c_int
    lib.nnlm_comm_set_form.argtypes = [vp, C.c_int]
    lib.nnlm_debug_set_cus.restype = C.c_int
    lib.nnlm_debug_set_cus.argtypes = [C.c_int]
    lib.nnlm_debug_set_xprod_waves.restype = C.c_int
    lib.nnlm_debug_set_xprod_waves.argtypes = [C.c_int]
    lib.nnlm_debug_set_a_stream.restype = C.c_int
    lib.nnlm_debug_set_a_stream.argtypes = [C.c_int]
    lib.nnlm_xprod_plan.restype = C.c_int
    lib.nnlm_xprod_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, ip]
    lib.nnlm_kl_plan.restype = C.c_int
    lib.nnlm_kl_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, ip]
    lib.nnlm_debug_alloc_limit.restype = C.c_int
    lib.nnlm_debug_alloc_limit.argtypes = [C.c_size_t]
    lib.nnlm_debug_poison_workspaces.restype = C.c_int
    lib.nnlm_debug_poison_workspaces.argtypes = [C.c_int]
    lib.nnlm_release_caches.restype = C.c_int
    lib.nnlm_release_caches.argtypes = []
    lib.nnlm_get_info.restype = C.c_int
    lib.nnlm_get_info.argtypes = [vp, C.c_char_p, dp]
    up = C.POINTER(C.c_uint)
    lib.nnlm_set_factors_batch.restype = C.c_int
    lib.nnlm_set_factors_batch.argtypes = [vp, C.c_uint, up, dp, dp]
    lib.nnlm_get_factors_batch.restype = C.c_int
    lib.nnlm_get_factors_batch.argtypes = [vp, dp, dp]
    lib.nnlm_run_batch.restype = C.c_int
    lib.nnlm_run_batch.argtypes = lib.nnlm_run.argtypes
    lib.nnlm_c_nnmf_batch.restype = C.c_int
    lib.nnlm_c_nnmf_batch.argtypes = [dp, C.c_int, C.c_int, C.c_uint, up, dp, dp, dp, dp, C.c_uint, C.c_double, C.c_int, C.c_int, C.c_int,
                                      C.c_uint, C.c_double, C.c_int, C.c_uint, dp, dp, dp, dp, dp, dp, ip, up, ip, C.POINTER(Callbacks)]
    lib.nnlm_c_nnmf_csc_batch.restype = C.c_int
    lib.nnlm_c_nnmf_csc_batch.argtypes = [C.c_int, C.c_int, lp, ip, dp] + lib.nnlm_c_nnmf_batch.argtypes[3:]
    lib.nnlm_set_matrix_csc_batch.restype = C.c_int
    lib.nnlm_set_matrix_csc_batch.argtypes = lib.nnlm_set_matrix_csc.argtypes
    lib.nnlm_c_nnmf_csc_kl_batch.restype = C.c_int
    lib.nnlm_c_nnmf_csc_kl_batch.argtypes = lib.nnlm_c_nnmf_csc_batch.argtypes
    lib.nnlm_set_matrix_csc_kl_batch.restype = C.c_int
    lib.nnlm_set_matrix_csc_kl_batch.argtypes = lib.nnlm_set_matrix_csc.argtypes
    lib.nnlm_set_matrix_csc_missing_batch.restype = C.c_int
    lib.nnlm_set_matrix_csc_missing_batch.argtypes = lib.nnlm_set_matrix_csc.argtypes + [lp, ip]
    lib.nnlm_c_nnmf_csc_missing_batch.restype = C.c_int
    lib.nnlm_c_nnmf_csc_missing_batch.argtypes = ([C.c_int, C.c_int, lp, ip, dp, lp, ip] + lib.nnlm_c_nnmf_batch.argtypes[3:-1]
                                                  + [dp, dp, C.POINTER(Callbacks)])
    lib.nnlm_set_matrix_holdout.restype = C.c_int
    lib.nnlm_set_matrix_holdout.argtypes = [vp, dp, C.c_int, C.c_int, lp, ip]
    lib.nnlm_holdout_errors.restype = C.c_int
    lib.nnlm_holdout_errors.argtypes = [vp, dp, dp]
    lib.nnlm_c_nnmf_holdout_batch.restype = C.c_int
    lib.nnlm_c_nnmf_holdout_batch.argtypes = (lib.nnlm_c_nnmf_batch.argtypes[:3] + [lp, ip] + lib.nnlm_c_nnmf_batch.argtypes[3:-1]
                                              + [dp, dp, C.POINTER(Callbacks)])
    dmp = C.POINTER(DevMatrix)
    lib.nnlm_set_matrix_device.restype = C.c_int
    lib.nnlm_set_matrix_device.argtypes = [vp, dmp, C.c_int, C.c_int, vp]
    lib.nnlm_set_factors_device.restype = C.c_int
    lib.nnlm_set_factors_device.argtypes = [vp, C.c_uint, dmp, dmp, ip, ip, vp]
    lib.nnlm_get_factors_device.restype = C.c_int
    lib.nnlm_get_factors_device.argtypes = [vp, dmp, dmp, vp]
    lib.nnlm_set_matrix_sparse_device.restype = C.c_int
    lib.nnlm_set_matrix_sparse_device.argtypes = [vp, C.POINTER(DevSparse), C.c_int, C.c_int, C.c_int, vp]
    lib.nnlm_debug_sparse_resident.restype = C.c_int
    lib.nnlm_debug_sparse_resident.argtypes = [vp, C.c_int, lp, ip, dp]
    lib.nnlm_set_matrix_sparse_device_weighted.restype = C.c_int
    lib.nnlm_set_matrix_sparse_device_weighted.argtypes = [vp, C.POINTER(DevSparse), C.POINTER(DevSparse), C.c_int, C.c_int, C.c_int, vp]
    lib.nnlm_debug_sparse_resident_weighted.restype = C.c_int
    lib.nnlm_debug_sparse_resident_weighted.argtypes = [vp, C.c_int, dp, dp]
    lib.nnlm_predict_entries.restype = C.c_int
    lib.nnlm_predict_entries.argtypes = [vp, C.c_longlong, ip, ip, dp]
    lib.nnlm_svd.argtypes = [vp, C.c_uint, C.c_uint, dp]
    lib.nnlm_get_svd.argtypes = [vp, C.c_uint, dp, dp, dp]
    lib.nnlm_debug_set_svd_rotate.argtypes = [C.c_int]
    lib.nnlm_set_factors_nndsvd.argtypes = [vp, C.c_uint, C.c_int]
    lib.nnlm_set_factors_nndsvd_batch.argtypes = [vp, C.c_uint, up, C.c_int]
    lib.nnlm_top_n.restype = C.c_int
    lib.nnlm_top_n.argtypes = [vp, C.c_int, C.c_int, ip, C.c_longlong, C.c_int, ip, dp]
    lib.nnlm_top_n_eval.restype = C.c_int
    lib.nnlm_top_n_eval.argtypes = [vp, C.c_int, ip, C.c_int, ip, C.c_longlong, C.c_int, C.POINTER(C.c_longlong), ip, dp,
                                    C.POINTER(C.c_longlong), dp]
    _lib = lib
    return lib


def _check(rc, handle=None):
    if rc != NNLM_OK:
        msg = load().nnlm_last_error(handle)
        raise NnlmError(rc, msg.decode() if msg else "unknown")


def _f64(a, shape=None):
    """Column-major fp64 array (what R hands to .Call).  The library never writes its inputs, so an array that already is fp64 and
    Fortran-contiguous is passed as it is (a 1.6 GB transposing copy of a C-ordered 20000 x 10000 matrix takes longer than its upload)."""
    arr = np.asarray(a, dtype=np.float64)
    if shape is not None:
        arr = arr.reshape(shape, order="F") if arr.flags.f_contiguous else np.asfortranarray(arr).reshape(shape, order="F")
    if not arr.flags.f_contiguous:
        arr = np.asfortranarray(arr)
    return arr


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))


def _lgl(mask, shape):
    """R logical matrix -> int32 column-major, or None when empty (src/nnmf.cpp:75-80)."""
    if mask is None or np.size(mask) == 0:
        return None
    return np.array(np.asarray(mask).reshape(shape) != 0, dtype=np.int32, order="F")


def _lp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_longlong))


def _csc_arrays(indptr, indices, data):
    """CSC arrays in the types of the C ABI (int64 pointers, int32 indices, fp64 values), contiguous; the structure is passed as it is
    (nnlm_set_matrix_csc checks it: canonicalisation is the caller's, see api.as_csc)."""
    return (np.ascontiguousarray(indptr, dtype=np.int64), np.ascontiguousarray(indices, dtype=np.int32),
            np.ascontiguousarray(data, dtype=np.float64))


def index_array(x, name):
    """A one-dimensional array of integers as contiguous int32 (ValueError for any other dtype, a value beyond int32 or another shape);
    the range against n / m is the library's check."""
    a = np.asarray(x)
    if a.ndim != 1:
        raise ValueError(f"{name} must be a one-dimensional array of integers (got shape {a.shape})")
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name} must hold integers (got dtype {a.dtype})")
    if a.size and (int(a.max()) > np.iinfo(np.int32).max or int(a.min()) < np.iinfo(np.int32).min):
        raise ValueError(f"{name} holds an index beyond 32 bits")
    return np.ascontiguousarray(a, dtype=np.int32)


def by_code(by):
    if by not in BY:
        raise ValueError(f"by must be 'column' or 'row' (got {by!r})")
    return BY[by]


# ----------------------------------------------------------------------------------------------
# arrays in device memory (nnlm_dev_matrix); no tensor library is ever imported here
# ----------------------------------------------------------------------------------------------
def _is_tensor_like(x):
    return all(hasattr(x, a) for a in ("data_ptr", "stride", "shape", "dtype", "device")) and callable(x.data_ptr)


def is_device_array(x):
    """True for what dev_matrix() takes as device memory: a tensor-like object (data_ptr(), stride(), shape, dtype, device) whose
    device is not the CPU, or any other object exposing __cuda_array_interface__."""
    if x is None or isinstance(x, (np.ndarray, np.generic, list, tuple, dict, int, float)):
        return False
    if _is_tensor_like(x):
        return getattr(x.device, "type", "cpu") != "cpu"
    try:
        return isinstance(getattr(x, "__cuda_array_interface__", None), dict)
    except Exception:
        return False


def _dev_restrict(what):
    return ValueError("device array: " + what)


def dev_matrix(x, device=None):
    """(DevMatrix, keep-alive, (rows, cols), stream or None) of a 2-D floating-point array in device memory.

    x: a tensor-like object (duck-typed on data_ptr(), stride() in elements, shape, dtype, device) or any object with
    __cuda_array_interface__ (versions 2 and 3; strides in bytes, None = C-contiguous).  device: the handle's device index, checked
    against the tensor's when it names one.  The `stream` of a version-3 interface is returned (1 = the default stream -> None).
    ValueError, before any device call, for anything not 2-D, an integer / bool / complex dtype, a zero or negative stride, a host
    tensor, a tensor of another device."""
    stream = None
    if _is_tensor_like(x):
        dev = x.device
        if getattr(dev, "type", "cpu") == "cpu":
            raise _dev_restrict("the tensor lives in host memory (device %s); pass it as a host array, or move it to the GPU" % (dev,))
        idx = getattr(dev, "index", None)
        if device is not None and idx is not None and int(idx) != int(device):
            raise _dev_restrict("the tensor lives on device %d, the handle on device %d" % (int(idx), int(device)))
        shape = tuple(int(v) for v in x.shape)
        name = str(x.dtype).split(".")[-1]
        if name not in _DT_NAMES:
            raise _dev_restrict("dtype %s is not supported: float64, float32, float16 or bfloat16 (no integer, bool or complex)" % (x.dtype,))
        dt = _DT_NAMES[name]
        if len(shape) != 2:
            raise _dev_restrict("a %d-D array; the matrix must be 2-D" % len(shape))
        strides = tuple(int(v) for v in x.stride())
        ptr = int(x.data_ptr())
    else:
        try:
            cai = x.__cuda_array_interface__
        except Exception:
            cai = None
        if not isinstance(cai, dict):
            raise _dev_restrict("%s is neither a tensor (data_ptr / stride / shape / dtype / device) nor a __cuda_array_interface__ "
                                "producer" % type(x).__name__)
        if int(cai.get("version", 0)) < 2:
            raise _dev_restrict("__cuda_array_interface__ version %s; versions 2 and 3 are supported" % cai.get("version"))
        shape = tuple(int(v) for v in cai["shape"])
        ts = str(cai["typestr"])
        if ts[:1] == ">" or ts[1:] not in _DT_TYPESTR:
            raise _dev_restrict("typestr %r is not supported: little-endian f8, f4 or f2 (no integer, bool or complex)" % ts)
        dt = _DT_TYPESTR[ts[1:]]
        if len(shape) != 2:
            raise _dev_restrict("a %d-D array; the matrix must be 2-D" % len(shape))
        es = _DT_SIZE[dt]
        if cai.get("strides") is None:
            strides = (shape[1], 1)
        else:
            sb = tuple(int(v) for v in cai["strides"])
            if any(v % es for v in sb):
                raise _dev_restrict("strides %s are not multiples of the %d-byte element" % (sb, es))
            strides = tuple(v // es for v in sb)
        ptr = int(cai["data"][0])
        idx = getattr(getattr(x, "device", None), "id", None)
        if device is not None and isinstance(idx, int) and idx != int(device):
            raise _dev_restrict("the array lives on device %d, the handle on device %d" % (idx, int(device)))
        st = cai.get("stream") if int(cai.get("version", 0)) >= 3 else None
        if st is not None and int(st) != 1:
            stream = int(st)
    if shape[0] < 1 or shape[1] < 1:
        raise _dev_restrict("an empty %d x %d array" % shape)
    if strides[0] < 1 or strides[1] < 1:
        raise _dev_restrict("strides %s (in elements): zero (broadcast / expand) and negative strides are not accepted; make the array "
                            "contiguous first" % (strides,))
    return DevMatrix(ptr, dt, strides[0], strides[1]), x, shape, stream


def _dev_vector(x, name, kinds, device):
    """(pointer, dtype code, length, stream or None) of a contiguous 1-D array in device memory; kinds = "int" or "float"."""
    names, typestrs, wanted = ((_IT_NAMES, _IT_TYPESTR, "int32 or int64") if kinds == "int"
                               else (_DT_NAMES, _DT_TYPESTR, "float64, float32, float16 or bfloat16"))
    stream = None
    if _is_tensor_like(x):
        dev = x.device
        if getattr(dev, "type", "cpu") == "cpu":
            raise _dev_restrict("%s lives in host memory (device %s); pass the matrix as a host sparse object, or move it to the GPU" % (name, dev))
        idx = getattr(dev, "index", None)
        if device is not None and idx is not None and int(idx) != int(device):
            raise _dev_restrict("%s lives on device %d, the handle on device %d" % (name, int(idx), int(device)))
        shape = tuple(int(v) for v in x.shape)
        dn = str(x.dtype).split(".")[-1]
        if dn not in names:
            raise _dev_restrict("%s has dtype %s; it must be %s" % (name, x.dtype, wanted))
        dt = names[dn]
        if len(shape) != 1:
            raise _dev_restrict("%s is a %d-D array; it must be 1-D" % (name, len(shape)))
        stride = int(x.stride()[0])
        ptr = int(x.data_ptr())
    else:
        try:
            cai = x.__cuda_array_interface__
        except Exception:
            cai = None
        if not isinstance(cai, dict):
            raise _dev_restrict("%s (%s) is neither a tensor (data_ptr / stride / shape / dtype / device) nor a __cuda_array_interface__ "
                                "producer" % (name, type(x).__name__))
        if int(cai.get("version", 0)) < 2:
            raise _dev_restrict("__cuda_array_interface__ version %s; versions 2 and 3 are supported" % cai.get("version"))
        shape = tuple(int(v) for v in cai["shape"])
        ts = str(cai["typestr"])
        if ts[:1] == ">" or ts[1:] not in typestrs:
            raise _dev_restrict("%s has typestr %r; it must be %s" % (name, ts, wanted))
        dt = typestrs[ts[1:]]
        if len(shape) != 1:
            raise _dev_restrict("%s is a %d-D array; it must be 1-D" % (name, len(shape)))
        es = int(ts[2:])
        stride = 1 if cai.get("strides") is None else int(cai["strides"][0]) // es if int(cai["strides"][0]) % es == 0 else 0
        ptr = int(cai["data"][0])
        idx = getattr(getattr(x, "device", None), "id", None)
        if device is not None and isinstance(idx, int) and idx != int(device):
            raise _dev_restrict("%s lives on device %d, the handle on device %d" % (name, idx, int(device)))
        st = cai.get("stream") if int(cai.get("version", 0)) >= 3 else None
        if st is not None and int(st) != 1:
            stream = int(st)
    if shape[0] > 1 and stride != 1:
        raise _dev_restrict("%s has stride %d (in elements); it must be contiguous" % (name, stride))
    return ptr, dt, shape[0], stream


def dev_sparse(ptr, idx, val, shape, layout, device=None):
    """(DevSparse, keep-alive, (n, m), stream or None) of a CSC / CSR matrix whose three arrays live in device memory: ptr (m + 1 entries
    for "csc", n + 1 for "csr") and idx (nnz) int32 or int64, val (nnz) any of the four floating types; tensor-like objects or
    __cuda_array_interface__ producers, as dev_matrix takes them.  ValueError, before any device call, for an array that is not 1-D or
    not contiguous, a wrong length, another dtype, a host tensor, a tensor of another device."""
    if layout not in SP_LAYOUTS:
        raise ValueError(f"layout must be 'csc' or 'csr' (got {layout!r})")
    n, m = (int(v) for v in shape)
    if n < 1 or m < 1:
        raise _dev_restrict("an empty %d x %d matrix" % (n, m))
    lines = m if layout == "csc" else n
    pp, pt, pl, s0 = _dev_vector(ptr, "ptr", "int", device)
    ip_, it, il, s1 = _dev_vector(idx, "idx", "int", device)
    vp_, vt, vl, s2 = _dev_vector(val, "val", "float", device)
    if pl != lines + 1:
        raise _dev_restrict("ptr has %d entries; a %s matrix of shape (%d, %d) needs %d" % (pl, layout, n, m, lines + 1))
    if il != vl:
        raise _dev_restrict("idx has %d entries, val has %d" % (il, vl))
    stream = next((s for s in (s0, s1, s2) if s is not None), None)
    return DevSparse(pp, ip_ or None, vp_ or None, pt, it, vt, SP_LAYOUTS[layout], il), (ptr, idx, val), (n, m), stream


def dev_sparse_weights(weights, nnz, shape, layout, device=None):
    """(DevSparse, keep-alive, stream or None) of the weights of a sparse matrix in device memory with nnz stored entries: a 1-D
    floating array of nnz weights in the order of the matrix's values, or a (ptr, idx, val) triple -- a sparse matrix of the same layout
    and shape whose pattern the library compares with the matrix's.  The ValueErrors of dev_sparse, before any device call."""
    if isinstance(weights, (tuple, list)):
        if len(weights) != 3:
            raise _dev_restrict("weights must be a 1-D array of nnz weights or a (ptr, idx, val) triple (got %d items)" % len(weights))
        d, keep, _, stream = dev_sparse(weights[0], weights[1], weights[2], shape, layout, device)
        return d, keep, stream
    if layout not in SP_LAYOUTS:
        raise ValueError(f"layout must be 'csc' or 'csr' (got {layout!r})")
    wp, wt, wl, stream = _dev_vector(weights, "weights", "float", device)
    if wl != int(nnz):
        raise _dev_restrict("weights has %d entries, val has %d" % (wl, int(nnz)))
    return DevSparse(None, None, wp or None, IT_I32, IT_I32, wt, SP_LAYOUTS[layout], wl), weights, stream


def sparse_tensor_parts(A):
    """(ptr, idx, val, shape, layout) of a compressed sparse tensor in device memory -- an object whose `layout` prints as
    torch.sparse_csc or torch.sparse_csr and whose device is not the CPU --, None for anything else; a device tensor of another sparse
    layout (COO, BSR, BSC) is a ValueError.  No tensor library is imported."""
    lay = getattr(A, "layout", None)
    if lay is None or isinstance(A, (np.ndarray, np.generic)) or not hasattr(A, "device"):
        return None
    name = str(lay)
    if not name.startswith("torch.sparse_"):
        return None
    if getattr(A.device, "type", "cpu") == "cpu":
        return None
    if name == "torch.sparse_csc":
        return A.ccol_indices(), A.row_indices(), A.values(), tuple(int(v) for v in A.shape), "csc"
    if name == "torch.sparse_csr":
        return A.crow_indices(), A.col_indices(), A.values(), tuple(int(v) for v in A.shape), "csr"
    raise ValueError(f"a device tensor of layout {name} is not accepted: convert it with A.to_sparse_csc() (or to_sparse_csr()) first")


def is_host_sparse_tensor(A):
    """True for a tensor of a torch sparse layout that lives in host memory (no entry takes one: scipy.sparse is the host form)."""
    lay = getattr(A, "layout", None)
    return (lay is not None and str(lay).startswith("torch.sparse_") and hasattr(A, "device")
            and getattr(A.device, "type", "cpu") == "cpu")


def _tensor_module(x):
    """The already imported tensor library of a tensor (sys.modules lookup: nothing is imported here), or None."""
    import sys
    root = (type(x).__module__ or "").split(".")[0]
    return sys.modules.get(root) if root == "torch" else None


def _stream_of(x, stream):
    """hipStream_t (int or None) for a call on x: an explicit stream (an int, or an object with cuda_stream), else the tensor library's
    current stream of x's device."""
    if stream is not None:
        return int(getattr(stream, "cuda_stream", stream)) or None
    mod = _tensor_module(x) if x is not None and _is_tensor_like(x) else None
    if mod is None:
        return None
    return int(mod.cuda.current_stream(x.device).cuda_stream) or None


def _vec3(v):
    return np.array(v, dtype=np.float64).reshape(3)


def make_callbacks(unif_rand=None, print_fn=None, warning=None, progress=None, check_interrupt=None):
    """Build an nnlm_callbacks struct from Python callables (kept alive by the returned object)."""
    cb = Callbacks()
    keep = []

    def wrap(ftype, fn, adapt):
        if fn is None:
            return ftype()
        f = ftype(adapt(fn))
        keep.append(f)
        return f

    fields = dict(Callbacks._fields_)
    cb.check_interrupt = wrap(fields["check_interrupt"], check_interrupt, lambda fn: (lambda ctx: int(bool(fn()))))
    cb.progress = wrap(fields["progress"], progress, lambda fn: (lambda ctx, d, t: fn(d, t)))
    cb.print = wrap(fields["print"], print_fn, lambda fn: (lambda ctx, s: fn(s.decode())))
    cb.warning = wrap(fields["warning"], warning, lambda fn: (lambda ctx, s: fn(s.decode())))
    cb.unif_rand = wrap(fields["unif_rand"], unif_rand, lambda fn: (lambda ctx: float(fn())))
    cb._keep = keep
    return cb


# ----------------------------------------------------------------------------------------------
# one-shot entries: same argument lists as the reference's c_nnmf / c_nnlm
# ----------------------------------------------------------------------------------------------
def c_nnmf(A, k, W, H, Wm, Hm, alpha, beta, max_iter, rel_tol, n_threads, verbose, show_warning,
           inner_max_iter, inner_rel_tol, method, trace, callbacks=None):
    """.Call('_NNLM_c_nnmf', ...) equivalent (reference src/RcppExports.cpp:29-54) -> named list as dict."""
    lib = load()
    A = _f64(A)
    n, m = A.shape
    return _nnmf(lib.nnlm_c_nnmf, (_dp(A), n, m), n, m, k, W, H, Wm, Hm, alpha, beta, max_iter, rel_tol, n_threads, verbose,
                 show_warning, inner_max_iter, inner_rel_tol, method, trace, callbacks)


def _nnmf(entry, lead, n, m, k, W, H, Wm, Hm, alpha, beta, max_iter, rel_tol, n_threads, verbose, show_warning, inner_max_iter,
          inner_rel_tol, method, trace, callbacks):
    """The body of the c_nnmf entries: lead = the entry's matrix arguments (in front of k)."""
    lib = load()
    k = int(k)
    Wi = _f64(W, (n, k)) if W is not None and np.size(W) > 0 else None
    Hi = _f64(H, (k, m)) if H is not None and np.size(H) > 0 else None
    Wm_, Hm_ = _lgl(Wm, (n, k)), _lgl(Hm, (k, m))
    al, be = _vec3(alpha), _vec3(beta)
    cap = lib.nnlm_trace_capacity(int(max_iter), int(trace) if int(trace) > 0 else 1)
    Wo = np.zeros((n, k), order="F")
    Ho = np.zeros((k, m), order="F")
    mse, mkl, terr, ep = (np.zeros(cap) for _ in range(4))
    n_trace, n_it, warned = C.c_int(0), C.c_uint(0), C.c_int(0)
    rc = entry(*lead, k, _dp(Wi), _dp(Hi), _ip(Wm_), _ip(Hm_), _dp(al), _dp(be), int(max_iter),
               float(rel_tol), int(n_threads), int(verbose), int(bool(show_warning)), int(inner_max_iter),
               float(inner_rel_tol), int(method), int(trace) & 0xFFFFFFFF, _dp(Wo), _dp(Ho), _dp(mse), _dp(mkl),
               _dp(terr), _dp(ep), C.byref(n_trace), C.byref(n_it), C.byref(warned),
               C.byref(callbacks) if callbacks is not None else None)
    _check(rc)
    e = n_trace.value
    return dict(W=np.ascontiguousarray(Wo), H=np.ascontiguousarray(Ho), mse_error=mse[:e].copy(), mkl_error=mkl[:e].copy(),
                target_error=terr[:e].copy(), average_epoch=ep[:e].copy(), n_iteration=int(n_it.value),
                warning=bool(warned.value))


def _batch_ranks(ks):
    ks = np.asarray(ks, dtype=np.int64).ravel()
    if ks.size < 1 or ks.size > BATCH_MAX or np.any(ks < 1):
        raise NnlmError(ERR_ARG, f"a batch needs 1..{BATCH_MAX} members of rank >= 1 (got ranks {ks.tolist()})")
    return np.ascontiguousarray(ks, dtype=np.uint32)


def _batch_blocks(X, shapes, what):
    """Member blocks -> their column-major concatenation (the layout of nnlm_set_factors_batch), or None."""
    if X is None:
        return None
    if len(X) != len(shapes):
        raise NnlmError(ERR_ARG, f"{what}: {len(X)} blocks for {len(shapes)} members")
    out = []
    for b, (x, shp) in enumerate(zip(X, shapes)):
        x = np.asarray(x, dtype=np.float64)
        if x.shape != shp:
            raise NnlmError(ERR_ARG, f"{what}[{b}] has shape {x.shape}, member {b} needs {shp}")
        out.append(x.ravel(order="F"))
    return np.ascontiguousarray(np.concatenate(out))


def _batch_split(Wc, Hc, ks, n, m):
    Ws, Hs, wo, ho = [], [], 0, 0
    for k in (int(v) for v in ks):
        Ws.append(np.ascontiguousarray(Wc[wo:wo + n * k].reshape((n, k), order="F")))
        Hs.append(np.ascontiguousarray(Hc[ho:ho + k * m].reshape((k, m), order="F")))
        wo, ho = wo + n * k, ho + k * m
    return Ws, Hs


def _batch_traces(ks, cap, mse, mkl, terr, ep, n_trace, n_it, warned):
    out = []
    for b in range(len(ks)):
        e, s = int(n_trace[b]), slice(b * cap, b * cap + int(n_trace[b]))
        out.append(dict(mse_error=mse[s].copy(), mkl_error=mkl[s].copy(), target_error=terr[s].copy(), average_epoch=ep[s].copy(),
                        n_iteration=int(n_it[b]), warning=bool(warned[b])))
        assert len(out[-1]["mse_error"]) == e
    return out


def _pattern_arrays(indptr, indices):
    """A hold-out pattern in the types of the C ABI (int64 pointers, int32 row indices); the library validates it."""
    return np.ascontiguousarray(indptr, dtype=np.int64), np.ascontiguousarray(indices, dtype=np.int32)


def c_nnmf_holdout_batch(A, indptr, indices, ks, W, H, alpha, beta, max_iter, rel_tol, n_threads, verbose, show_warning, inner_max_iter,
                         inner_rel_tol, method, trace, callbacks=None):
    """c_nnmf_batch on A with the CSC pattern (indptr[m + 1], indices) held out (nnlm_c_nnmf_holdout_batch): each member's dict also
    carries holdout_mse and holdout_mkl, the errors of its final factors on the held-out entries."""
    ptr, idx = _pattern_arrays(indptr, indices)
    return c_nnmf_batch(A, ks, W, H, alpha, beta, max_iter, rel_tol, n_threads, verbose, show_warning, inner_max_iter, inner_rel_tol,
                        method, trace, callbacks, _holdout=(ptr, idx))


def c_nnmf_csc_batch(indptr, indices, data, shape, ks, W, H, alpha, beta, max_iter, rel_tol, n_threads, verbose, show_warning,
                     inner_max_iter, inner_rel_tol, method, trace, callbacks=None):
    """c_nnmf_batch on a sparse A given as canonical CSC arrays (indptr[m+1], indices, data) of shape (n, m), absent entries zeros
    (nnlm_c_nnmf_csc_batch): one SpMM per half-step and one walk over the non-zeros per trace iteration for all members."""
    n, m = (int(v) for v in shape)
    ptr, idx, val = _csc_arrays(indptr, indices, data)
    return c_nnmf_batch(None, ks, W, H, alpha, beta, max_iter, rel_tol, n_threads, verbose, show_warning, inner_max_iter, inner_rel_tol,
                        method, trace, callbacks, _csc=(n, m, ptr, idx, val))


def c_nnmf_csc_kl_batch(indptr, indices, data, shape, ks, W, H, alpha, beta, max_iter, rel_tol, n_threads, verbose, show_warning,
                        inner_max_iter, inner_rel_tol, method, trace, callbacks=None):
    """c_nnmf_csc_batch through nnlm_set_matrix_csc_kl_batch (nnlm_c_nnmf_csc_kl_batch): all four methods (KL loss over the stored
    entries; stored values >= 0); per KL half-step one solver launch over the short lines for all members."""
    n, m = (int(v) for v in shape)
    ptr, idx, val = _csc_arrays(indptr, indices, data)
    return c_nnmf_batch(None, ks, W, H, alpha, beta, max_iter, rel_tol, n_threads, verbose, show_warning, inner_max_iter, inner_rel_tol,
                        method, trace, callbacks, _csc=(n, m, ptr, idx, val), _csc_kl=True)


def c_nnmf_csc_missing_batch(indptr, indices, data, shape, ks, W, H, alpha, beta, max_iter, rel_tol, n_threads, verbose, show_warning,
                             inner_max_iter, inner_rel_tol, method, trace, callbacks=None, holdout=None):
    """c_nnmf_csc_batch with the absent entries of A MISSING (nnlm_c_nnmf_csc_missing_batch).  holdout: None or a CSC pattern
    (indptr[m + 1], indices), a subset of the stored pattern, kept out of the fit.  Every member's dict carries holdout_mse and
    holdout_mkl (NaN without a hold-out set or with an empty one)."""
    n, m = (int(v) for v in shape)
    ptr, idx, val = _csc_arrays(indptr, indices, data)
    ho = _holdout_pattern(holdout, m)
    return c_nnmf_batch(None, ks, W, H, alpha, beta, max_iter, rel_tol, n_threads, verbose, show_warning, inner_max_iter, inner_rel_tol,
                        method, trace, callbacks, _csc=(n, m, ptr, idx, val), _csc_missing=(ho,))


def _holdout_pattern(holdout, m):
    """None, or the (indptr, indices) of a hold-out pattern over m columns in the types of the C ABI."""
    if holdout is None:
        return None
    ptr, idx = _pattern_arrays(*holdout)
    if ptr.size != m + 1:
        raise NnlmError(ERR_ARG, f"the hold-out pattern has {ptr.size} column pointers, A has {m} columns")
    if idx.size < int(ptr[-1]):
        raise NnlmError(ERR_ARG, "the hold-out pattern has fewer row indices than its last column pointer")
    return ptr, idx


def c_nnmf_batch(A, ks, W, H, alpha, beta, max_iter, rel_tol, n_threads, verbose, show_warning, inner_max_iter, inner_rel_tol, method,
                 trace, callbacks=None, _holdout=None, _csc=None, _csc_missing=None, _csc_kl=False):
    """Batched c_nnmf (nnlm_c_nnmf_batch): member b has rank ks[b] and starts from W[b] (n x k_b), H[b] (k_b x m) -- either list may
    be None for the library's default init.  Returns one c_nnmf-style dict per member."""
    lib = load()
    if _csc is None:
        A = _f64(A)
        n, m = A.shape
    else:
        n, m = _csc[:2]
    ks = _batch_ranks(ks)
    Wc = _batch_blocks(W, [(n, int(k)) for k in ks], "W")
    Hc = _batch_blocks(H, [(int(k), m) for k in ks], "H")
    B, K = len(ks), int(ks.sum())
    al, be = _vec3(alpha), _vec3(beta)
    cap = lib.nnlm_trace_capacity(int(max_iter), int(trace) if int(trace) > 0 else 1)
    Wo, Ho = np.zeros(n * K), np.zeros(K * m)
    mse, mkl, terr, ep = (np.zeros(B * cap) for _ in range(4))
    n_trace, warned = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    n_it = np.zeros(B, dtype=np.uint32)
    args = [B, ks.ctypes.data_as(C.POINTER(C.c_uint)), _dp(Wc), _dp(Hc), _dp(al), _dp(be), int(max_iter),
            float(rel_tol), int(n_threads), int(verbose), int(bool(show_warning)), int(inner_max_iter), float(inner_rel_tol),
            int(method), int(trace) & 0xFFFFFFFF, _dp(Wo), _dp(Ho), _dp(mse), _dp(mkl), _dp(terr), _dp(ep), _ip(n_trace),
            n_it.ctypes.data_as(C.POINTER(C.c_uint)), _ip(warned)]
    cbp = C.byref(callbacks) if callbacks is not None else None
    if _csc_missing is not None:
        ho = _csc_missing[0]
        hmse, hmkl = np.zeros(B), np.zeros(B)
        rc = lib.nnlm_c_nnmf_csc_missing_batch(n, m, _lp(_csc[2]), _ip(_csc[3]), _dp(_csc[4]), _lp(ho[0]) if ho else None,
                                               _ip(ho[1]) if ho else None, *args, _dp(hmse), _dp(hmkl), cbp)
    elif _csc is not None:
        entry = lib.nnlm_c_nnmf_csc_kl_batch if _csc_kl else lib.nnlm_c_nnmf_csc_batch
        rc = entry(n, m, _lp(_csc[2]), _ip(_csc[3]), _dp(_csc[4]), *args, cbp)
    elif _holdout is None:
        rc = lib.nnlm_c_nnmf_batch(_dp(A), n, m, *args, cbp)
    else:
        hmse, hmkl = np.zeros(B), np.zeros(B)
        rc = lib.nnlm_c_nnmf_holdout_batch(_dp(A), n, m, _lp(_holdout[0]), _ip(_holdout[1]), *args, _dp(hmse), _dp(hmkl), cbp)
    _check(rc)
    out = _batch_traces(ks, cap, mse, mkl, terr, ep, n_trace, n_it, warned)
    for o, Wb, Hb in zip(out, *_batch_split(Wo, Ho, ks, n, m)):
        o["W"], o["H"] = Wb, Hb
    if _holdout is not None or _csc_missing is not None:
        for b, o in enumerate(out):
            o["holdout_mse"], o["holdout_mkl"] = float(hmse[b]), float(hmkl[b])
    return out


def c_nnlm(x, y, alpha, mask, beta0, max_iter, rel_tol, n_threads, method, callbacks=None):
    """.Call('_NNLM_c_nnlm', ...) equivalent (reference src/RcppExports.cpp:10-27)."""
    lib = load()
    x = _f64(x)
    n, p = x.shape
    y = _f64(np.asarray(y, dtype=np.float64).reshape(n, -1))
    q = y.shape[1]
    return _nnlm(lib.nnlm_c_nnlm, (_dp(x), _dp(y), n, p, q), p, q, alpha, mask, beta0, max_iter, rel_tol, n_threads, method, callbacks)


def _nnlm(entry, lead, p, q, alpha, mask, beta0, max_iter, rel_tol, n_threads, method, callbacks):
    """The body of the c_nnlm entries: lead = the entry's arguments in front of alpha (x, y and the shape)."""
    b0 = _f64(beta0, (p, q)) if beta0 is not None and np.size(beta0) > 0 else None
    mk = _lgl(mask, (p, q))
    al = _vec3(alpha)
    coef = np.zeros((p, q), order="F")
    nit = C.c_int(0)
    rc = entry(*lead, _dp(al), _ip(mk), _dp(b0), int(max_iter), float(rel_tol), int(n_threads), int(method), _dp(coef), C.byref(nit),
               C.byref(callbacks) if callbacks is not None else None)
    _check(rc)
    return dict(coefficient=np.ascontiguousarray(coef), n_iteration=int(nit.value))


def c_nnmf_csc(indptr, indices, data, shape, k, W, H, Wm, Hm, alpha, beta, max_iter, rel_tol, n_threads, verbose, show_warning,
               inner_max_iter, inner_rel_tol, method, trace, callbacks=None):
    """c_nnmf on a sparse A given as canonical CSC arrays (indptr[m+1], indices, data) of shape (n, m); square loss (methods 1, 2)."""
    return _nnmf_csc(load().nnlm_c_nnmf_csc, indptr, indices, data, shape, k, W, H, Wm, Hm, alpha, beta, max_iter, rel_tol, n_threads,
                     verbose, show_warning, inner_max_iter, inner_rel_tol, method, trace, callbacks)


def c_nnmf_csc_missing(indptr, indices, data, shape, k, W, H, Wm, Hm, alpha, beta, max_iter, rel_tol, n_threads, verbose, show_warning,
                       inner_max_iter, inner_rel_tol, method, trace, callbacks=None):
    """c_nnmf_csc with the absent entries of A missing (every stored entry, zeros included, is an observation); k <= 64."""
    return _nnmf_csc(load().nnlm_c_nnmf_csc_missing, indptr, indices, data, shape, k, W, H, Wm, Hm, alpha, beta, max_iter, rel_tol,
                     n_threads, verbose, show_warning, inner_max_iter, inner_rel_tol, method, trace, callbacks)


def c_nnmf_csc_kl(indptr, indices, data, shape, k, W, H, Wm, Hm, alpha, beta, max_iter, rel_tol, n_threads, verbose, show_warning,
                  inner_max_iter, inner_rel_tol, method, trace, callbacks=None):
    """c_nnmf_csc through nnlm_set_matrix_csc_kl: all four methods (KL loss over the stored entries; k <= 64, stored values >= 0)."""
    return _nnmf_csc(load().nnlm_c_nnmf_csc_kl, indptr, indices, data, shape, k, W, H, Wm, Hm, alpha, beta, max_iter, rel_tol,
                     n_threads, verbose, show_warning, inner_max_iter, inner_rel_tol, method, trace, callbacks)


def _weights(weights, nnz):
    """One fp64 weight per stored entry, in the order of the values (the library checks the values themselves)."""
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
    if w.size != nnz:
        raise ValueError("weights has %d entries, the matrix stores %d" % (w.size, nnz))
    return w


def c_nnmf_csc_weighted(indptr, indices, data, weights, absent_missing, shape, k, W, H, Wm, Hm, alpha, beta, max_iter, rel_tol, n_threads,
                        verbose, show_warning, inner_max_iter, inner_rel_tol, method, trace, callbacks=None):
    """c_nnmf_csc with one weight >= 0 per stored entry (in the order of data).  absent_missing: an absent entry is missing (True:
    weighted NMF on the stored entries) or a zero of weight 1 (False: implicit feedback).  Methods 1 and 2, k <= 64."""
    wt = _weights(weights, np.size(data))
    return _nnmf_csc(load().nnlm_c_nnmf_csc_weighted, indptr, indices, data, shape, k, W, H, Wm, Hm, alpha, beta, max_iter, rel_tol,
                     n_threads, verbose, show_warning, inner_max_iter, inner_rel_tol, method, trace, callbacks,
                     _extra=(_dp(wt), 1 if absent_missing else 0))


def _nnmf_csc(entry, indptr, indices, data, shape, k, W, H, Wm, Hm, alpha, beta, max_iter, rel_tol, n_threads, verbose, show_warning,
              inner_max_iter, inner_rel_tol, method, trace, callbacks, _extra=()):
    n, m = (int(v) for v in shape)
    ptr, idx, val = _csc_arrays(indptr, indices, data)
    return _nnmf(entry, (n, m, _lp(ptr), _ip(idx), _dp(val)) + tuple(_extra), n, m, k, W, H, Wm, Hm, alpha, beta, max_iter, rel_tol, n_threads, verbose,
                 show_warning, inner_max_iter, inner_rel_tol, method, trace, callbacks)


def c_nnlm_csc(x, y_indptr, y_indices, y_data, y_shape, alpha, mask, beta0, max_iter, rel_tol, n_threads, method, callbacks=None):
    """c_nnlm with a sparse y (canonical CSC arrays of shape (n, q)); x stays dense; square loss (methods 1, 2)."""
    return _nnlm_csc(load().nnlm_c_nnlm_csc, x, y_indptr, y_indices, y_data, y_shape, alpha, mask, beta0, max_iter, rel_tol, n_threads,
                     method, callbacks)


def c_nnlm_csc_missing(x, y_indptr, y_indices, y_data, y_shape, alpha, mask, beta0, max_iter, rel_tol, n_threads, method, callbacks=None):
    """c_nnlm_csc with the absent entries of y missing (the recommender's fold-in of new columns); p <= 64."""
    return _nnlm_csc(load().nnlm_c_nnlm_csc_missing, x, y_indptr, y_indices, y_data, y_shape, alpha, mask, beta0, max_iter, rel_tol,
                     n_threads, method, callbacks)


def c_nnlm_csc_kl(x, y_indptr, y_indices, y_data, y_shape, alpha, mask, beta0, max_iter, rel_tol, n_threads, method, callbacks=None):
    """c_nnlm_csc through nnlm_set_matrix_csc_kl: all four methods (KL loss over the stored entries; p <= 64, stored values >= 0)."""
    return _nnlm_csc(load().nnlm_c_nnlm_csc_kl, x, y_indptr, y_indices, y_data, y_shape, alpha, mask, beta0, max_iter, rel_tol,
                     n_threads, method, callbacks)


def c_nnlm_csc_weighted(x, y_indptr, y_indices, y_data, weights, absent_missing, y_shape, alpha, mask, beta0, max_iter, rel_tol, n_threads,
                        method, callbacks=None):
    """c_nnlm_csc with one weight >= 0 per stored entry of y (absent_missing as in c_nnmf_csc_weighted): the weighted fold-in; p <= 64."""
    wt = _weights(weights, np.size(y_data))
    return _nnlm_csc(load().nnlm_c_nnlm_csc_weighted, x, y_indptr, y_indices, y_data, y_shape, alpha, mask, beta0, max_iter, rel_tol,
                     n_threads, method, callbacks, _extra=(_dp(wt), 1 if absent_missing else 0))


def _nnlm_csc(entry, x, y_indptr, y_indices, y_data, y_shape, alpha, mask, beta0, max_iter, rel_tol, n_threads, method, callbacks, _extra=()):
    x = _f64(x)
    n, p = x.shape
    if int(y_shape[0]) != n:
        raise ValueError("y has %d rows, x has %d" % (int(y_shape[0]), n))
    q = int(y_shape[1])
    ptr, idx, val = _csc_arrays(y_indptr, y_indices, y_data)
    return _nnlm(entry, (_dp(x), n, p, q, _lp(ptr), _ip(idx), _dp(val)) + tuple(_extra), p, q, alpha, mask, beta0, max_iter, rel_tol, n_threads, method,
                 callbacks)


# ----------------------------------------------------------------------------------------------
# resident API
# ----------------------------------------------------------------------------------------------
class Handle:
    """Device-resident problem (A stays in HBM across calls)."""

    def __init__(self, device=0, precision=PREC_F32):
        self._lib = load()
        self._h = C.c_void_p()
        _check(self._lib.nnlm_create(C.byref(self._h), int(device), int(precision)))
        self.device = int(device)
        self.n = self.m = self.k = 0

    def close(self):
        if getattr(self, "_h", None):
            self._lib.nnlm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _ck(self, rc):
        _check(rc, self._h)

    def set_matrix(self, A):
        A = _f64(A)
        self.n, self.m = A.shape
        self._ck(self._lib.nnlm_set_matrix(self._h, _dp(A), self.n, self.m))

    def set_matrix_csc(self, indptr, indices, data, shape):
        """Sparse A of shape (n, m) as CSC arrays (canonical: see nnlm_set_matrix_csc; absent entries are zeros)."""
        ptr, idx, val = _csc_arrays(indptr, indices, data)
        n, m = (int(v) for v in shape)
        self._ck(self._lib.nnlm_set_matrix_csc(self._h, n, m, _lp(ptr), _ip(idx), _dp(val)))
        self.n, self.m = n, m

    def set_matrix_csc_batch(self, indptr, indices, data, shape):
        """set_matrix_csc for restarts and rank sweeps: the same sparse handle, which also accepts set_factors_batch / run_batch."""
        ptr, idx, val = _csc_arrays(indptr, indices, data)
        n, m = (int(v) for v in shape)
        self._ck(self._lib.nnlm_set_matrix_csc_batch(self._h, n, m, _lp(ptr), _ip(idx), _dp(val)))
        self.n, self.m = n, m

    def set_matrix_csc_kl(self, indptr, indices, data, shape):
        """set_matrix_csc for KL loss: stored values >= 0; the handle also runs methods 3 and 4 (over the stored entries, rank <= 64)."""
        ptr, idx, val = _csc_arrays(indptr, indices, data)
        n, m = (int(v) for v in shape)
        self._ck(self._lib.nnlm_set_matrix_csc_kl(self._h, n, m, _lp(ptr), _ip(idx), _dp(val)))
        self.n, self.m = n, m

    def set_matrix_csc_kl_batch(self, indptr, indices, data, shape):
        """set_matrix_csc_kl for restarts and rank sweeps: the same sparse KL handle, which also accepts set_factors_batch / run_batch
        with all four methods."""
        ptr, idx, val = _csc_arrays(indptr, indices, data)
        n, m = (int(v) for v in shape)
        self._ck(self._lib.nnlm_set_matrix_csc_kl_batch(self._h, n, m, _lp(ptr), _ip(idx), _dp(val)))
        self.n, self.m = n, m

    def set_matrix_csc_missing(self, indptr, indices, data, shape):
        """Sparse A of shape (n, m) as CSC arrays whose absent entries are MISSING: every stored entry, zeros included, is an observation."""
        ptr, idx, val = _csc_arrays(indptr, indices, data)
        n, m = (int(v) for v in shape)
        self._ck(self._lib.nnlm_set_matrix_csc_missing(self._h, n, m, _lp(ptr), _ip(idx), _dp(val)))
        self.n, self.m = n, m

    def set_matrix_csc_weighted(self, indptr, indices, data, weights, shape, absent_missing=True):
        """Sparse A of shape (n, m) as CSC arrays with one weight >= 0 per stored entry (in the order of data; None: a NULL pointer, which
        the library refuses).  absent_missing: an absent entry is missing (True) or a zero of weight 1 (False)."""
        ptr, idx, val = _csc_arrays(indptr, indices, data)
        wt = None if weights is None else _weights(weights, val.size)
        n, m = (int(v) for v in shape)
        self._ck(self._lib.nnlm_set_matrix_csc_weighted(self._h, n, m, _lp(ptr), _ip(idx), _dp(val), _dp(wt), 1 if absent_missing else 0))
        self.n, self.m = n, m

    def set_matrix_csc_missing_batch(self, indptr, indices, data, shape, holdout=None):
        """set_matrix_csc_missing for restarts, rank sweeps and rank selection: the same sparse-missing handle (of the entries left after
        taking out the optional hold-out pattern holdout = (indptr[m + 1], indices), a subset of the stored pattern), which also accepts
        set_factors_batch / run_batch and, with a hold-out set, holdout_errors."""
        ptr, idx, val = _csc_arrays(indptr, indices, data)
        n, m = (int(v) for v in shape)
        ho = _holdout_pattern(holdout, m)
        self._ck(self._lib.nnlm_set_matrix_csc_missing_batch(self._h, n, m, _lp(ptr), _ip(idx), _dp(val), _lp(ho[0]) if ho else None,
                                                             _ip(ho[1]) if ho else None))
        self.n, self.m = n, m

    def set_matrix_holdout(self, A, indptr, indices):
        """Dense finite A with the CSC pattern (indptr[m + 1], indices) held out: the handle of set_matrix(A with NaN at the pattern) that
        also keeps the held-out entries (holdout_errors) and is accepted by the batch entries."""
        A = _f64(A)
        ptr, idx = _pattern_arrays(indptr, indices)
        n, m = A.shape
        if ptr.size != m + 1:
            raise NnlmError(ERR_ARG, f"the hold-out pattern has {ptr.size} column pointers, A has {m} columns")
        if idx.size < (int(ptr[-1]) if ptr.size else 0):
            raise NnlmError(ERR_ARG, "the hold-out pattern has fewer row indices than its last column pointer")
        self._ck(self._lib.nnlm_set_matrix_holdout(self._h, _dp(A), n, m, _lp(ptr), _ip(idx)))
        self.n, self.m = n, m

    def set_matrix_device(self, x, stream=None):
        """set_matrix for a matrix in device memory (see dev_matrix): no copy through the host, any of fp64 / fp32 / fp16 / bf16, any
        non-overlapping strides.  stream: the hipStream_t (or an object with cuda_stream) that produced x; None = the tensor library's
        current stream for x's device (a tensor), the interface's own stream (__cuda_array_interface__ version 3) or the default stream."""
        d, keep, (n, m), st = dev_matrix(x, self.device)
        st = _stream_of(x, stream) if (stream is not None or st is None) else st
        self._ck(self._lib.nnlm_set_matrix_device(self._h, C.byref(d), n, m, C.c_void_p(st)))
        self.n, self.m = n, m
        del keep

    def set_matrix_sparse_device(self, ptr, idx, val, shape, layout="csc", absent="zero", kl=False, batch=False, stream=None):
        """A sparse matrix of shape (n, m) whose CSC / CSR arrays live in device memory (see dev_sparse): validated, transposed and
        converted by kernels, nothing of size nnz crosses to the host.  absent = "zero" | "missing", kl and batch choose the host entry
        whose handle this leaves (set_matrix_csc, _missing, _kl, each with or without _batch).  stream: as for set_matrix_device."""
        if absent not in ("zero", "missing"):
            raise ValueError(f"absent must be 'zero' or 'missing' (got {absent!r})")
        d, keep, (n, m), st = dev_sparse(ptr, idx, val, shape, layout, self.device)
        st = _stream_of(val if _is_tensor_like(val) else None, stream) if (stream is not None or st is None) else st
        door = (SP_ABSENT_MISSING if absent == "missing" else 0) | (SP_KL if kl else 0) | (SP_BATCH if batch else 0)
        self._ck(self._lib.nnlm_set_matrix_sparse_device(self._h, C.byref(d), n, m, door, C.c_void_p(st)))
        self.n, self.m = n, m
        del keep

    def set_matrix_sparse_device_weighted(self, ptr, idx, val, weights, shape, layout="csc", absent="missing", stream=None):
        """set_matrix_csc_weighted for a sparse matrix AND its weights in device memory (see dev_sparse, dev_sparse_weights): weights is
        a 1-D device array of nnz floats in the order of val, or a (ptr, idx, val) triple of the same layout and shape whose pattern the
        library checks against the matrix's.  absent = "missing" | "zero" (a zero of weight 1).  stream: as for set_matrix_device; it
        orders the matrix's arrays and the weights alike."""
        if absent not in ("zero", "missing"):
            raise ValueError(f"absent must be 'zero' or 'missing' (got {absent!r})")
        d, keep, (n, m), st = dev_sparse(ptr, idx, val, shape, layout, self.device)
        dw, keepw, stw = dev_sparse_weights(weights, d.nnz, (n, m), layout, self.device)
        st = st if st is not None else stw
        st = _stream_of(val if _is_tensor_like(val) else None, stream) if (stream is not None or st is None) else st
        self._ck(self._lib.nnlm_set_matrix_sparse_device_weighted(self._h, C.byref(d), C.byref(dw), n, m, 1 if absent == "missing" else 0,
                                                                  C.c_void_p(st)))
        self.n, self.m = n, m
        del keep, keepw

    def debug_sparse_resident_weighted(self, side):
        """(weights fp64, weights * values fp64) of the resident weighted sparse matrix, in the order of side 0 (by columns) or 1 (by rows)."""
        nnz = max(int(self.get_info("matrix_nnz")), 0)
        wt, wa = np.zeros(nnz, dtype=np.float64), np.zeros(nnz, dtype=np.float64)
        self._ck(self._lib.nnlm_debug_sparse_resident_weighted(self._h, int(side), _dp(wt), _dp(wa)))
        return wt, wa

    def debug_sparse_resident(self, side):
        """(ptr int64, idx int32, val fp64) of the resident sparse matrix: side 0 by columns (idx = rows), side 1 by rows."""
        side = int(side)
        nnz = int(self.get_info("matrix_nnz"))
        if nnz < 0:
            raise NnlmError(ERR_ARG, "debug_sparse_resident: the handle holds no sparse matrix")
        ptr = np.zeros((self.m if side == 0 else self.n) + 1, dtype=np.int64)
        idx, val = np.zeros(nnz, dtype=np.int32), np.zeros(nnz, dtype=np.float64)
        self._ck(self._lib.nnlm_debug_sparse_resident(self._h, side, _lp(ptr), _ip(idx), _dp(val)))
        return ptr, idx, val

    def set_factors_device(self, k, W=None, H=None, Wm=None, Hm=None, stream=None):
        """set_factors with W (n x k) and H (k x m) in device memory; None = zeros; the masks are host arrays."""
        k = int(k)
        dW = dev_matrix(W, self.device) if W is not None else None
        dH = dev_matrix(H, self.device) if H is not None else None
        for d, shp, nm in ((dW, (self.n, k), "W"), (dH, (k, self.m), "H")):
            if d is not None and d[2] != shp:
                raise NnlmError(ERR_ARG, f"{nm} has shape {d[2]}, rank {k} needs {shp}")
        first = W if W is not None else H
        st = _stream_of(first, stream)
        self.k = k
        self._batch = False
        self._ck(self._lib.nnlm_set_factors_device(self._h, k, C.byref(dW[0]) if dW else None, C.byref(dH[0]) if dH else None,
                                                   _ip(_lgl(Wm, (self.n, k))), _ip(_lgl(Hm, (k, self.m))), C.c_void_p(st)))

    def get_factors_device(self, W_out, H_out, stream=None):
        """The current factors into the caller's device buffers (fp64 or fp32; n x k and k x m; either may be None).  Asynchronous: the
        caller's stream is made to wait for the export."""
        dW = dev_matrix(W_out, self.device) if W_out is not None else None
        dH = dev_matrix(H_out, self.device) if H_out is not None else None
        for d, shp, nm in ((dW, (self.n, self.k), "W_out"), (dH, (self.k, self.m), "H_out")):
            if d is not None and d[2] != shp:
                raise NnlmError(ERR_ARG, f"{nm} has shape {d[2]}, the factors need {shp}")
        first = W_out if W_out is not None else H_out
        st = _stream_of(first, stream)
        self._ck(self._lib.nnlm_get_factors_device(self._h, C.byref(dW[0]) if dW else None, C.byref(dH[0]) if dH else None, C.c_void_p(st)))

    def holdout_errors(self):
        """(mse, mkl) arrays over the held-out entries: one value per batch member, or one for solo factors."""
        B = len(self.ks) if getattr(self, "_batch", False) else 1
        mse, mkl = np.zeros(B), np.zeros(B)
        self._ck(self._lib.nnlm_holdout_errors(self._h, _dp(mse), _dp(mkl)))
        return mse, mkl

    def predict_entries(self, rows, cols):
        """(W H)[rows[e], cols[e]] of the current factors as a float64 array; W H is never formed."""
        r, c = index_array(rows, "rows"), index_array(cols, "cols")
        if r.size != c.size:
            raise ValueError(f"rows and cols must have the same length (got {r.size} and {c.size})")
        out = np.zeros(r.size)
        self._ck(self._lib.nnlm_predict_entries(self._h, r.size, _ip(r), _ip(c), _dp(out)))
        return out

    def top_n(self, n_top, by="column", lines=None, exclude=False):
        """(idx int32 [L, n_top], score float64 [L, n_top]): per listed column (by = "column": the best rows) or row (by = "row": the
        best columns) of W H, best first, equal scores by ascending index, (-1, NaN) behind a line with fewer candidates.  lines = None:
        every line of that side.  exclude: the entries stored in the handle's sparse matrix are not candidates."""
        code, n_top = by_code(by), int(n_top)
        ln = None if lines is None else index_array(lines, "lines")
        L = (self.m if code == 0 else self.n) if ln is None else ln.size
        width = min(max(n_top, 0), TOPN_MAX)  # (an n_top out of range is the library's refusal: nothing is written then)
        idx, score = np.full((L, width), -1, dtype=np.int32), np.full((L, width), np.nan)
        self._ck(self._lib.nnlm_top_n(self._h, code, n_top, _ip(ln), L, int(bool(exclude)), _ip(idx), _dp(score)))
        return idx, score

    def top_n_eval(self, cutoffs, by="column", lines=None, exclude=False, held_ptr=None, held_idx=None, per_line=False):
        """Ranking metrics of the top-n lists (n = the last cutoff) against held-out entries; the lists stay on the device.  held_ptr /
        held_idx: the held-out pattern in the orientation of ``by`` (a CSC for "column", a CSR for "row").  Returns dict(cutoffs,
        n_evaluated, precision, recall, hit_rate, ndcg, map, mrr: means over the lines with held-out entries, one value per cutoff)
        and with per_line also n_heldout, first_hit (int64 [L]), hits (int64), dcg, apn (float64) [L, n_cut]."""
        code = by_code(by)
        cut = index_array(np.atleast_1d(np.asarray(cutoffs)), "cutoffs")
        ln = None if lines is None else index_array(lines, "lines")
        L = (self.m if code == 0 else self.n) if ln is None else ln.size
        if held_ptr is None:
            raise ValueError("held_ptr: the held-out pattern is required")
        hp = np.ascontiguousarray(held_ptr, dtype=np.int64)
        hi = index_array([] if held_idx is None else held_idx, "held_idx")
        side = self.m if code == 0 else self.n
        if hp.ndim != 1 or hp.size != side + 1 or (hp.size and hi.size < hp[-1]):
            raise ValueError(f"held_ptr must hold {side + 1} pointers into held_idx (got {hp.shape} and {hi.size} indices)")
        nc = min(cut.size, TOPN_EVAL_MAX_CUT)  # (more cutoffs are the library's refusal: nothing is written then)
        agg, n_eval = np.full((nc, 6), np.nan), C.c_longlong(0)
        rec = np.zeros((L, 2 + 3 * nc)) if per_line else None
        self._ck(self._lib.nnlm_top_n_eval(self._h, code, _ip(cut), cut.size, _ip(ln), L, int(bool(exclude)),
                                           _lp(hp), _ip(hi), _dp(agg), C.byref(n_eval), _dp(rec)))
        out = dict(cutoffs=cut.copy(), n_evaluated=int(n_eval.value))
        for s, name in enumerate(("precision", "recall", "hit_rate", "ndcg", "map", "mrr")):
            out[name] = agg[:, s].copy()
        if per_line:
            body = rec[:, 2:].reshape(L, nc, 3)
            out.update(n_heldout=rec[:, 0].astype(np.int64), first_hit=rec[:, 1].astype(np.int64), hits=body[:, :, 0].astype(np.int64),
                       dcg=body[:, :, 1].copy(), apn=body[:, :, 2].copy())
        return out

    def matrix_info(self):
        nn, am, kc = C.c_double(0), C.c_int(0), C.c_double(0)
        self._ck(self._lib.nnlm_matrix_info(self._h, C.byref(nn), C.byref(am), C.byref(kc)))
        return dict(n_non_missing=nn.value, any_missing=bool(am.value), kl_const=kc.value)

    def set_factors(self, k, W=None, H=None, Wm=None, Hm=None):
        self.k = int(k)
        self._batch = False  # (a solo set ends a batch)
        Wi = _f64(W, (self.n, self.k)) if W is not None else None
        Hi = _f64(H, (self.k, self.m)) if H is not None else None
        self._ck(self._lib.nnlm_set_factors(self._h, self.k, _dp(Wi), _dp(Hi), _ip(_lgl(Wm, (self.n, self.k))),
                                            _ip(_lgl(Hm, (self.k, self.m)))))

    def get_factors(self):
        W = np.zeros((self.n, self.k), order="F")
        H = np.zeros((self.k, self.m), order="F")
        self._ck(self._lib.nnlm_get_factors(self._h, _dp(W), _dp(H)))
        return np.ascontiguousarray(W), np.ascontiguousarray(H)

    def half_step(self, which, reg, inner_max_iter, inner_rel_tol, method):
        r = _vec3(reg)
        self._ck(self._lib.nnlm_half_step(self._h, int(which), _dp(r), int(inner_max_iter), float(inner_rel_tol), int(method)))

    def iterate(self, n_iter, alpha, beta, inner_max_iter, inner_rel_tol, method):
        a, b = _vec3(alpha), _vec3(beta)
        self._ck(self._lib.nnlm_iterate(self._h, int(n_iter), _dp(a), _dp(b), int(inner_max_iter), float(inner_rel_tol), int(method)))

    def run(self, alpha, beta, max_iter, rel_tol, verbose, show_warning, inner_max_iter, inner_rel_tol, method, trace,
            callbacks=None):
        """The resident c_nnmf loop (reference src/nnmf.cpp:100-209); returns the traces as a dict."""
        a, b = _vec3(alpha), _vec3(beta)
        cap = self._lib.nnlm_trace_capacity(int(max_iter), int(trace) if int(trace) > 0 else 1)
        mse, mkl, terr, ep = (np.zeros(cap) for _ in range(4))
        n_trace, n_it, warned = C.c_int(0), C.c_uint(0), C.c_int(0)
        self._ck(self._lib.nnlm_run(self._h, _dp(a), _dp(b), int(max_iter), float(rel_tol), int(verbose), int(bool(show_warning)),
                                    int(inner_max_iter), float(inner_rel_tol), int(method), int(trace) & 0xFFFFFFFF, _dp(mse),
                                    _dp(mkl), _dp(terr), _dp(ep), C.byref(n_trace), C.byref(n_it), C.byref(warned),
                                    C.byref(callbacks) if callbacks is not None else None))
        e = n_trace.value
        return dict(mse_error=mse[:e].copy(), mkl_error=mkl[:e].copy(), target_error=terr[:e].copy(),
                    average_epoch=ep[:e].copy(), n_iteration=int(n_it.value), warning=bool(warned.value))

    def set_factors_batch(self, ks, W=None, H=None):
        """Batched factorisation: member b has rank ks[b] and factors W[b] (n x k_b), H[b] (k_b x m); None = zeros."""
        ks = _batch_ranks(ks)
        Wc = _batch_blocks(W, [(self.n, int(k)) for k in ks], "W")
        Hc = _batch_blocks(H, [(int(k), self.m) for k in ks], "H")
        self._ck(self._lib.nnlm_set_factors_batch(self._h, len(ks), ks.ctypes.data_as(C.POINTER(C.c_uint)), _dp(Wc), _dp(Hc)))
        self.k, self.ks, self._batch = int(ks.sum()), [int(k) for k in ks], True

    def get_factors_batch(self):
        """[(W_b, H_b)] of the members."""
        Wc, Hc = np.zeros(self.n * self.k), np.zeros(self.k * self.m)
        self._ck(self._lib.nnlm_get_factors_batch(self._h, _dp(Wc), _dp(Hc)))
        return list(zip(*_batch_split(Wc, Hc, self.ks, self.n, self.m)))

    def run_batch(self, alpha, beta, max_iter, rel_tol, verbose, show_warning, inner_max_iter, inner_rel_tol, method, trace,
                  callbacks=None):
        """nnlm_run for every member of the batch: one trace dict per member."""
        a, b = _vec3(alpha), _vec3(beta)
        B = len(self.ks)
        cap = self._lib.nnlm_trace_capacity(int(max_iter), int(trace) if int(trace) > 0 else 1)
        mse, mkl, terr, ep = (np.zeros(B * cap) for _ in range(4))
        n_trace, warned = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        n_it = np.zeros(B, dtype=np.uint32)
        self._ck(self._lib.nnlm_run_batch(self._h, _dp(a), _dp(b), int(max_iter), float(rel_tol), int(verbose), int(bool(show_warning)),
                                          int(inner_max_iter), float(inner_rel_tol), int(method), int(trace) & 0xFFFFFFFF, _dp(mse),
                                          _dp(mkl), _dp(terr), _dp(ep), _ip(n_trace), n_it.ctypes.data_as(C.POINTER(C.c_uint)),
                                          _ip(warned), C.byref(callbacks) if callbacks is not None else None))
        return _batch_traces(self.ks, cap, mse, mkl, terr, ep, n_trace, n_it, warned)

    def svd(self, l, power_iters, omega):
        """Truncated SVD of the resident matrix by randomised subspace iteration (nnlm_svd): sketch width l, omega l x m supplied by the
        caller (the library draws nothing).  The decomposition stays on the handle; the handle is left without factors."""
        l = int(l)
        om = _f64(omega)
        if l > 0 and om.size != l * self.m:
            raise NnlmError(ERR_ARG, f"omega has {om.size} entries, a sketch of width {l} needs {l} x {self.m}")
        self._ck(self._lib.nnlm_svd(self._h, l, int(power_iters), _dp(om)))
        self.k, self._batch = 0, False

    def get_svd(self, k):
        """(U n x k, sigma k, Vt k x m) of the resident decomposition."""
        k = int(k)
        s, U, Vt = np.zeros(k), np.zeros((self.n, k), order="F"), np.zeros((k, self.m), order="F")
        self._ck(self._lib.nnlm_get_svd(self._h, k, _dp(s), _dp(U), _dp(Vt)))
        return np.ascontiguousarray(U), s, np.ascontiguousarray(Vt)

    def set_factors_nndsvd(self, k, variant="nndsvd"):
        """NNDSVD start from the first k resident triplets; variant "nndsvd" (zeros stay: not for Lee's updates or KL loss) or "nndsvda"
        (zeros filled with mean(A)), or the C code 0 / 1."""
        v = NNDSVD_VARIANTS[variant] if isinstance(variant, str) else int(variant)
        self._ck(self._lib.nnlm_set_factors_nndsvd(self._h, int(k), v))
        self.k, self._batch = int(k), False

    def set_factors_nndsvd_batch(self, ks, variant="nndsvd"):
        """Batched factorisation whose member b starts from the NNDSVD of the first ks[b] resident triplets."""
        ks = _batch_ranks(ks)
        v = NNDSVD_VARIANTS[variant] if isinstance(variant, str) else int(variant)
        self._ck(self._lib.nnlm_set_factors_nndsvd_batch(self._h, len(ks), ks.ctypes.data_as(C.POINTER(C.c_uint)), v))
        self.k, self.ks, self._batch = int(ks.sum()), [int(k) for k in ks], True

    def take_sweeps(self, reset=True):
        v = C.c_longlong(0)
        self._ck(self._lib.nnlm_take_sweeps(self._h, C.byref(v), int(reset)))
        return int(v.value)

    def errors(self):
        mse, kl = C.c_double(0), C.c_double(0)
        pen = np.zeros(6)
        self._ck(self._lib.nnlm_errors(self._h, C.byref(mse), C.byref(kl), _dp(pen)))
        return mse.value, kl.value, pen

    def sync(self):
        self._ck(self._lib.nnlm_sync(self._h))

    def profile_enable(self, on=True):
        self._ck(self._lib.nnlm_profile_enable(self._h, int(on)))

    def profile_reset(self):
        self._ck(self._lib.nnlm_profile_reset(self._h))

    def profile_get(self, name):
        ms, cnt = C.c_double(0), C.c_longlong(0)
        self._ck(self._lib.nnlm_profile_get(self._h, name.encode(), C.byref(ms), C.byref(cnt)))
        return ms.value, int(cnt.value)

    def comm_init(self, unique_id, rank: int, nranks: int, form="cols"):
        """unique_id=None -> virtual rank (no communicator; partial sums stay un-reduced).  form: "cols" (column-sharded half-steps,
        one all-gather each) or "reduce" (dense square loss: contraction-sharded + all-reduce, then sweep + all-gather)."""
        buf = C.create_string_buffer(bytes(unique_id), COMM_ID_BYTES) if unique_id is not None else None
        self._ck(self._lib.nnlm_comm_init(self._h, buf, int(rank), int(nranks)))
        self.comm_set_form(form)

    def comm_set_form(self, form):
        self._ck(self._lib.nnlm_comm_set_form(self._h, FORMS[form] if isinstance(form, str) else int(form)))

    def get_info(self, key):
        """cus, xprod_waves_w / xprod_waves_h and xprod_splits_w / xprod_splits_h (wavefronts per block and slabs of the last xprod16_tn_kernel
        launch of each side), xprod_splits_err (slabs of the last fused xprod16_err_kernel launch), a_stream_nt_from (first stage whose requests
        for A were non-temporal in the last A-streaming cross product, -1 none yet), sweep_form_w / sweep_form_h (0 plain, 1 persistent -- strict fp64 --, 2 fp32 chain, -1 none yet), sweep_groups_w / sweep_groups_h,
        lee_lanes_w / lee_lanes_h and lee_regs_w / lee_regs_h (L and R of the last sweep_ls_kernel<R, L, 2> launch, -1 none yet),
        kl_form_w / kl_form_h (KL solver of the last half-step: 0 tile, 1 tile on its own starting states, 2 reg64, 3 streaming, -1 none yet),
        kl_pieces_w / kl_pieces_h and kl_cols_w / kl_cols_h (instantiated pieces per thread and columns per block of that launch as in
        kl_plan(); 0 streaming, -1 none yet),
        na_solver_w / na_solver_h and na_solver_kr_w / na_solver_kr_h (missing values: family -- 0 colsolve_row, 1 colsolve_strict, 2
        colsolve_ls, 3 sweep_generic -- and KR of the last per-column solver launch, -1 none yet), na_gram_w / na_gram_h and na_gram_nt_w /
        na_gram_nt_h (family -- 0 na_gram_f16, 1 na_gram_lds, 2 its tail form, 3 sp_gram, 4 na_gram_generic -- and NT of the last
        per-column Gram launch, -1 none yet),
        sp_ingest_check_share / sp_ingest_sort_tile (stored entries per workgroup of the entry check / of a radix pass of
        set_matrix_sparse_device),
        matrix_nnz (-1 for a dense matrix), matrix_bytes, matrix_min_col_observed / matrix_min_row_observed (fewest finite entries of a
        column / a row of a dense matrix),
        svd_width / svd_kept (sketch width of the resident decomposition and directions its last orth kept, -1 none), svd_rotate_form
        (column tile of its last rotation, 0 out of place), svd_ms_cross / svd_ms_gram / svd_ms_rotate / svd_ms_eig / svd_ms_wait /
        svd_ms_setup / svd_ms_total (host milliseconds of the last svd() by phase)."""
        v = C.c_double(0)
        self._ck(self._lib.nnlm_get_info(self._h, key.encode(), C.byref(v)))
        return v.value

    def debug_phase(self, which, phase, reg, inner_max_iter, inner_rel_tol, method):
        r = _vec3(reg)
        self._ck(self._lib.nnlm_debug_phase(self._h, int(which), int(phase), _dp(r), int(inner_max_iter), float(inner_rel_tol), int(method)))

    def debug_partial(self, which):
        cols = self.m if which == 1 else self.n
        G = np.zeros((self.k, self.k), order="F")
        Cm = np.zeros((self.k, cols), order="F")
        self._ck(self._lib.nnlm_debug_partial(self._h, int(which), _dp(G), _dp(Cm)))
        return np.ascontiguousarray(G), np.ascontiguousarray(Cm)

    def comm_info(self):
        r, n = C.c_int(0), C.c_int(0)
        self._ck(self._lib.nnlm_comm_info(self._h, C.byref(r), C.byref(n)))
        return r.value, n.value


def shard_range(n, m, precision, which, rank, nranks):
    """Contraction range [begin, end) of `rank` (pure host function of the C ABI, works without a GPU)."""
    b, e = C.c_int(0), C.c_int(0)
    _check(load().nnlm_shard_range(int(n), int(m), int(precision), int(which), int(rank), int(nranks), C.byref(b), C.byref(e)))
    return b.value, e.value


def shard_cols(ncols, rank, nranks):
    """(cpr, col0, col1): the columns `rank` solves and the packed slab width (pure host function of the C ABI)."""
    cpr, c0, c1 = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(load().nnlm_shard_cols(int(ncols), int(rank), int(nranks), C.byref(cpr), C.byref(c0), C.byref(c1)))
    return cpr.value, c0.value, c1.value


def debug_exchange(handles, which, stage):
    """Host stand-in for ncclAllReduce (stage 1) / ncclAllGather (stage 2) between virtual ranks (test hook)."""
    arr = (C.c_void_p * len(handles))(*[h._h for h in handles])
    _check(load().nnlm_debug_exchange(arr, len(handles), int(which), int(stage)))


def debug_set_cus(cus: int):
    """Test hook: handles created from now on plan their launches for `cus` compute units (0 = the device's own count)."""
    _check(load().nnlm_debug_set_cus(int(cus)))


def debug_set_svd_rotate(form: int):
    """Test hook: form of the rotations of Handle.svd from now on: 32, 16, 8 (column tile, where it fits), 0 (out of place), -1 (the width decides)."""
    _check(load().nnlm_debug_set_svd_rotate(int(form)))


def debug_set_xprod_waves(waves: int):
    """Test hook: handles created from now on run the split-fp16 cross product with 8 or 10 wavefronts per block (0 = the plan decides)."""
    _check(load().nnlm_debug_set_xprod_waves(int(waves)))


A_STREAM_NONE = 2**31 - 1  # debug_set_a_stream: no request for A is non-temporal


def debug_set_a_stream(nt_from_stage: int):
    """Test hook: handles created from now on issue the requests for A of the contraction stages >= nt_from_stage of the A-streaming cross
    products non-temporally (0 = all of A, A_STREAM_NONE = none, -1 = the library's choice).  Results do not depend on it."""
    _check(load().nnlm_debug_set_a_stream(int(nt_from_stage)))


def xprod_plan(ldc, stages, k, cus, force_waves=0):
    """Launch plan of the split-fp16 cross product (pure host function of the C ABI, works without a GPU)."""
    out = (C.c_int * 8)()
    _check(load().nnlm_xprod_plan(int(ldc), int(stages), int(k), int(cus), int(force_waves), out))
    return dict(zip(("waves", "splits", "stages_per_split", "tiles", "blocks", "pieces", "lds_bytes"), list(out)[:7]))


KL_TILE2, KL_TILE1, KL_REG64, KL_STREAM = 0, 1, 2, 3  # "kernel" of kl_plan()


def kl_plan(p, k, precision, mask_words=0):
    """Which KL solver a dense half-step with a contraction of length p takes when its workspaces fit (pure host function of the C ABI,
    works without a GPU): kernel (KL_TILE2 / KL_TILE1 / KL_REG64 / KL_STREAM), exact and instantiated pieces per thread, columns per
    block, dynamic LDS bytes, wavefronts of a block that own a last piece."""
    out = (C.c_int * 8)()
    _check(load().nnlm_kl_plan(int(p), int(k), int(precision), int(mask_words), out))
    return dict(zip(("kernel", "pieces_exact", "pieces", "cols", "lds_bytes", "last_waves"), list(out)[:6]))


def debug_alloc_limit(nbytes: int):
    """Test hook: matrix-sized KL workspaces beyond `nbytes` "do not fit" (0 = no limit) -> the streaming path over column chunks."""
    _check(load().nnlm_debug_alloc_limit(int(nbytes)))


def debug_poison_workspaces(on: int):
    """Test hook: while on, a newly allocated per-column Gram buffer (missing values) is filled with 0xFF bytes -- NaN in every double the
    Gram kernels do not write.  Process-global; reset it in a `finally`."""
    _check(load().nnlm_debug_poison_workspaces(int(on)))


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(load().nnlm_comm_unique_id(buf))
    return buf.raw


def release_caches():
    """Release the process-wide caches of the library (resources of the last destroyed handle, pinned bounce buffers)."""
    _check(load().nnlm_release_caches())
