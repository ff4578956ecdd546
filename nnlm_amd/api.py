"""Host-side mirror of the reference's R interface for the nnmf()/nnlm() path.

Same names, argument meaning, defaults, error and warning behaviour as the R functions, so that the
parity tests read like the reference's own tests:

    nnmf()          <- R/nnmf.R:135-225
    nnlm()          <- R/nnlm.R:70-145
    predict_nnmf()  <- R/nnmf_methods.R:22-48   (S3 predict.nnmf)
    mse_mkl()       <- R/misc.R:9-16
    reformat_input(), get_method_code(), check_matrix() <- R/misc.R:28-129

Compute goes through the C ABI of libnnlm_mi355x.so (nnlm_amd._lib) and nowhere else: there is no
CPU fallback.  The argument normalisation (``prepare_*``) and result decoration (``finish_*``) are
pure host logic and are split out so they can be unit-tested without a GPU.
"""
from __future__ import annotations

import os
import time
import warnings
from collections import namedtuple

import numpy as np

from . import _lib


class NnlmStop(ValueError):
    """R's stop()."""


# ------------------------------------------------------------------------------------------------
# sparse input
# ------------------------------------------------------------------------------------------------
CSC = namedtuple("CSC", "indptr indices data shape")
CSC.__doc__ = "Canonical CSC of a sparse matrix: int64 indptr[m+1], int32 indices (sorted, unique within a column), fp64 data, (n, m)."
CSC.tocsc = lambda self: self  # (a CSC is itself a sparse argument: what holdout_split returns goes into nnmf() and seen=)


def is_sparse(A):
    """Duck typing: anything with tocsc() (scipy sparse matrices and arrays qualify; scipy itself is never imported)."""
    return not isinstance(A, np.ndarray) and callable(getattr(A, "tocsc", None))


def as_csc(A):
    """Canonical CSC of a sparse object (tocsc() yielding indptr, indices, data, shape): duplicates summed (in their stored order), row
    indices sorted within each column.  Explicitly stored zeros are kept (they are zeros either way)."""
    c = A.tocsc()
    n, m = (int(v) for v in c.shape)
    indptr = np.asarray(c.indptr, dtype=np.int64)
    rows = np.asarray(c.indices, dtype=np.int64)
    data = np.asarray(c.data, dtype=np.float64)
    if indptr.shape != (m + 1,) or indptr[0] != 0 or np.any(np.diff(indptr) < 0) or indptr[-1] != rows.size or rows.size != data.size:
        raise NnlmStop("A sparse matrix must have a valid CSC structure (indptr of length ncol + 1, non-decreasing, ending at nnz).")
    if rows.size and (rows.min() < 0 or rows.max() >= n):
        raise NnlmStop("A sparse matrix has a row index out of range.")
    cols = np.repeat(np.arange(m, dtype=np.int64), np.diff(indptr))
    order = np.lexsort((rows, cols))  # (stable: duplicates keep their stored order)
    rows, cols, data = rows[order], cols[order], data[order]
    if rows.size:
        first = np.ones(rows.size, dtype=bool)
        first[1:] = (rows[1:] != rows[:-1]) | (cols[1:] != cols[:-1])
        starts = np.flatnonzero(first)
        data = np.add.reduceat(data, starts)
        rows, cols = rows[starts], cols[starts]
    indptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=m), out=indptr[1:])
    return CSC(indptr, rows.astype(np.int32), np.ascontiguousarray(data), (n, m))


def csc_toarray(c):
    """Dense n x m array of a CSC (host side: small matrices and the error summary of nnlm())."""
    n, m = c.shape
    out = np.zeros((n, m))
    cols = np.repeat(np.arange(m), np.diff(c.indptr))
    out[np.asarray(c.indices, dtype=np.int64), cols] = c.data
    return out


_SPARSE_KL_MISSING = "sparse_kl = True cannot be combined with absent = 'missing': the sparse KL solvers treat absent entries as zeros."


def _sparse_input(A, name, loss, absent="zero", sparse_kl=False):
    """Sparse argument of nnmf() / nnlm(): canonical CSC; square loss only unless sparse_kl; no non-finite stored values.  absent = "zero":
    absent entries are zeros; "missing": they are missing and every stored entry (an explicit zero included) is an observation.
    sparse_kl (absent = "zero" only): loss = 'mkl' is accepted, and then no stored value may be negative."""
    if sparse_kl and absent == "missing":
        raise NnlmStop(_SPARSE_KL_MISSING)
    if loss == "mkl" and not sparse_kl:
        raise NnlmStop("Sparse %s is supported for loss = 'mse' only; use a dense matrix for loss = 'mkl'." % name)
    c = as_csc(A)
    if not np.all(np.isfinite(c.data)):
        if absent == "missing":
            raise NnlmStop("Sparse %s must not store NA / non-finite values: with absent = 'missing' a missing entry is one left out of "
                           "the structure." % name)
        raise NnlmStop("Sparse %s must not contain NA / non-finite values: absent entries are zeros, not missing; use a dense matrix for "
                       "missing values." % name)
    if sparse_kl and loss == "mkl" and np.any(c.data < 0):
        raise NnlmStop("Sparse %s must not store negative values with loss = 'mkl' (sparse_kl = True): KL loss needs non-negative data." % name)
    return c


def _absent_arg(absent, x, name):
    """The `absent` argument of nnmf() / nnlm() / predict_nnmf(): "zero" (default) or "missing"; "missing" needs a sparse argument (the
    missing entries of a dense matrix are its NA)."""
    absent = _match_arg(absent, ("zero", "missing"), "absent")
    if absent == "missing" and not is_sparse(x):
        raise NnlmStop("absent = 'missing' needs a sparse %s (an object with tocsc()): the missing entries of a dense matrix are its NA "
                       "values." % name)
    return absent


# ------------------------------------------------------------------------------------------------
# per-entry weights on a sparse A (nnlm_set_matrix_csc_weighted)
# ------------------------------------------------------------------------------------------------
def _in_device_memory(x):
    """A dense or sparse tensor (or __cuda_array_interface__ producer) that does not live on the host."""
    if str(getattr(x, "layout", "")).startswith("torch.sparse_"):
        return getattr(getattr(x, "device", None), "type", "cpu") != "cpu"
    return _lib.is_device_array(x)


def _weights_refusals(who, name, x, loss, sparse_kl, init=None, weights=None, device_door=False):
    """What `weights` cannot be combined with, each refused by name.  True when the pair goes through the device door (device_door: the
    caller has one): a sparse tensor of the GPU with weights that live there too."""
    on_device = (device_door and _in_device_memory(weights) and str(getattr(x, "layout", "")).startswith("torch.sparse_")
                 and _in_device_memory(x))
    if not on_device and (_lib.is_device_array(x) or str(getattr(x, "layout", "")).startswith("torch.sparse_")):
        raise NnlmStop("%s: weights cannot be combined with a %s in device memory (dense or sparse tensor); pass a host sparse matrix "
                       "(an object with tocsc())." % (who, name))
    if not on_device and _in_device_memory(weights):
        raise NnlmStop("%s: weights live in device memory, but %s is a host matrix; pass the weights as a host array or sparse matrix (or "
                       "both as sparse tensors of the GPU)." % (who, name))
    if not on_device and not is_sparse(x):
        raise NnlmStop("%s: weights need a sparse %s (an object with tocsc()): one weight per stored entry; weights on a dense matrix are "
                       "not supported." % (who, name))
    if loss == "mkl" or sparse_kl:
        raise NnlmStop("%s: weights are supported for loss = 'mse' only (not loss = 'mkl' / sparse_kl)." % who)
    if isinstance(init, str):
        raise NnlmStop("%s: weights cannot be combined with init = %r: a matrix with per-entry weights has no SVD start here." % (who, init))
    return on_device


def _device_weights_arg(weights, parts, who):
    """`weights` of the device door as Handle.set_matrix_sparse_device_weighted takes them: a 1-D array of the GPU aligned with the
    values of the sparse tensor whose arrays are `parts`, or the (ptr, idx, val) of a sparse tensor of the same layout and shape (its
    pattern is the library's to check)."""
    try:
        wparts = _lib.sparse_tensor_parts(weights)
    except ValueError as e:
        raise NnlmStop("%s: weights: %s" % (who, e)) from None
    if wparts is None:
        return weights
    shape, layout = parts[3], parts[4]
    if wparts[4] != layout:
        raise NnlmStop("%s: weights is a sparse %s tensor, the matrix a sparse %s tensor; convert one of them (to_sparse_%s())." %
                       (who, wparts[4].upper(), layout.upper(), layout))
    if tuple(wparts[3]) != tuple(shape):
        raise NnlmStop("%s: weights is %d x %d, the matrix %d x %d." % (who, wparts[3][0], wparts[3][1], shape[0], shape[1]))
    return wparts[:3]


def _weights_arg(weights, A, c, who):
    """One fp64 weight per stored entry of the canonical CSC c = as_csc(A), in the order of c.data.  weights: an object with tocsc()
    whose canonical pattern equals c's, or a 1-D array of length nnz aligned with c.data -- the latter only when A was canonical already
    (as_csc neither reordered nor merged anything: otherwise the alignment is not defined)."""
    n, m = c.shape
    if is_sparse(weights):
        w = as_csc(weights)
        if tuple(w.shape) != (n, m):
            raise NnlmStop("%s: weights is %d x %d, the matrix %d x %d." % (who, w.shape[0], w.shape[1], n, m))
        if not np.array_equal(w.indptr, c.indptr) or not np.array_equal(w.indices, c.indices):
            for j in range(m):
                a0, a1, b0, b1 = c.indptr[j], c.indptr[j + 1], w.indptr[j], w.indptr[j + 1]
                if a1 - a0 != b1 - b0 or not np.array_equal(c.indices[a0:a1], w.indices[b0:b1]):
                    raise NnlmStop("%s: the stored pattern of weights differs from the matrix's (first in column %d): one weight per stored "
                                   "entry is needed." % (who, j))
        wd = w.data
    else:
        wd = np.asarray(weights, dtype=np.float64)
        if wd.ndim != 1 or wd.size != c.data.size:
            raise NnlmStop("%s: weights must be a sparse matrix with the matrix's stored pattern, or a 1-D array with one weight per stored "
                           "entry (%d); got shape %s." % (who, c.data.size, wd.shape))
        raw = A.tocsc()
        if not (np.array_equal(np.asarray(raw.indptr, dtype=np.int64), c.indptr) and np.asarray(raw.indices).size == c.indices.size
                and np.array_equal(np.asarray(raw.indices, dtype=np.int64), c.indices)):
            raise NnlmStop("%s: a weights array is aligned with the stored entries of a canonical CSC, but the matrix is not canonical "
                           "(unsorted or duplicate entries were reordered / merged); pass weights as a sparse matrix of the same pattern." % who)
    wd = np.ascontiguousarray(wd, dtype=np.float64)
    if not np.all(np.isfinite(wd)) or np.any(wd < 0):
        raise NnlmStop("%s: weights must be finite and >= 0." % who)
    return wd


def _stored_counts(c):
    """Stored entries per row and per column of a CSC."""
    n, m = c.shape
    return np.bincount(np.asarray(c.indices, dtype=np.int64), minlength=n), np.diff(c.indptr)


# ------------------------------------------------------------------------------------------------
# R/misc.R
# ------------------------------------------------------------------------------------------------
def mse_mkl(obs, pred, na_rm=True, show_warning=True):
    """R/misc.R:9-16 -> dict(MSE=, MKL=)."""
    obs = np.asarray(obs, dtype=np.float64)
    pred = np.asarray(pred, dtype=np.float64)
    mean = np.nanmean if na_rm else np.mean
    with np.errstate(divide="ignore", invalid="ignore"):
        if (not show_warning) and (np.any(obs < 0) or np.any(pred < 0)):
            mkl = float("nan")
        else:
            mkl = float(mean((obs + 1e-16) * np.log((obs + 1e-16) / (pred + 1e-16)) - obs + pred))
        mse = float(mean((obs - pred) ** 2))
    return {"MSE": mse, "MKL": mkl}


def _match_arg(value, choices, name):
    """R's match.arg for a scalar string (a tuple/list default selects its first entry)."""
    if isinstance(value, (tuple, list)):
        value = value[0]
    hits = [c for c in choices if c.startswith(str(value))]
    if len(hits) != 1:
        raise NnlmStop(f"'{name}' should be one of {', '.join(repr(c) for c in choices)}")
    return hits[0]


def get_method_code(method="scd", loss="mse"):
    """R/misc.R:28-35: 1 scd+mse, 2 lee+mse, 3 scd+mkl, 4 lee+mkl."""
    method = _match_arg(method, ("scd", "lee"), "method")
    loss = _match_arg(loss, ("mse", "mkl"), "loss")
    code = 1
    if loss == "mkl":
        code += 2
    if method == "lee":
        code += 1
    return code


def _is_empty(x):
    return x is None or np.size(x) == 0


def _as_matrix(x):
    """R's as.matrix(): a vector becomes a one-column matrix."""
    a = np.asarray(x)
    if a.ndim == 0:
        a = a.reshape(1, 1)
    elif a.ndim == 1:
        a = a.reshape(-1, 1)
    return a


def check_matrix(A, dm=None, mode="numeric", check_na=False, input_name="", check_negative=False):
    """R/misc.R:38-45."""
    if A is None:
        return
    A = np.asarray(A)
    if dm is not None:
        shp = A.shape if A.ndim == 2 else (A.shape[0] if A.ndim else 1, 1)
        bad = any(e is not None and int(e) != int(s) for s, e in zip(shp, dm))
        if bad:
            raise NnlmStop("Dimension of matrix %s is expected to be (%d, %d), but got (%d, %d)" % (
                input_name, shp[0], shp[1], -1 if dm[0] is None else dm[0], -1 if dm[1] is None else dm[1]))
    is_logical = A.dtype == np.bool_
    if mode == "logical" and not is_logical:
        raise NnlmStop("Matrix %s must be %s." % (input_name, mode))
    if mode == "numeric" and (is_logical or not np.issubdtype(A.dtype, np.number)):
        raise NnlmStop("Matrix %s must be %s." % (input_name, mode))
    if check_negative and mode == "numeric":
        v = A[~np.isnan(A.astype(np.float64))]
        if np.any(v < 0):
            raise NnlmStop("Matrix %s must be non-negative." % input_name)
    if check_na and mode == "numeric" and np.any(np.isnan(A.astype(np.float64))):
        raise NnlmStop("Matrix %s contains missing values." % input_name)


def reformat_input(init, mask, n, m, k, rng=None):
    """R/misc.R:48-129: stack [W W0 W1] / [H; H1; H0] and their masks.

    ``rng`` (numpy Generator) stands in for R's runif() used for blocks that are not supplied while
    a sibling block is (R/misc.R:107-112).
    """
    mask = {} if mask is None else dict(mask)
    init = {} if init is None else dict(init)
    if not isinstance(mask, dict) or not isinstance(init, dict):
        raise NnlmStop("init and mask must be lists (dicts)")
    rng = rng or np.random.default_rng()
    known_W = init.get("W0") is not None
    known_H = init.get("H0") is not None
    kW0 = kH0 = 0
    if known_W:
        init["W0"] = _as_matrix(init["W0"])
        kW0 = init["W0"].shape[1]
        mask["W0"] = np.ones((n, kW0), dtype=bool)
    else:
        mask["W0"] = None
        mask["H1"] = None
        init["H1"] = None
    if known_H:
        init["H0"] = _as_matrix(init["H0"])
        kH0 = init["H0"].shape[0]
        mask["H0"] = np.ones((kH0, m), dtype=bool)
    else:
        mask["H0"] = None
        mask["W1"] = None
        init["W1"] = None
    K = k + kW0 + kH0

    def dims(ew, eh):
        return {"W": (n, k * ew), "W0": (n, kW0 * ew), "W1": (n, kH0 * ew),
                "H": (k * eh, m), "H1": (kW0 * eh, m), "H0": (kH0 * eh, m)}

    ew = int(not all(_is_empty(mask.get(b)) for b in ("W", "W0", "W1")))
    eh = int(not all(_is_empty(mask.get(b)) for b in ("H", "H0", "H1")))
    dm = dims(ew, eh)
    for b in ("W", "W0", "W1", "H", "H0", "H1"):
        if not _is_empty(mask.get(b)):
            check_matrix(mask[b], dm[b], "logical", True, "mask$" + b)
            mask[b] = np.asarray(mask[b], dtype=bool).reshape(dm[b])
        else:
            mask[b] = np.zeros(dm[b], dtype=bool)
    ew = int(not all(_is_empty(init.get(b)) for b in ("W", "W0", "W1")))
    eh = int(not all(_is_empty(init.get(b)) for b in ("H", "H0", "H1")))
    di = dims(ew, eh)
    for b in ("W", "W0", "W1", "H", "H0", "H1"):
        if not _is_empty(init.get(b)):
            check_matrix(init[b], di[b], "numeric", True, "init$" + b)
            init[b] = np.asarray(init[b], dtype=np.float64).reshape(di[b])
        else:
            # matrix(runif(prod(dim)), ...): column-major fill
            init[b] = rng.random(di[b][0] * di[b][1]).reshape(di[b], order="F")
    return dict(
        Wm=np.concatenate([mask["W"], mask["W0"], mask["W1"]], axis=1),
        Hm=np.concatenate([mask["H"], mask["H1"], mask["H0"]], axis=0),
        Wi=np.concatenate([init["W"], init["W0"], init["W1"]], axis=1),
        Hi=np.concatenate([init["H"], init["H1"], init["H0"]], axis=0),
        kW0=kW0, kH0=kH0, K=K)


# ------------------------------------------------------------------------------------------------
# nnmf
# ------------------------------------------------------------------------------------------------
class NnmfResult(dict):
    """The reference's S3 object of class 'nnmf' (R/nnmf.R:184-224): a dict with attribute access."""

    __getattr__ = dict.__getitem__

    def __repr__(self):  # print.nnmf, R/nnmf_methods.R:53-80 (cosmetic, abbreviated)
        o = self["options"]
        return ("Non-negative matrix factorization:\n   Algorithm: %s\n        Loss: %s\n         MSE: %g\n         MKL: %g\n"
                "      Target: %g\n   Rel. tol.: %.3g\nTotal epochs: %d\n# Interation: %d\n" % (
                    {"scd": "Sequential coordinate-wise descent", "lee": "Lee's multiplicative algorithm"}[o["method"]],
                    {"mse": "Mean squared error", "mkl": "Mean Kullback-Leibler divergence"}[o["loss"]],
                    self["mse"][-1], self["mkl"][-1], self["target_loss"][-1],
                    abs(np.diff(self["target_loss"][-2:])[0] / np.mean(self["target_loss"][-2:])) if len(self["target_loss"]) > 1 else float("nan"),
                    int(np.sum(self["average_epochs"])), self["n_iteration"]))


def _nnmf_matrix_missing(A, loss):
    """_nnmf_matrix for a sparse A whose absent entries are missing: canonical CSC, and check_k's bound of the reference for missing
    data (R/nnmf.R:157-162): the fewest observed entries of a row or a column."""
    A = _sparse_input(A, "A", loss, "missing")
    n, m = A.shape
    min_k = min(n, m)
    if A.indices.size < n * m:
        rows, cols = _stored_counts(A)
        min_k = min(min_k, int(rows.min()), int(cols.min()))
    return dict(A=A, n=n, m=m, min_k=min_k)


def _nnmf_matrix(A, loss):
    """The matrix part of prepare_nnmf: A checked and converted once (dense: fp64; sparse: canonical CSC), its shape, and the largest
    k the check_k rule allows (min(n, m), less where rows or columns have missing entries)."""
    if is_sparse(A):  # canonical CSC (args[0]); absent entries are zeros, so there is nothing missing
        A = _sparse_input(A, "A", loss)
        n, m = A.shape
        return dict(A=A, n=n, m=m, min_k=min(n, m))
    A = np.asarray(A)
    if A.ndim != 2:
        raise NnlmStop("A must be a matrix")
    check_matrix(A, input_name="A")
    A = np.asarray(A, dtype=np.float64)
    n, m = A.shape
    min_k = min(n, m)
    isna = np.isnan(A)
    if isna.any():
        min_k = min(min_k, int((m - isna.sum(axis=1)).min()), int((n - isna.sum(axis=0)).min()))
    return dict(A=A, n=n, m=m, min_k=min_k)


def prepare_nnmf(A, k=1, alpha=(0, 0, 0), beta=(0, 0, 0), method="scd", loss="mse", init=None, mask=None, W_norm=-1,
                 check_k=True, max_iter=500, rel_tol=1e-4, n_threads=1, trace=None, verbose=1, show_warning=True,
                 inner_max_iter=None, inner_rel_tol=1e-9, rng=None, absent="zero", sparse_kl=False):
    """Argument normalisation of nnmf(), R/nnmf.R:142-183 -> (17-tuple for c_nnmf, context dict)."""
    args, ctx, _ = _prepare_nnmf(A, k, alpha, beta, method, loss, init, mask, W_norm, check_k, max_iter, rel_tol, n_threads, trace,
                                 verbose, show_warning, inner_max_iter, inner_rel_tol, rng, absent=absent, sparse_kl=sparse_kl)
    return args, ctx


def _prepare_nnmf(A, k=1, alpha=(0, 0, 0), beta=(0, 0, 0), method="scd", loss="mse", init=None, mask=None, W_norm=-1,
                  check_k=True, max_iter=500, rel_tol=1e-4, n_threads=1, trace=None, verbose=1, show_warning=True,
                  inner_max_iter=None, inner_rel_tol=1e-9, rng=None, matrix=None, absent="zero", sparse_kl=False):
    """prepare_nnmf, also returning the checked matrix; `matrix` = what an earlier call returned for the same A (nnmf_batch: the
    members share one checked, converted A)."""
    method = _match_arg(method, ("scd", "lee"), "method")
    loss = _match_arg(loss, ("mse", "mkl"), "loss")
    absent = _absent_arg(absent, A, "A")
    if sparse_kl and absent == "missing":
        raise NnlmStop(_SPARSE_KL_MISSING)
    if sparse_kl and loss == "mkl" and matrix is None and is_sparse(A):  # the opt-in door: KL loss on a sparse A (absent entries zeros)
        c = _sparse_input(A, "A", loss, sparse_kl=True)
        matrix = dict(A=c, n=c.shape[0], m=c.shape[1], min_k=min(c.shape))
    if inner_max_iter is None:
        inner_max_iter = 50 if loss == "mse" else 1  # R/nnmf.R:139
    if trace is None:
        trace = 100 / inner_max_iter  # R/nnmf.R:138
    if matrix is not None:
        mat = matrix
    else:
        mat = _nnmf_matrix_missing(A, loss) if absent == "missing" else _nnmf_matrix(A, loss)
    A, n, m = mat["A"], mat["n"], mat["m"]
    im = reformat_input(init, mask, n, m, int(k), rng=rng)
    K = im["K"]
    alpha = np.concatenate([np.atleast_1d(np.asarray(alpha, dtype=np.float64)), np.zeros(3)])[:3]
    beta = np.concatenate([np.atleast_1d(np.asarray(beta, dtype=np.float64)), np.zeros(3)])[:3]
    code = get_method_code(method, loss)
    min_k = mat["min_k"]
    if check_k and K > min_k and np.all(np.concatenate([alpha, beta]) == 0):
        raise NnlmStop("k larger than %d is not recommended, unless properly masked or regularized.\n"
                       "\t\t\t\tSet check.k = FALSE if you want to skip this checking." % min_k)
    if n_threads < 0:
        n_threads = 0
    verbose = int(verbose)
    if trace <= 0:
        trace = 999999
    args = (A, int(K), im["Wi"], im["Hi"], im["Wm"], im["Hm"], alpha, beta, int(max_iter), float(rel_tol),
            int(n_threads), verbose, bool(show_warning), int(inner_max_iter), float(inner_rel_tol), code, int(trace))
    ctx = dict(method=method, loss=loss, alpha=alpha, beta=beta, init=init, mask=mask, n_threads=n_threads, trace=trace,
               verbose=verbose, max_iter=max_iter, rel_tol=rel_tol, inner_max_iter=inner_max_iter,
               inner_rel_tol=inner_rel_tol, W_norm=W_norm, absent=absent,
               sparse_kl=bool(sparse_kl) and loss == "mkl" and isinstance(A, CSC))  # (the call goes through the *_csc_kl entries)
    return args, ctx, mat


def finish_nnmf(out, ctx, run_time=None):
    """Result decoration of nnmf(), R/nnmf.R:184-224."""
    on_device = _lib.is_device_array(out["W"])  # (nnmf() on a tensor in device memory: W and H stay tensors of that device)
    res = NnmfResult(W=out["W"] if on_device else np.array(out["W"]), H=out["H"] if on_device else np.array(out["H"]),
                     mse=np.asarray(out["mse_error"]).ravel(),
                     mkl=np.asarray(out["mkl_error"]).ravel(), target_loss=np.asarray(out["target_error"]).ravel(),
                     average_epochs=np.asarray(out["average_epoch"]).ravel(), n_iteration=int(out["n_iteration"]))
    W_norm = ctx["W_norm"]
    if W_norm > 0 and on_device:  # the same scaling with the tensor's own operators (a diagonal product is a scaling of columns / rows)
        W, H = res["W"], res["H"]
        scale = (W ** W_norm).sum(0) ** (1.0 / W_norm) if np.isfinite(W_norm) else W.max(0).values
        res["W"], res["H"] = W * (1.0 / scale)[None, :], scale[:, None] * H
    elif W_norm > 0:
        if np.isfinite(W_norm):
            scale = np.sum(res["W"] ** W_norm, axis=0) ** (1.0 / W_norm)
        else:
            scale = res["W"].max(axis=0)
        res["W"] = res["W"] @ np.diag(1.0 / scale)
        res["H"] = np.diag(scale) @ res["H"]
    res["run_time"] = run_time
    res["options"] = {key: ctx[key] for key in ("method", "loss", "alpha", "beta", "init", "mask", "n_threads", "trace",
                                                "verbose", "max_iter", "rel_tol", "inner_max_iter", "inner_rel_tol")}
    res["options"]["absent"] = ctx.get("absent", "zero")
    if out.get("warning"):
        warnings.warn("Target tolerance not reached. Try a larger max.iter.", RuntimeWarning, stacklevel=3)
    return res


# ------------------------------------------------------------------------------------------------
# A in device memory
# ------------------------------------------------------------------------------------------------
def _refuse_device(x, who, name):
    """The entries that stage their matrix on the host say so by name when handed device memory."""
    _refuse_sparse_tensor(x, who, name)
    if _lib.is_device_array(x):
        raise NnlmStop("%s: %s lives in device memory; this entry takes host arrays only (nnmf() and nnmf_batch() accept a device "
                       "matrix) -- copy it to the host first." % (who, name))


def _refuse_sparse_tensor(x, who, name):
    """A sparse tensor (any torch sparse layout) where an entry takes host arrays: refused by name, in device or in host memory."""
    if x is None or isinstance(x, (np.ndarray, np.generic, list, tuple, dict, int, float)):
        return
    if _lib.is_host_sparse_tensor(x):
        raise NnlmStop("%s: %s is a sparse tensor in host memory; pass a host sparse matrix as an object with tocsc() (scipy.sparse), or "
                       "move the tensor to the GPU for nnmf() / nnmf_batch()." % (who, name))
    if str(getattr(x, "layout", "")).startswith("torch.sparse_") and _lib.is_device_array(x):
        raise NnlmStop("%s: %s is a sparse tensor in device memory; this entry takes host arrays only (nnmf() and nnmf_batch() accept a "
                       "sparse CSC / CSR tensor of the GPU) -- pass the matrix as a host sparse object (tocsc())." % (who, name))


def _sparse_device_parts(A, who):
    """_lib.sparse_tensor_parts(A) for nnmf() / nnmf_batch(); a sparse tensor in host memory is refused by name."""
    if A is None or isinstance(A, (np.ndarray, np.generic, list, tuple, dict, int, float)):
        return None
    if _lib.is_host_sparse_tensor(A):
        raise NnlmStop("%s: A is a sparse tensor in host memory; pass a host sparse matrix as an object with tocsc() (scipy.sparse), or move "
                       "the tensor to the GPU." % who)
    try:
        return _lib.sparse_tensor_parts(A)
    except ValueError as e:
        raise NnlmStop("%s: %s" % (who, e)) from None


def _sparse_device_refusals(loss, absent, sparse_kl):
    """What _sparse_input refuses without looking at the values (the rest is the library's message)."""
    if sparse_kl and absent == "missing":
        raise NnlmStop(_SPARSE_KL_MISSING)
    if loss == "mkl" and not sparse_kl:
        raise NnlmStop("Sparse A is supported for loss = 'mse' only; use a dense matrix for loss = 'mkl'.")


def _sparse_device_matrix(parts, h, absent, kl, batch, weights=None):
    """The `matrix` of _prepare_nnmf for a sparse tensor in device memory: ingested into h (nnlm_set_matrix_sparse_device, or with
    `weights` of _device_weights_arg nnlm_set_matrix_sparse_device_weighted); check_k's bound with absent = 'missing' is the fewest
    stored entries of a row or a column, from the handle."""
    ptr, idx, val, shape, layout = parts
    try:
        if weights is not None:
            h.set_matrix_sparse_device_weighted(ptr, idx, val, weights, shape, layout, absent=absent)
        else:
            h.set_matrix_sparse_device(ptr, idx, val, shape, layout, absent=absent, kl=kl, batch=batch)
    except ValueError as e:
        if weights is None:
            raise
        raise NnlmStop("nnmf: %s" % e) from None
    n, m = h.n, h.m
    min_k = min(n, m)
    if absent == "missing" and h.matrix_info()["any_missing"]:
        min_k = min(min_k, int(h.get_info("matrix_min_row_observed")), int(h.get_info("matrix_min_col_observed")))
    return dict(A=None, n=n, m=m, min_k=min_k)


def _device_index(A):
    idx = getattr(getattr(A, "device", None), "index", None)
    if idx is None:
        idx = getattr(getattr(A, "device", None), "id", None)
    return int(idx) if isinstance(idx, (int, np.integer)) else int(os.environ.get("NNLM_DEVICE", "0") or 0)


def _device_matrix(A, h):
    """_nnmf_matrix for a matrix in device memory: ingested into the handle h (nnlm_set_matrix_device), its shape, and check_k's bound
    from the handle's counts of observed entries -- every NON-FINITE entry counts as missing here (the fit's own rule); the host route
    counts NaN only, so a matrix with +-Inf entries can get a smaller bound here."""
    h.set_matrix_device(A)
    n, m = h.n, h.m
    min_k = min(n, m)
    if h.matrix_info()["any_missing"]:
        min_k = min(min_k, int(h.get_info("matrix_min_row_observed")), int(h.get_info("matrix_min_col_observed")))
    return dict(A=A, n=n, m=m, min_k=min_k)


def _host_factor_entries(init, who):
    """init entries that are tensors in device memory, as host fp64 arrays (k (n + m) elements: the one small copy of the device route;
    the stacking of W / W0 / W1 and the checks of reformat_input stay one piece of host code)."""
    if init is None:
        return None
    out = dict(init)
    for key, v in out.items():
        if _lib.is_device_array(v):
            if not callable(getattr(v, "cpu", None)):
                raise NnlmStop("%s: init$%s lives in device memory but is not a tensor (no cpu()); pass it as a host array." % (who, key))
            out[key] = np.asarray(v.detach().cpu().double().numpy() if callable(getattr(v, "detach", None)) else v.cpu(), dtype=np.float64)
    return out


def _default_init(W, H, Wm, Hm, n, m, K, g):
    """What nnmf() leaves empty, c_nnmf draws through unif_rand (src/nnmf.cpp:82-98): 0.01 U(0,1), W row by row first, then H
    column-major, masked entries drawn and zeroed."""
    if not np.size(W):
        W = 0.01 * g.random(n * K).reshape((n, K))
        if np.size(Wm):
            W[np.asarray(Wm, dtype=bool).reshape(n, K)] = 0.0
    if not np.size(H):
        H = 0.01 * g.random(K * m).reshape((K, m), order="F")
        if np.size(Hm):
            H[np.asarray(Hm, dtype=bool).reshape(K, m)] = 0.0
    return W, H


def _tensor_lib(A):
    """The tensor library of A when A is one of its tensors (imported here only: the package itself never imports it), else None."""
    if (type(A).__module__ or "").split(".")[0] != "torch":
        return None
    import torch
    return torch


def _nnmf_device(A, k, alpha, beta, method, loss, init, mask, W_norm, check_k, max_iter, rel_tol, n_threads, trace, verbose,
                 show_warning, inner_max_iter, inner_rel_tol, rng, absent, sparse_kl=False, parts=None, weights=None):
    """nnmf() on a matrix in device memory: ingest, factors, run and export on one Handle; A never visits the host.  parts: the arrays
    of a sparse CSC / CSR tensor (_lib.sparse_tensor_parts), ingested through the door `absent` and `sparse_kl` name -- with `weights`
    (device memory too, _weights_refusals has passed them) through the weighted door."""
    torch = _tensor_lib(A)
    if parts is not None:
        loss = _match_arg(loss, ("mse", "mkl"), "loss")
        absent = _match_arg(absent, ("zero", "missing"), "absent")
        _sparse_device_refusals(loss, absent, sparse_kl)
        sparse_kl = bool(sparse_kl) and loss == "mkl"
        if weights is not None:
            weights = _device_weights_arg(weights, parts, "nnmf")
    g = rng or np.random.default_rng()
    t0 = time.perf_counter()
    with _lib.Handle(_device_index(A), _env_precision()) as h:
        mat = _device_matrix(A, h) if parts is None else _sparse_device_matrix(parts, h, absent, sparse_kl, False, weights)
        # (a sparse tensor: the handle knows what absent entries are; _prepare_nnmf's `absent` asks for an object with tocsc())
        args, ctx, _ = _prepare_nnmf(A, k, alpha, beta, method, loss, _host_factor_entries(init, "nnmf"), mask, W_norm, check_k, max_iter,
                                     rel_tol, n_threads, trace, verbose, show_warning, inner_max_iter, inner_rel_tol, rng, matrix=mat,
                                     absent=absent if parts is None else "zero")
        ctx["init"] = init
        if parts is not None:
            ctx["absent"], ctx["sparse_kl"] = absent, sparse_kl
        n, m, K = mat["n"], mat["m"], args[1]
        Wm, Hm = args[4], args[5]
        W, H = _default_init(args[2], args[3], Wm, Hm, n, m, K, g)
        cb = _lib.make_callbacks(print_fn=(lambda s: print(s, end="")) if ctx["verbose"] == 2 else None)
        h.set_factors(K, W, H, Wm, Hm)
        # (alpha, beta, max_iter, rel_tol | verbose, show_warning, inner_max_iter, inner_rel_tol, method, trace: n_threads has no place)
        out = h.run(*args[6:10], *args[11:], callbacks=cb)
        if torch is not None:
            Wo = torch.empty((n, K), dtype=torch.float64, device=A.device)
            Ho = torch.empty((K, m), dtype=torch.float64, device=A.device)
            h.get_factors_device(Wo, Ho)
            out["W"], out["H"] = Wo, Ho
        else:
            out["W"], out["H"] = h.get_factors()
    return finish_nnmf(out, ctx, run_time=time.perf_counter() - t0)


# ------------------------------------------------------------------------------------------------
# truncated SVD of A and the NNDSVD start
# ------------------------------------------------------------------------------------------------
SVD_INITS = ("nndsvd", "nndsvda")


def _svd_init_arg(init, who):
    """A string init names an NNDSVD variant."""
    if init not in SVD_INITS:
        raise NnlmStop("%s: init = %r is not a start this library knows; a string init is one of %s." % (who, init, ", ".join(map(repr, SVD_INITS))))
    return init


def _svd_width(k, oversample, power_iters, n, m, who):
    try:
        k, oversample, power_iters = int(k), int(oversample), int(power_iters)
    except (TypeError, ValueError):
        raise NnlmStop("%s: k, the oversampling and the power iterations must be integers" % who) from None
    if k < 1 or k > min(n, m):
        raise NnlmStop("%s: k = %d outside 1 .. min(n, m) = %d: a matrix has no more singular triplets than that." % (who, k, min(n, m)))
    if oversample < 0 or power_iters < 0:
        raise NnlmStop("%s: the oversampling and the power iterations must be >= 0" % who)
    return min(k + oversample, n, m), power_iters


def _svd_omega(l, m, g):
    """The l x m sketch matrix, uniform on (-1, 1), filled column by column as reformat_input fills H."""
    return (2.0 * g.random(l * m) - 1.0).reshape((l, m), order="F")


def _svd_refuse_missing(what, who):
    raise NnlmStop("%s: %s; the truncated SVD and the NNDSVD start need a matrix without missing entries." % (who, what))


def _svd_ingest(A, h, who, loss="mse", kl=False, batch=False, parts=None):
    """A of any supported kind into the handle h, absent entries of a sparse A zeros -> the `matrix` of _prepare_nnmf."""
    if parts is not None:
        mat = _sparse_device_matrix(parts, h, "zero", kl, batch)
    elif _lib.is_device_array(A):
        mat = _device_matrix(A, h)
        if h.matrix_info()["any_missing"]:
            _svd_refuse_missing("A has non-finite (NA, NaN or +-Inf) entries", who)
    elif is_sparse(A):
        c = _sparse_input(A, "A", loss, sparse_kl=kl)
        mat = dict(A=c, n=c.shape[0], m=c.shape[1], min_k=min(c.shape))
        door = {(False, False): h.set_matrix_csc, (False, True): h.set_matrix_csc_batch, (True, False): h.set_matrix_csc_kl,
                (True, True): h.set_matrix_csc_kl_batch}[(bool(kl), bool(batch))]
        door(c.indptr, c.indices, c.data, c.shape)
    else:
        mat = _nnmf_matrix(A, loss)
        if not np.isfinite(mat["A"]).all():
            _svd_refuse_missing("A has non-finite (NA, NaN or +-Inf) entries", who)
        h.set_matrix(mat["A"])
    return mat


def _precision_arg(precision):
    if precision is None:
        return _env_precision()
    table = {"f32": _lib.PREC_F32, "fp32": _lib.PREC_F32, "f64": _lib.PREC_F64, "fp64": _lib.PREC_F64,
             _lib.PREC_F32: _lib.PREC_F32, _lib.PREC_F64: _lib.PREC_F64}
    if precision not in table:
        raise NnlmStop("precision must be None (NNLM_PRECISION decides), 'f32' or 'f64' (got %r)" % (precision,))
    return table[precision]


def truncated_svd(A, k, oversample=10, power_iters=2, rng=None, precision=None):
    """The leading k singular triplets of A on the GPU -> (U n x k, s descending, Vt k x m), by randomised subspace iteration with a
    sketch of width l = min(k + oversample, n, m) and ``power_iters`` power iterations: 2 power_iters + 2 passes over A through the
    library's cross products, l x l eigendecompositions on the host.  The sketch matrix is 2 rng.random(l m) - 1; nothing else is
    random, and two calls with equal ``rng`` give identical bits.  The sign of a triplet is unspecified (joint for u_j and v_j).

    ``A``: a host array, a sparse object with tocsc() (absent entries are zeros), a tensor in device memory or a sparse CSC / CSR tensor
    of the GPU.  ``precision``: "f32" (split-fp16 cross products, about 22 bits of A) or "f64"; None: what NNLM_PRECISION names.
    Use: a scree of the singular values beside nnmf_cv; the error of the rank-k SVD, sum(s[k:]**2), as the floor for any rank-k model."""
    who = "truncated_svd"
    parts = _sparse_device_parts(A, who)
    prec = _precision_arg(precision)
    on_device = parts is not None or _lib.is_device_array(A)
    if not on_device and not is_sparse(A):
        shape = np.shape(A)
        if len(shape) != 2:
            raise NnlmStop("A must be a matrix")
        _svd_width(k, oversample, power_iters, shape[0], shape[1], who)
        if not np.isfinite(np.asarray(A, dtype=np.float64)).all():
            _svd_refuse_missing("A has non-finite (NA, NaN or +-Inf) entries", who)
    g = rng or np.random.default_rng()
    with _lib.Handle(_device_index(A) if on_device else int(os.environ.get("NNLM_DEVICE", "0") or 0), prec) as h:
        mat = _svd_ingest(A, h, who, parts=parts)
        l, q = _svd_width(k, oversample, power_iters, mat["n"], mat["m"], who)
        h.svd(l, q, _svd_omega(l, mat["m"], g))
        return h.get_svd(int(k))


def _svd_init_refusals(who, init, loss, mask, absent, sparse_A, sparse_kl):
    """What a string init cannot be combined with, named before any device is touched."""
    if not _is_empty(mask) and any(not _is_empty(v) for v in dict(mask).values()):
        raise NnlmStop("%s: init = %r cannot be combined with masks: the start is made from the SVD of A, not from masked blocks." % (who, init))
    if absent == "missing":
        raise NnlmStop("%s: init = %r needs absent = 'zero': a matrix whose absent entries are missing has no SVD here." % (who, init))
    if loss == "mkl" and not sparse_A:
        raise NnlmStop("%s: init = %r with loss = 'mkl' on a dense A is not supported; use loss = 'mse', or a sparse count matrix with "
                       "sparse_kl and init = 'nndsvda'." % (who, init))
    if loss == "mkl" and sparse_A and not sparse_kl:
        raise NnlmStop("Sparse A is supported for loss = 'mse' only; use a dense matrix for loss = 'mkl'.")
    if loss == "mkl" and init == "nndsvd":
        raise NnlmStop("%s: init = 'nndsvd' leaves exact zeros in W and H, which KL loss cannot start from; use init = 'nndsvda'." % who)


def _nnmf_svd_init(A, k, alpha, beta, method, loss, init, mask, W_norm, check_k, max_iter, rel_tol, n_threads, trace, verbose,
                   show_warning, inner_max_iter, inner_rel_tol, rng, absent, sparse_kl, parts, oversample, power_iters):
    """nnmf(init = "nndsvd" | "nndsvda"): ingest, svd, set_factors_nndsvd, run and export on one Handle, for every kind of A."""
    who = "nnmf"
    init = _svd_init_arg(init, who)
    loss = _match_arg(loss, ("mse", "mkl"), "loss")
    on_device = parts is not None or _lib.is_device_array(A)
    sparse_A = parts is not None or is_sparse(A)
    absent = _match_arg(absent, ("zero", "missing"), "absent") if sparse_A else "zero"
    _svd_init_refusals(who, init, loss, mask, absent, sparse_A, sparse_kl)
    kl = bool(sparse_kl) and loss == "mkl"
    if not on_device and not sparse_A and np.ndim(A) == 2 and not np.isfinite(np.asarray(A, dtype=np.float64)).all():
        _svd_refuse_missing("A has non-finite (NA, NaN or +-Inf) entries", who)
    torch = _tensor_lib(A)
    g = rng or np.random.default_rng()
    t0 = time.perf_counter()
    with _lib.Handle(_device_index(A) if on_device else int(os.environ.get("NNLM_DEVICE", "0") or 0), _env_precision()) as h:
        mat = _svd_ingest(A, h, who, loss, kl, False, parts)
        n, m = mat["n"], mat["m"]
        l, q = _svd_width(k, oversample, power_iters, n, m, who)
        omega = _svd_omega(l, m, g)  # (drawn before anything else consumes the generator)
        args, ctx, _ = _prepare_nnmf(A, k, alpha, beta, method, loss, None, None, W_norm, check_k, max_iter, rel_tol, n_threads, trace,
                                     verbose, show_warning, inner_max_iter, inner_rel_tol, np.random.default_rng(0), matrix=mat, absent="zero",
                                     sparse_kl=kl)
        ctx["init"] = init
        ctx["sparse_kl"] = kl
        K = args[1]
        cb = _lib.make_callbacks(print_fn=(lambda s: print(s, end="")) if ctx["verbose"] == 2 else None)
        h.svd(l, q, omega)
        h.set_factors_nndsvd(K, init)
        out = h.run(*args[6:10], *args[11:], callbacks=cb)
        if torch is not None:
            Wo = torch.empty((n, K), dtype=torch.float64, device=A.device)
            Ho = torch.empty((K, m), dtype=torch.float64, device=A.device)
            h.get_factors_device(Wo, Ho)
            out["W"], out["H"] = Wo, Ho
        else:
            out["W"], out["H"] = h.get_factors()
    return finish_nnmf(out, ctx, run_time=time.perf_counter() - t0)


def _nnmf_batch_svd_init(A, ks, nrun, init, g, opts, unsupported, missing_door, kl_door, parts):
    """nnmf_batch(init = "nndsvd" | "nndsvda"): ONE decomposition at the top rank for all members (component j of the start depends on
    triplet j alone), then the batch on the same handle."""
    who = "nnmf_batch"
    if nrun != 1:
        raise _lib.NnlmError(_lib.ERR_ARG, "%s: init = %r is deterministic: nrun = %d members of one rank would be identical (use nrun = 1)"
                             % (who, init, nrun))
    if missing_door:
        raise unsupported("init = %r is not supported with sparse_batch = 'missing': a matrix whose absent entries are missing has no SVD here" % init)
    if kl_door and init == "nndsvd":
        raise unsupported("init = 'nndsvd' leaves exact zeros in W and H, which KL loss cannot start from; use init = 'nndsvda'")
    opts = dict(opts)
    oversample, power_iters = opts.pop("svd_oversample", 10), opts.pop("svd_power_iters", 2)
    on_device = parts is not None or _lib.is_device_array(A)
    if not on_device and not is_sparse(A) and np.ndim(A) == 2 and not np.isfinite(np.asarray(A, dtype=np.float64)).all():
        raise unsupported("A has missing (NA, NaN or +-Inf) entries; the batched factorisation needs a finite A")
    with _lib.Handle(_device_index(A) if on_device else int(os.environ.get("NNLM_DEVICE", "0") or 0), _env_precision()) as h:
        try:
            mat = _svd_ingest(A, h, who, "mkl" if kl_door else "mse", kl_door, True, parts)
        except NnlmStop as e:
            if "non-finite" in str(e):
                raise unsupported("A has missing (NA, NaN or +-Inf) entries; the batched factorisation needs a finite A") from None
            raise
        n, m = mat["n"], mat["m"]
        l, q = _svd_width(max(ks), oversample, power_iters, n, m, who)
        omega = _svd_omega(l, m, g)
        opts["absent"] = "zero"
        prep = []
        for kb in ks:
            args, ctx, mat = _prepare_nnmf(A, kb, init=None, rng=np.random.default_rng(0), matrix=mat, **opts)
            ctx["init"] = init
            if kl_door:
                ctx["sparse_kl"] = True
            prep.append((args, ctx))
        a0 = prep[0][0]
        cb = _lib.make_callbacks(print_fn=(lambda s: print(s, end="")) if prep[0][1]["verbose"] == 2 else None)
        t0 = time.perf_counter()
        h.svd(l, q, omega)
        h.set_factors_nndsvd_batch(ks, init)
        outs = h.run_batch(*a0[6:10], *a0[11:], callbacks=cb)
        torch = _tensor_lib(A)
        for o, (W, H) in zip(outs, h.get_factors_batch()):
            o["W"], o["H"] = (W, H) if torch is None else (torch.from_numpy(W).to(A.device), torch.from_numpy(H).to(A.device))
        run_time = time.perf_counter() - t0
    res = [finish_nnmf(o, p[1], run_time=run_time) for o, p in zip(outs, prep)]
    best = int(np.argmin([r["target_loss"][-1] if len(r["target_loss"]) else np.inf for r in res]))
    return res, best


def nnmf(A, k=1, alpha=(0, 0, 0), beta=(0, 0, 0), method="scd", loss="mse", init=None, mask=None, W_norm=-1,
         check_k=True, max_iter=500, rel_tol=1e-4, n_threads=1, trace=None, verbose=0, show_warning=True,
         inner_max_iter=None, inner_rel_tol=1e-9, rng=None, absent="zero", sparse_kl=False, svd_oversample=10, svd_power_iters=2,
         weights=None):
    """Non-negative matrix factorisation A ~ W H on the MI355X (drop-in for R's NNLM::nnmf, R/nnmf.R:135-225).

    ``weights`` (sparse A, loss "mse", k <= 64): one weight c >= 0 per stored entry -- a sparse matrix with A's stored pattern, or a
    1-D array aligned with the stored entries of a canonical A.  With A a sparse CSC / CSR tensor of the GPU the weights live there too:
    a 1-D tensor (or __cuda_array_interface__ object) aligned with A.values(), or a sparse tensor of A's layout and shape whose pattern
    the library checks; A and the weights are ingested where they lie.  The loss is 1/2 sum of c (a - (WH))^2 over the observed entries + the
    penalties.  With absent = "missing" the observed entries are the stored ones (weighted NMF: inverse-variance weights, down-weighted
    doubtful ratings).  With absent = "zero" every entry is observed and an absent one is a zero of weight 1: implicit feedback (Hu,
    Koren & Volinsky 2008: store r with weight 1 + alpha r).  The traces are the weighted sums over N = nnz (missing) or n m (zero).
    Refused by name: a dense A, host weights with an A in device memory (and device weights with a host A), a sparse weights tensor of
    another layout or shape than A, loss "mkl" / sparse_kl, a string init.

    ``init`` = "nndsvd" or "nndsvda": a deterministic, data-driven start (Boutsidis & Gallopoulos 2008) from a truncated SVD of A made on
    the GPU (truncated_svd(): sketch width min(k + svd_oversample, n, m), svd_power_iters power iterations, the sketch matrix drawn from
    ``rng`` -- the only random numbers of such a fit).  Every kind of A (host array, sparse object, device tensor, sparse device tensor)
    then runs on one handle in the arithmetic mode NNLM_PRECISION names: A is uploaded once, decomposed, started and fitted there.
    "nndsvd" leaves exact zeros in W and H: fine for method "scd", but Lee's multiplicative updates keep a zero forever -- use
    "nndsvda" (zeros replaced by mean(A)) with method "lee".  Refused with a string init (NnlmStop): masks, absent = "missing", an A
    with non-finite entries, loss "mkl" on a dense A, and "nndsvd" with loss "mkl" (sparse_kl: "nndsvda" only).  Known profiles are
    entries of an init dict and so cannot be combined with it.

    ``verbose`` defaults to 0 here (R: 1 = progress bar); ``rng`` seeds the default random init (R uses its global RNG).
    ``absent`` (sparse A only): "zero" -- absent entries are zeros; "missing" -- they are missing and the fit runs over the stored
    entries only, as the reference does for NA (a score matrix such as movies x customers; square loss, k <= 64).
    ``sparse_kl`` (sparse A, absent = "zero"): True admits loss = 'mkl' on a sparse A (count data; stored values >= 0, k <= 64): the KL
    solvers then run over the stored entries only.  The default refuses loss = 'mkl' on a sparse A, as before.

    ``A`` may live in device memory: a torch tensor on the GPU (fp64, fp32, fp16 or bf16; any non-overlapping strides) or any object with
    ``__cuda_array_interface__``.  It is then ingested where it is -- no copy through the host -- and fitted in the arithmetic mode
    NNLM_PRECISION names.  For a torch tensor W and H come back as fp64 tensors on A's device (W_norm applied there) and the traces as
    numpy arrays; for another producer W and H come back as numpy arrays.  With the same seeded ``rng`` the fit is the host route's.
    init entries and known profiles may be host arrays or tensors of that device (the latter are copied to the host, k (n + m) elements,
    stacked there and uploaded with the other factors); masks are host arrays.  check_k with missing entries:
    this route counts every non-finite entry (NaN, +-Inf) as missing, as the fit does; the host route counts NaN only.

    ``A`` may also be a SPARSE tensor of the GPU, ``torch.sparse_csc_tensor`` or ``sparse_csr_tensor`` (int32 or int64 indices, any of the
    four value types): its three arrays are validated, transposed and converted by kernels where they lie, and ``absent``, ``sparse_kl``,
    ``loss`` mean what they mean for a host sparse A.  The structure must be canonical (indices strictly increasing in every line): what
    as_csc() repairs on the host is refused here, with the library's message.  W and H come back as fp64 tensors on A's device.  Other
    sparse layouts (COO, BSR, BSC) and sparse tensors in host memory are refused by name.
    """
    device_weights = weights is not None and _weights_refusals("nnmf", "A", A, _match_arg(loss, ("mse", "mkl"), "loss"), sparse_kl, init,
                                                               weights, device_door=True)
    parts = _sparse_device_parts(A, "nnmf")
    if isinstance(init, str):
        return _nnmf_svd_init(A, k, alpha, beta, method, loss, init, mask, W_norm, check_k, max_iter, rel_tol, n_threads, trace, verbose,
                              show_warning, inner_max_iter, inner_rel_tol, rng, absent, sparse_kl, parts, svd_oversample, svd_power_iters)
    if parts is not None or _lib.is_device_array(A):
        return _nnmf_device(A, k, alpha, beta, method, loss, init, mask, W_norm, check_k, max_iter, rel_tol, n_threads, trace, verbose,
                            show_warning, inner_max_iter, inner_rel_tol, rng, absent, sparse_kl, parts, weights if device_weights else None)
    args, ctx = prepare_nnmf(A, k, alpha, beta, method, loss, init, mask, W_norm, check_k, max_iter, rel_tol, n_threads,
                             trace, verbose, show_warning, inner_max_iter, inner_rel_tol, rng, absent, sparse_kl)
    g = rng or np.random.default_rng()
    cb = _lib.make_callbacks(unif_rand=lambda: g.random(), print_fn=(lambda s: print(s, end="")) if ctx["verbose"] == 2 else None)
    t0 = time.perf_counter()
    if weights is not None:
        c = args[0]
        wd = _weights_arg(weights, A, c, "nnmf")
        out = _lib.c_nnmf_csc_weighted(c.indptr, c.indices, c.data, wd, ctx["absent"] == "missing", c.shape, *args[1:], callbacks=cb)
    elif isinstance(args[0], CSC):
        entry = _lib.c_nnmf_csc_missing if ctx["absent"] == "missing" else (_lib.c_nnmf_csc_kl if ctx["sparse_kl"] else _lib.c_nnmf_csc)
        out = entry(*args[0], *args[1:], callbacks=cb)
    else:
        out = _lib.c_nnmf(*args, callbacks=cb)
    return finish_nnmf(out, ctx, run_time=time.perf_counter() - t0)


def _batch_rank_list(k, nrun):
    """nnmf_batch's members: every rank of k (an int or a sequence) nrun times, rank after rank."""
    try:
        ranks = [int(k)] if np.ndim(k) == 0 else [int(v) for v in k]
        nrun = int(nrun)
    except (TypeError, ValueError):
        raise _lib.NnlmError(_lib.ERR_ARG, "k must be an integer or a sequence of integers, nrun an integer") from None
    ks = [r for r in ranks for _ in range(nrun)]
    if not ks or min(ks) < 1 or nrun < 1 or len(ks) > _lib.BATCH_MAX:
        raise _lib.NnlmError(_lib.ERR_ARG, "a batch needs 1..%d members of rank >= 1 (k = %s, nrun = %d)" % (_lib.BATCH_MAX, ranks, nrun))
    return ks


def nnmf_batch(A, k, nrun=1, init=None, rng=None, sparse_batch=False, **nnmf_options):
    """Several nnmf() runs of one dense matrix at once: random restarts (nrun) and rank sweeps (k a sequence) share every pass over A.

    Member list: each rank of ``k`` gets ``nrun`` members, rank after rank (k = [2, 3], nrun = 2 -> ranks 2, 2, 3, 3).  ``init`` is None
    or one ``{"W": n x k_b, "H": k_b x m}`` dict per member (either entry may be missing); what is not given is drawn from ``rng``
    member by member exactly as nnmf() draws it.  ``nnmf_options`` are nnmf()'s other arguments, shared by all members.
    Each member's result is what nnmf() returns for that member alone.  Returns (list of per-member nnmf results, index of the member
    with the smallest final target error).

    Square loss only, dense A without missing entries, no masks or known profiles, ranks summing to at most 64: anything else raises
    NnlmError with code NNLM_ERR_UNSUPPORTED; a bad k list or an init that does not match it, NNLM_ERR_ARG.

    ``sparse_batch`` = True admits a sparse A (an object with tocsc(); absent entries are zeros): it is made canonical once for all
    members, every half-step is one SpMM over the non-zeros at the stacked rank and every trace iteration one walk over them.  The other
    limits stay, and absent = 'missing' is refused.  With a dense A the flag changes nothing; the default refuses a sparse A as before.

    ``sparse_batch`` = "missing" takes a sparse A whose absent entries are MISSING (a score matrix; every stored entry, an explicit zero
    included, is an observation): per half-step one SpMM and, per column chunk, one launch for the per-column Grams of all members.
    check_k's bound is the fewest stored entries of a row or a column, as for nnmf(absent = 'missing'); ``absent``, if given with it, must
    be 'missing'; a dense A is refused.

    ``sparse_batch`` = "kl" takes a sparse A of counts (stored values >= 0, absent entries zeros) and admits loss = 'mkl' (method "scd"
    or "lee"): per half-step one solver launch over the lines of at most 256 stored entries for all members; member b is bit for bit
    nnmf(A, k_b, loss = 'mkl', sparse_kl = True) from the same start.  loss = 'mse' with it behaves as ``sparse_batch`` = True.  A dense
    A and absent = 'missing' are refused; without it loss = 'mkl' is refused as before.

    ``init`` = "nndsvd" or "nndsvda" starts every member from the NNDSVD of ONE truncated SVD of A, made at the width min(max(k) +
    svd_oversample, n, m) (options svd_oversample = 10, svd_power_iters = 2; the sketch matrix comes from ``rng``): member b takes the
    first k_b triplets, so a rank sweep ``k = range(1, 11)`` costs one decomposition, not ten.  A then runs on one handle in the mode
    NNLM_PRECISION names.  nrun > 1 is refused (NNLM_ERR_ARG: the members would be identical); sparse_batch = True is taken,
    sparse_batch = "kl" with "nndsvda" only, sparse_batch = "missing" is refused.
    """
    missing_door = _sparse_batch_arg(sparse_batch, "nnmf_batch")
    kl_door = sparse_batch == "kl" if isinstance(sparse_batch, str) else False
    sparse_batch = bool(sparse_batch)
    ks = _batch_rank_list(k, nrun)
    B = len(ks)
    svd_init = None
    if isinstance(init, str):  # one truncated SVD of A starts every member
        svd_init, init = _svd_init_arg(init, "nnmf_batch"), None
    if init is not None:
        if isinstance(init, dict) or len(init) != B:
            raise _lib.NnlmError(_lib.ERR_ARG, "init must be a list of %d dicts {'W': ..., 'H': ...}, one per member" % B)
        init = [dict(x) if x is not None else {} for x in init]
    unsupported = lambda msg: _lib.NnlmError(_lib.ERR_UNSUPPORTED, "nnmf_batch: " + msg)
    if not _is_empty(nnmf_options.get("mask")) and any(not _is_empty(v) for v in dict(nnmf_options["mask"]).values()):
        raise unsupported("masks are not supported by the batched factorisation")
    if init is not None and any(x.get("W0") is not None or x.get("H0") is not None for x in init):
        raise unsupported("known profiles (W0 / H0) are not supported by the batched factorisation")
    loss = _match_arg(nnmf_options.get("loss", "mse"), ("mse", "mkl"), "loss")
    if loss != "mse" and not kl_door:
        raise unsupported("loss = 'mkl' (KL) is not supported by the batched factorisation: square loss only")
    parts = _sparse_device_parts(A, "nnmf_batch")  # (a sparse CSC / CSR tensor of the GPU: the same doors, ingested where it lies)
    sparse_A = is_sparse(A) or parts is not None
    if sparse_A and not sparse_batch:
        raise unsupported("a sparse A is not supported by the batched factorisation (dense A only)")
    if kl_door and not sparse_A:
        raise unsupported("sparse_batch = 'kl' needs a sparse A (an object with tocsc()): the batched KL solver runs over the stored "
                          "entries of a sparse count matrix")
    kl_door = kl_door and loss == "mkl"  # (square loss through this door: sparse_batch = True)
    if missing_door:
        _missing_door_checks(A, nnmf_options, unsupported, sparse_A)
        nnmf_options = dict(nnmf_options, absent="missing")
    elif sparse_A and _match_arg(nnmf_options.get("absent", "zero"), ("zero", "missing"), "absent") == "missing":
        raise unsupported("absent = 'missing' is not supported by the batched factorisation of a sparse A (sparse_batch = True): "
                          "absent entries are zeros")
    if sum(ks) > _lib.BATCH_MAX:
        raise unsupported("the ranks sum to %d; a batch holds at most %d" % (sum(ks), _lib.BATCH_MAX))
    if svd_init is not None:
        opts = dict(nnmf_options)
        opts.setdefault("verbose", 0)
        return _nnmf_batch_svd_init(A, ks, int(nrun), svd_init, rng or np.random.default_rng(), opts, unsupported, missing_door, kl_door, parts)
    for key in ("svd_oversample", "svd_power_iters"):
        if key in nnmf_options:
            raise _lib.NnlmError(_lib.ERR_ARG, "nnmf_batch: %s belongs to init = 'nndsvd' / 'nndsvda'" % key)
    on_device = _lib.is_device_array(A)
    shape = tuple(A.shape) if isinstance(A, np.ndarray) or on_device else np.shape(A)
    if on_device and init is not None:
        init = [_host_factor_entries(x, "nnmf_batch") for x in init]
    if init is not None and len(shape) == 2:
        n, m = shape
        for b, x in enumerate(init):
            for key, shp in (("W", (n, ks[b])), ("H", (ks[b], m))):
                if x.get(key) is not None and np.shape(x[key]) != shp:
                    raise _lib.NnlmError(_lib.ERR_ARG, "init[%d]['%s'] has shape %s, member %d (rank %d) needs %s"
                                         % (b, key, np.shape(x[key]), b, ks[b], shp))
    opts = dict(nnmf_options)
    opts.setdefault("verbose", 0)
    g = rng or np.random.default_rng()
    h = None
    if on_device:  # one ingest shared by all members; the handle then runs the batch (what nnlm_c_nnmf_batch does around a host A)
        h = _lib.Handle(_device_index(A), _env_precision())
    try:
        return _nnmf_batch_members(A, ks, init, g, opts, unsupported, h, missing_door, kl_door, parts)
    finally:
        if h is not None:
            h.close()


def _sparse_batch_arg(sparse_batch, who):
    """True when sparse_batch is the string "missing" (the door of a sparse A whose absent entries are missing); "kl" (nnmf_batch's door
    of KL loss on a sparse count matrix) passes as not that door; any other string is an argument error, anything else is the flag it
    has always been."""
    if isinstance(sparse_batch, str):
        if sparse_batch == "kl":
            if who == "nnmf_cv":
                raise _lib.NnlmError(_lib.ERR_UNSUPPORTED, "nnmf_cv: sparse_batch = 'kl' is not supported: a hold-out set on a sparse matrix "
                                                           "whose absent entries are zeros is not built (use nnmf_batch)")
            return False
        if sparse_batch != "missing":
            raise _lib.NnlmError(_lib.ERR_ARG, "%s: sparse_batch must be False, True, 'missing' or 'kl' (got %r)" % (who, sparse_batch))
        return True
    return False


def _missing_door_checks(A, nnmf_options, unsupported, sparse_A=None):
    """sparse_batch = 'missing': a sparse A, and `absent`, if given, 'missing'."""
    if not (is_sparse(A) if sparse_A is None else sparse_A):
        raise unsupported("sparse_batch = 'missing' needs a sparse A (an object with tocsc()): the missing entries of a dense matrix of "
                          "the batched factorisation come from a hold-out set only")
    if _match_arg(nnmf_options.get("absent", "missing"), ("zero", "missing"), "absent") != "missing":
        raise unsupported("absent = 'zero' contradicts sparse_batch = 'missing' (the batched factorisation of a sparse A whose absent "
                          "entries are missing); use sparse_batch = True for absent entries that are zeros")


def _nnmf_batch_members(A, ks, init, g, opts, unsupported, h, missing_door=False, kl_door=False, parts=None):
    """nnmf_batch behind its argument checks; h: the handle of a device A (None for a host A); parts: the arrays of a sparse tensor in
    device memory (_lib.sparse_tensor_parts), ingested through the door's batch entry."""
    B = len(ks)
    prep, Ws, Hs, mat = [], [], [], None
    if parts is not None:
        _sparse_device_refusals("mkl" if kl_door else "mse", "missing" if missing_door else "zero", kl_door)
        mat = _sparse_device_matrix(parts, h, "missing" if missing_door else "zero", kl_door, True)
        opts = dict(opts, absent="zero")  # (the handle knows; _prepare_nnmf's `absent` asks for an object with tocsc())
    elif h is not None:
        mat = _device_matrix(A, h)
        if h.matrix_info()["any_missing"]:
            raise unsupported("A has missing (NA, NaN or +-Inf) entries; the batched factorisation needs a finite A")
    elif missing_door:  # (canonical CSC once for all members; check_k's bound: the fewest stored entries of a line)
        mat = _nnmf_matrix_missing(A, "mse")
    elif is_sparse(A):  # (sparse_batch = True / 'kl': canonical CSC once for all members; check_k's bound is min(n, m))
        c = _sparse_input(A, "A", "mkl" if kl_door else "mse", sparse_kl=kl_door)
        mat = dict(A=c, n=c.shape[0], m=c.shape[1], min_k=min(c.shape))
    for b in range(B):  # member after member, each consuming the generator as nnmf() would
        # (A is checked and converted by the first member's call only: every member shares that one fp64 copy)
        args, ctx, mat = _prepare_nnmf(A, ks[b], init=None if init is None else init[b], rng=g, matrix=mat, **opts)
        if kl_door:
            ctx["sparse_kl"] = True  # (what nnmf(sparse_kl = True) records for the same member)
        if parts is not None and missing_door:
            ctx["absent"] = "missing"
        if b == 0 and h is None and not isinstance(mat["A"], CSC) and not np.isfinite(mat["A"]).all():
            raise unsupported("A has missing (NA, NaN or +-Inf) entries; the batched factorisation needs a finite A")
        n, m = mat["n"], mat["m"]
        W, H = _default_init(args[2], args[3], (), (), n, m, ks[b], g)
        Ws.append(W)
        Hs.append(H)
        prep.append((args, ctx))
    a0 = prep[0][0]
    cb = _lib.make_callbacks(print_fn=(lambda s: print(s, end="")) if prep[0][1]["verbose"] == 2 else None)
    t0 = time.perf_counter()
    if missing_door and parts is None:
        outs = _lib.c_nnmf_csc_missing_batch(*a0[0], ks, Ws, Hs, *a0[6:], callbacks=cb)
    elif isinstance(a0[0], CSC):
        entry = _lib.c_nnmf_csc_kl_batch if kl_door else _lib.c_nnmf_csc_batch
        outs = entry(*a0[0], ks, Ws, Hs, *a0[6:], callbacks=cb)
    elif h is None:
        outs = _lib.c_nnmf_batch(a0[0], ks, Ws, Hs, *a0[6:], callbacks=cb)
    else:
        h.set_factors_batch(ks, Ws, Hs)
        outs = h.run_batch(*a0[6:10], *a0[11:], callbacks=cb)
        torch = _tensor_lib(A)
        for o, (W, H) in zip(outs, h.get_factors_batch()):
            o["W"], o["H"] = (W, H) if torch is None else (torch.from_numpy(W).to(A.device), torch.from_numpy(H).to(A.device))
    run_time = time.perf_counter() - t0
    res = [finish_nnmf(o, p[1], run_time=run_time) for o, p in zip(outs, prep)]
    best = int(np.argmin([r["target_loss"][-1] if len(r["target_loss"]) else np.inf for r in res]))
    return res, best


def _pack_batches(ks, cap=None):
    """nnmf_cv's batches: the members in order, a new batch whenever the next rank would take the rank sum beyond `cap` (64) ->
    [(first, last + 1)].  A single rank beyond the cap fits no batch (NNLM_ERR_UNSUPPORTED)."""
    cap = _lib.BATCH_MAX if cap is None else cap
    out, start, tot = [], 0, 0
    for b, kb in enumerate(ks):
        if kb > cap:
            raise _lib.NnlmError(_lib.ERR_UNSUPPORTED, "nnmf_cv: rank %d exceeds %d, the largest rank sum of a batch" % (kb, cap))
        if tot + kb > cap:
            out.append((start, b))
            start, tot = b, 0
        tot += kb
    out.append((start, len(ks)))
    return out


def _holdout_pattern(holdout, n, m, rng):
    """nnmf_cv's hold-out set as a canonical CSC pattern (indptr int64 [m + 1], row indices int32).  A fraction in (0, 1): round(f n m)
    entries drawn uniformly without replacement from `rng`; a boolean n x m array: its True entries; a {"indptr", "indices"} dict (what
    nnmf_cv returned): that pattern again."""
    if isinstance(holdout, dict):
        ptr, idx = np.asarray(holdout["indptr"], dtype=np.int64), np.asarray(holdout["indices"], dtype=np.int32)
        if ptr.shape != (m + 1,) or ptr[0] != 0 or np.any(np.diff(ptr) < 0) or ptr[-1] != idx.size:
            raise _lib.NnlmError(_lib.ERR_ARG, "nnmf_cv: the hold-out pattern needs indptr of length ncol + 1, non-decreasing from 0 to len(indices)")
        return ptr, idx
    if np.ndim(holdout) == 0:
        f = float(holdout)
        if not 0.0 < f < 1.0:
            raise _lib.NnlmError(_lib.ERR_ARG, "nnmf_cv: holdout must be a fraction in (0, 1) or a boolean %d x %d array (got %r)" % (n, m, holdout))
        flat = np.sort(rng.choice(n * m, size=int(round(f * n * m)), replace=False))  # column-major position j n + i
        cols, rows = flat // n, flat % n
    else:
        mask = np.asarray(holdout)
        if mask.dtype != np.bool_ or mask.shape != (n, m):
            raise _lib.NnlmError(_lib.ERR_ARG, "nnmf_cv: holdout must be a fraction in (0, 1) or a boolean %d x %d array" % (n, m))
        cols, rows = np.nonzero(mask.T)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=m))]).astype(np.int64)
    return ptr, rows.astype(np.int32)


def _env_precision():
    """The precision rule of the one-shot entries: NNLM_PRECISION = f32 selects the fp32-operand mode, anything else strict fp64."""
    return _lib.PREC_F32 if os.environ.get("NNLM_PRECISION") in ("f32", "fp32", "0") else _lib.PREC_F64


def _holdout_pattern_stored(holdout, c, rng):
    """nnmf_cv's hold-out set on a sparse A whose absent entries are missing, as positions into the stored entries of the canonical CSC c
    (sorted, unique).  A fraction in (0, 1): round(f nnz) stored entries drawn uniformly without replacement from `rng`; a {"indptr",
    "indices"} dict (what nnmf_cv returned): that pattern again, which must be canonical and a subset of the stored pattern."""
    n, m = c.shape
    nnz = int(c.indices.size)
    if isinstance(holdout, dict):
        ptr, idx = np.asarray(holdout["indptr"], dtype=np.int64), np.asarray(holdout["indices"], dtype=np.int64)
        if ptr.shape != (m + 1,) or ptr[0] != 0 or np.any(np.diff(ptr) < 0) or ptr[-1] != idx.size:
            raise _lib.NnlmError(_lib.ERR_ARG, "nnmf_cv: the hold-out pattern needs indptr of length ncol + 1, non-decreasing from 0 to len(indices)")
        if idx.size and (idx.min() < 0 or idx.max() >= n):
            raise _lib.NnlmError(_lib.ERR_ARG, "nnmf_cv: the hold-out pattern has a row index out of range")
        hkey = np.repeat(np.arange(m, dtype=np.int64), np.diff(ptr)) * n + idx  # column-major position j n + i
        if np.any(np.diff(hkey) <= 0):
            raise _lib.NnlmError(_lib.ERR_ARG, "nnmf_cv: the hold-out pattern is not canonical (row indices strictly increasing within a column)")
        skey = np.repeat(np.arange(m, dtype=np.int64), np.diff(c.indptr)) * n + np.asarray(c.indices, dtype=np.int64)
        pos = np.searchsorted(skey, hkey)
        bad = (pos >= nnz) | (skey[np.minimum(pos, max(nnz - 1, 0))] != hkey) if nnz else np.ones(hkey.size, dtype=bool)
        if bad.any():
            e = int(np.flatnonzero(bad)[0])
            raise _lib.NnlmError(_lib.ERR_ARG, "nnmf_cv: held-out entry %d (row %d, column %d) is not a stored entry of A"
                                 % (e, int(hkey[e] % n), int(hkey[e] // n)))
        return pos
    if np.ndim(holdout) != 0:
        raise _lib.NnlmError(_lib.ERR_ARG, "nnmf_cv: on a sparse A, holdout must be a fraction in (0, 1) of the stored entries or the holdout "
                                           "dict of an earlier result")
    f = float(holdout)
    if not 0.0 < f < 1.0:
        raise _lib.NnlmError(_lib.ERR_ARG, "nnmf_cv: holdout must be a fraction in (0, 1) of the stored entries (got %r)" % (holdout,))
    return np.sort(rng.choice(nnz, size=int(round(f * nnz)), replace=False))


def _split_stored(c, pos):
    """The canonical CSC c without its stored entries at the (sorted) positions pos, and the pattern of those entries:
    (training CSC, (indptr int64, indices int32))."""
    n, m = c.shape
    cols = np.repeat(np.arange(m, dtype=np.int64), np.diff(c.indptr))
    held = np.zeros(c.indices.size, dtype=bool)
    held[pos] = True
    hptr, tptr = np.zeros(m + 1, dtype=np.int64), np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols[held], minlength=m), out=hptr[1:])
    np.cumsum(np.bincount(cols[~held], minlength=m), out=tptr[1:])
    train = CSC(tptr, np.ascontiguousarray(c.indices[~held], dtype=np.int32), np.ascontiguousarray(c.data[~held]), (n, m))
    return train, (hptr, np.ascontiguousarray(c.indices[held], dtype=np.int32))


def nnmf_cv(A, k, nrun=1, holdout=0.1, rng=None, init=None, sparse_batch=False, **nnmf_options):
    """Rank selection on held-out entries (the reference's vignette method): a share of the entries of the dense matrix A is kept out
    of the fit, every member (``k`` and ``nrun`` as in nnmf_batch) is fitted on the rest by the batched factorisation, and the member
    whose reconstruction of the held-out entries has the lowest mean squared error is ``best``.

    ``holdout``: a fraction in (0, 1), drawn uniformly without replacement from ``rng`` BEFORE any member's init is drawn; or a boolean
    n x m array (True = held out); or the ``holdout`` entry of an earlier result.  With check_k (the default) and no penalties, a
    hold-out set that leaves a row or a column fewer than max(k) + 1 training entries is rejected (NnlmStop, the check_k wording).
    Members whose ranks sum to more than 64 run as successive batches, in order, on one handle: A is uploaded once.
    Refused as by nnmf_batch (NnlmError, NNLM_ERR_UNSUPPORTED): loss = 'mkl', masks, known profiles, a sparse A, an A with non-finite
    entries; a single rank above 64.  The arithmetic mode is NNLM_PRECISION's, as for nnmf().

    ``sparse_batch`` = "missing" takes a sparse A whose absent entries are MISSING (a ratings matrix): ``holdout`` is then a fraction of
    the STORED entries (round(f nnz) of them, drawn without replacement from ``rng`` before any init) or the ``holdout`` dict of an earlier
    result (a subset of the stored pattern); check_k's bound is the fewest training entries of a row or a column, as for
    nnmf(absent = 'missing'); nothing n x m sized is formed.  ``absent``, if given with it, must be 'missing'.  Without the flag a sparse
    A is refused as before.

    Returns a dict: fits (nnmf results with holdout_mse / holdout_mkl added), k (rank per member), holdout_mse, holdout_mkl (arrays),
    best (index of the lowest holdout_mse, the first on ties), holdout ({"indptr", "indices", "shape"}: the pattern used)."""
    missing_door = _sparse_batch_arg(sparse_batch, "nnmf_cv")
    if isinstance(init, str):
        raise _lib.NnlmError(_lib.ERR_UNSUPPORTED, "nnmf_cv: init = %r is not supported: the fit runs on a matrix whose held-out entries are "
                                                   "missing, and a matrix with missing entries has no SVD here" % init)
    ks = _batch_rank_list(k, nrun)
    B = len(ks)
    if init is not None:
        if isinstance(init, dict) or len(init) != B:
            raise _lib.NnlmError(_lib.ERR_ARG, "init must be a list of %d dicts {'W': ..., 'H': ...}, one per member" % B)
        init = [dict(x) if x is not None else {} for x in init]
    unsupported = lambda msg: _lib.NnlmError(_lib.ERR_UNSUPPORTED, "nnmf_cv: " + msg)
    if not _is_empty(nnmf_options.get("mask")) and any(not _is_empty(v) for v in dict(nnmf_options["mask"]).values()):
        raise unsupported("masks are not supported by the batched factorisation")
    if init is not None and any(x.get("W0") is not None or x.get("H0") is not None for x in init):
        raise unsupported("known profiles (W0 / H0) are not supported by the batched factorisation")
    if _match_arg(nnmf_options.get("loss", "mse"), ("mse", "mkl"), "loss") != "mse":
        raise unsupported("loss = 'mkl' (KL) is not supported by the batched factorisation: square loss only")
    if is_sparse(A) and not missing_door:
        raise unsupported("a sparse A is not supported by the batched factorisation (dense A only)")
    if missing_door:
        _missing_door_checks(A, nnmf_options, unsupported)
        nnmf_options = dict(nnmf_options, absent="missing")
    _refuse_device(A, "nnmf_cv", "A")  # (the hold-out pattern is applied in the upload's host staging pass)
    batches = _pack_batches(ks)
    if missing_door:
        full = _sparse_input(A, "A", "mse", "missing")  # (canonical CSC, once)
        mat = dict(A=full, n=full.shape[0], m=full.shape[1], min_k=min(full.shape))
    else:
        mat = _nnmf_matrix(A, "mse")
        if not np.isfinite(mat["A"]).all():
            raise unsupported("A has missing (NA, NaN or +-Inf) entries; the batched factorisation takes missing entries through the "
                              "hold-out set only")
    n, m = mat["n"], mat["m"]
    if init is not None:
        for b, x in enumerate(init):
            for key, shp in (("W", (n, ks[b])), ("H", (ks[b], m))):
                if x.get(key) is not None and np.shape(x[key]) != shp:
                    raise _lib.NnlmError(_lib.ERR_ARG, "init[%d]['%s'] has shape %s, member %d (rank %d) needs %s"
                                         % (b, key, np.shape(x[key]), b, ks[b], shp))
    g = rng or np.random.default_rng()
    if missing_door:
        pos = _holdout_pattern_stored(holdout, full, g)
        if full.indices.size and pos.size == full.indices.size:
            raise _lib.NnlmError(_lib.ERR_ARG, "nnmf_cv: every stored entry of A is held out; nothing is left to fit")
        train, (ptr, idx) = _split_stored(full, pos)
        # check.k on the training entries, the bound of nnmf(absent = 'missing'): the fewest stored entries of a row or a column
        row_obs, col_obs = _stored_counts(train)
        min_k = min(n, m) if train.indices.size == n * m else min(n, m, int(row_obs.min()), int(col_obs.min()))
        mat = dict(mat, min_k=min_k)
    else:
        ptr, idx = _holdout_pattern(holdout, n, m, g)
        # check.k (R/nnmf.R:157-164) on the training entries: k + 1 of them in every row and column
        row_obs = m - np.bincount(idx, minlength=n)
        col_obs = n - np.diff(ptr)
        mat = dict(mat, min_k=min(mat["min_k"], int(row_obs.min()) - 1, int(col_obs.min()) - 1))
    opts = dict(nnmf_options)
    opts.setdefault("verbose", 0)
    prep, Ws, Hs = [], [], []
    _prepare_nnmf(A, max(ks), rng=np.random.default_rng(0), matrix=mat, **opts)  # (the check_k rule at the largest rank, before any init is drawn from g)
    for b in range(B):  # member after member, each consuming the generator as nnmf() would
        args, ctx, _ = _prepare_nnmf(A, ks[b], init=None if init is None else init[b], rng=g, matrix=mat, **opts)
        W, H = args[2], args[3]
        Ws.append(W if np.size(W) else 0.01 * g.random(n * ks[b]).reshape((n, ks[b])))
        Hs.append(H if np.size(H) else 0.01 * g.random(ks[b] * m).reshape((ks[b], m), order="F"))
        prep.append((args, ctx))
    a0 = prep[0][0]
    cb = _lib.make_callbacks(print_fn=(lambda s: print(s, end="")) if prep[0][1]["verbose"] == 2 else None)
    fits, hmse, hmkl = [], np.zeros(B), np.zeros(B)
    with _lib.Handle(int(os.environ.get("NNLM_DEVICE", "0") or 0), _env_precision()) as h:
        if missing_door:  # (one upload: the stored entries and the pattern; the library takes the held-out ones out)
            h.set_matrix_csc_missing_batch(*full, holdout=(ptr, idx))
        else:
            h.set_matrix_holdout(mat["A"], ptr, idx)
        for b0, b1 in batches:
            t0 = time.perf_counter()
            h.set_factors_batch(ks[b0:b1], Ws[b0:b1], Hs[b0:b1])
            # (alpha, beta, max_iter, rel_tol | verbose, show_warning, inner_max_iter, inner_rel_tol, method, trace: n_threads has no place)
            outs = h.run_batch(*a0[6:10], *a0[11:], callbacks=cb)
            facs = h.get_factors_batch()
            hmse[b0:b1], hmkl[b0:b1] = h.holdout_errors()
            run_time = time.perf_counter() - t0
            for b, o, (W, H) in zip(range(b0, b1), outs, facs):
                o["W"], o["H"] = W, H
                r = finish_nnmf(o, prep[b][1], run_time=run_time)
                r["holdout_mse"], r["holdout_mkl"] = float(hmse[b]), float(hmkl[b])
                fits.append(r)
    best = int(np.argmin(np.where(np.isnan(hmse), np.inf, hmse)))
    return dict(fits=fits, k=list(ks), holdout_mse=hmse, holdout_mkl=hmkl, best=best,
                holdout=dict(indptr=ptr, indices=idx, shape=(n, m)))


# ------------------------------------------------------------------------------------------------
# nnlm / predict
# ------------------------------------------------------------------------------------------------
class NnlmResult(dict):
    __getattr__ = dict.__getitem__


def _rcond(x):
    """R's rcond(x) for a tall matrix: reciprocal 1-norm condition number of the R factor of qr(x)."""
    r = np.linalg.qr(x, mode="r")
    try:
        return 1.0 / (np.linalg.norm(r, 1) * np.linalg.norm(np.linalg.inv(r), 1))
    except np.linalg.LinAlgError:
        return 0.0


def prepare_nnlm(x, y, alpha=(0, 0, 0), method="scd", loss="mse", init=None, mask=None, check_x=True, max_iter=10000,
                 rel_tol=1e-12, n_threads=1, show_warning=True, absent="zero", sparse_kl=False):
    """Argument normalisation of nnlm(), R/nnlm.R:75-120 -> (9-tuple for c_nnlm, context)."""
    method = _match_arg(method, ("scd", "lee"), "method")
    loss = _match_arg(loss, ("mse", "mkl"), "loss")
    absent = _absent_arg(absent, y, "y")
    _refuse_device(x, "nnlm", "x")
    _refuse_device(y, "nnlm", "y")
    x = np.asarray(x)
    y_sparse = is_sparse(y)
    yv = _sparse_input(y, "y", loss, absent, sparse_kl) if y_sparse else np.asarray(y)
    with np.errstate(invalid="ignore"):
        if show_warning and loss == "mkl" and (np.any(x < 0) or (not y_sparse and np.any(yv < 0))):  # (a sparse y with loss 'mkl' holds no negative value)
            warnings.warn("x or y have negative values. One should instead use method == 'mse'.", RuntimeWarning, stacklevel=3)
    is_y_vector = (not y_sparse) and yv.ndim == 1
    ym = yv if y_sparse else _as_matrix(yv)  # (sparse y: canonical CSC, args[1])
    if not y_sparse:
        check_matrix(ym, check_na=False)
    check_matrix(x, check_na=True)
    if x.ndim != 2:
        raise NnlmStop("x must be a matrix")
    if x.shape[0] != ym.shape[0]:
        raise NnlmStop("Dimensions of x and y do not match.")
    x = np.asarray(x, dtype=np.float64)
    if not y_sparse:
        ym = np.asarray(ym, dtype=np.float64)
    if max_iter <= 0:
        raise NnlmStop("max.iter must be positive.")
    if n_threads < 0:
        n_threads = 0
    if check_x:
        if x.shape[0] < x.shape[1] or _rcond(x) < np.finfo(np.float64).eps:
            warnings.warn("x does not have a full column rank. Solution may not be unique.", RuntimeWarning, stacklevel=3)
    alpha = np.concatenate([np.atleast_1d(np.asarray(alpha, dtype=np.float64)), np.zeros(3)])[:3]
    if show_warning and alpha[0] < alpha[1]:
        warnings.warn("If alpha[1] < alpha[2], be aware that that algorithm may not converge or unique.", RuntimeWarning, stacklevel=3)
    p, q = x.shape[1], ym.shape[1]
    if not _is_empty(mask):
        check_matrix(mask, dm=(p, q), mode="logical", check_na=True)
    if not _is_empty(init):
        check_matrix(init, dm=(p, q), check_na=True, check_negative=True)
    mask_m = None if _is_empty(mask) else np.asarray(mask, dtype=bool).reshape(p, q)
    init_m = None if _is_empty(init) else np.asarray(init, dtype=np.float64).reshape(p, q)
    if mask_m is not None and init_m is None:
        init_m = (~mask_m).astype(np.float64)  # masked entries fixed to 0, R/nnlm.R:110-112
    code = get_method_code(method, loss)
    args = (x, ym, alpha, mask_m, init_m, int(max_iter), float(rel_tol), int(n_threads), code)
    ctx = dict(method=method, loss=loss, max_iter=max_iter, rel_tol=rel_tol, is_y_vector=is_y_vector, alpha=alpha, x=x, y=ym, absent=absent,
               sparse_kl=bool(sparse_kl) and loss == "mkl" and y_sparse)
    return args, ctx


def _weighted_mse_mkl(x, y, coef, wd, missing):
    """The weighted error summary of nnlm(weights=): MSE = sum c (y - x beta)^2 / N and MKL = (sum c ((y + eps) log(y + eps) - y) + sum c
    (-(y + eps) log(pred + eps) + pred)) / N over the observed entries -- the stored ones (N = nnz), or all n q with weight 1 and y = 0
    at the absent ones (N = n q).  Nothing n x q sized: the absent entries' sums come from the Gram of x and the sums of x and beta."""
    eps = 1e-16
    n, q = y.shape
    cols = np.repeat(np.arange(q), np.diff(y.indptr))
    rows = np.asarray(y.indices, dtype=np.int64)
    pred = np.einsum("ek,ek->e", x[rows], coef.T[cols]) if cols.size else np.zeros(0)
    a = y.data
    with np.errstate(divide="ignore", invalid="ignore"):
        sq = float(np.sum(wd * (a - pred) ** 2))
        kl = float(np.sum(wd * ((a + eps) * np.log(a + eps) - a))) + float(np.sum(wd * (-(a + eps) * np.log(pred + eps) + pred)))
        N = float(a.size)
        if not missing:  # the absent entries: weight 1, y = 0 -- sum pred^2, sum eps log eps - eps log(pred + eps) + pred (the log term <= 3.7e-15 each, left out)
            sq += max(0.0, float(np.sum((x.T @ x) * (coef @ coef.T))) - float(np.sum(pred ** 2)))
            N = float(n) * float(q)
            kl += (N - a.size) * (eps * np.log(eps)) + float(x.sum(axis=0) @ coef.sum(axis=1)) - float(np.sum(pred))
        if np.any(a < 0) or np.any(pred < 0):
            kl = float("nan")
    return {"MSE": sq / N if N else float("nan"), "MKL": kl / N if N else float("nan")}


def finish_nnlm(sol, ctx):
    """R/nnlm.R:122-144."""
    coef = np.array(sol["coefficient"])
    x, y, alpha, loss = ctx["x"], ctx["y"], ctx["alpha"], ctx["loss"]
    if ctx.get("weights") is not None:
        err = _weighted_mse_mkl(x, y, coef, ctx["weights"], ctx.get("absent") == "missing")
    elif isinstance(y, CSC) and ctx.get("absent") == "missing":  # (mse_mkl with na.rm over the stored entries only: nothing n x q sized)
        cols = np.repeat(np.arange(y.shape[1]), np.diff(y.indptr))
        pred = np.einsum("ek,ek->e", x[np.asarray(y.indices, dtype=np.int64)], coef.T[cols]) if cols.size else np.zeros(0)
        err = mse_mkl(y.data, pred, na_rm=True, show_warning=False)
    else:
        if isinstance(y, CSC):  # (the summary compares y with the dense x beta: n x q either way)
            y = csc_toarray(y)
        err = mse_mkl(y, x @ coef, na_rm=True, show_warning=False)
    target = 0.5 * err["MSE"] if loss == "mse" else err["MKL"]
    target = target + (alpha[0] - alpha[1]) * float(np.sum(coef ** 2)) + alpha[1] * float(np.sum(coef.sum(axis=0) ** 2)) \
        + alpha[2] * float(np.sum(coef))
    res = NnlmResult(coefficients=coef[:, 0] if ctx["is_y_vector"] else coef, n_iteration=int(sol["n_iteration"]),
                     error={"MSE": err["MSE"], "MKL": err["MKL"], "target.error": target},
                     options={"method": ctx["method"], "loss": loss, "max_iter": ctx["max_iter"], "rel_tol": ctx["rel_tol"]})
    return res


def nnlm(x, y, alpha=(0, 0, 0), method="scd", loss="mse", init=None, mask=None, check_x=True, max_iter=10000,
         rel_tol=1e-12, n_threads=1, show_warning=True, rng=None, absent="zero", sparse_kl=False, weights=None):
    """Non-negative linear model y ~ x beta on the MI355X (drop-in for R's NNLM::nnlm, R/nnlm.R:70-145).

    ``weights`` (host sparse y, loss "mse", at most 64 columns of x): one weight >= 0 per stored entry of y, as for nnmf(); the error
    summary is then the weighted one (MSE = sum c (y - x beta)^2 / N over the observed entries, N = nnz or n q).

    ``absent`` (sparse y only): "zero" -- absent entries are zeros; "missing" -- they are missing, each column of beta is fitted to the
    stored entries of its column of y only (square loss, at most 64 columns of x).
    ``sparse_kl`` (sparse y, absent = "zero"): True admits loss = 'mkl' (stored values >= 0, at most 64 columns of x); see nnmf()."""
    if weights is not None:
        _weights_refusals("nnlm", "y", y, _match_arg(loss, ("mse", "mkl"), "loss"), sparse_kl, weights=weights)
    args, ctx = prepare_nnlm(x, y, alpha, method, loss, init, mask, check_x, max_iter, rel_tol, n_threads, show_warning, absent, sparse_kl)
    g = rng or np.random.default_rng()
    cb = _lib.make_callbacks(unif_rand=lambda: g.random())
    if weights is not None:
        c = args[1]
        ctx["weights"] = wd = _weights_arg(weights, y, c, "nnlm")
        sol = _lib.c_nnlm_csc_weighted(args[0], c.indptr, c.indices, c.data, wd, ctx["absent"] == "missing", c.shape, *args[2:], callbacks=cb)
        return finish_nnlm(sol, ctx)
    if isinstance(args[1], CSC):
        entry = _lib.c_nnlm_csc_missing if ctx["absent"] == "missing" else (_lib.c_nnlm_csc_kl if ctx["sparse_kl"] else _lib.c_nnlm_csc)
        return finish_nnlm(entry(args[0], *args[1], *args[2:], callbacks=cb), ctx)
    return finish_nnlm(_lib.c_nnlm(*args, callbacks=cb), ctx)


def predict_nnmf(object, newdata=None, which="A", method=None, loss=None, _nnlm=None, absent="zero", weights=None, **kw):
    """S3 predict.nnmf, R/nnmf_methods.R:22-48.  ``_nnlm`` lets the CPU tests substitute the solver.  ``absent = "missing"`` with a
    sparse ``newdata`` and which = "H" is the recommender's fold-in of new users: their H columns fitted to their stored scores only
    (which = "W": new rows, the same over their stored entries; which = "A" returns W H and ignores ``absent``).  ``weights``: one
    weight per stored entry of a sparse ``newdata``, as for nnlm() -- the weighted fold-in (which = "H" only)."""
    which = _match_arg(which, ("A", "W", "H"), "which")
    method = method or object["options"]["method"]
    loss = loss or object["options"]["loss"]
    solver = _nnlm or nnlm
    _refuse_device(newdata, "predict_nnmf", "newdata")
    for key in ("W", "H"):
        _refuse_device(object[key], "predict_nnmf", "object$" + key)
    if which != "A" and _absent_arg(absent, newdata, "newdata") == "missing":  # (which = "A" solves nothing: `absent` is not used)
        kw["absent"] = "missing"
    if which != "A" and is_sparse(newdata):  # (passed on to nnlm() as it is: duck-typed there)
        nd = newdata
        want = object["H"].shape[1] if which == "W" else object["W"].shape[0]
        got = nd.shape[1] if which == "W" else nd.shape[0]
        if int(got) != int(want):
            raise NnlmStop("Dimension of newdata does not match the %s factor of the model." % ("H" if which == "W" else "W"))
    elif which != "A":
        nd = np.asarray(newdata)
        if which == "W":
            check_matrix(nd, dm=(None, object["H"].shape[1]))
        if which == "H":
            check_matrix(nd, dm=(object["W"].shape[0], None))
        nd = np.asarray(nd, dtype=np.float64)
    if which == "A":
        return object["W"] @ object["H"]
    if weights is not None and which == "W":
        raise NnlmStop("predict_nnmf: weights are supported with which = 'H' (the fold-in of new columns) only.")
    if weights is not None and which == "H":
        kw["weights"] = weights
    if which == "W":
        out = solver(object["H"].T, nd.T, method=method, loss=loss, **kw)
        out["coefficients"] = np.asarray(out["coefficients"]).T
        return out
    return solver(object["W"], nd, method=method, loss=loss, **kw)


# ------------------------------------------------------------------------------------------------
# scores of a fit without forming W H (nnlm_predict_entries / nnlm_top_n)
# ------------------------------------------------------------------------------------------------
def _fit_factors(fit, who):
    """Host W (n x k) and H (k x m) of an nnmf() result, checked against each other."""
    for key in ("W", "H"):
        _refuse_device(fit[key], who, "fit$" + key)
    W, H = np.asarray(fit["W"], dtype=np.float64), np.asarray(fit["H"], dtype=np.float64)
    if W.ndim != 2 or H.ndim != 2 or W.shape[1] != H.shape[0] or W.shape[1] < 1:
        raise NnlmStop("%s: fit must hold W (n x k) and H (k x m) of one rank k >= 1 (got %s and %s)." % (who, W.shape, H.shape))
    return W, H


def _index_arg(x, name, limit):
    try:
        a = _lib.index_array(x, name)
    except ValueError as e:
        raise NnlmStop(str(e)) from None
    if a.size and (a.min() < 0 or a.max() >= limit):
        raise NnlmStop("%s holds an index out of range (0 .. %d)." % (name, limit - 1))
    return a


def _scoring_handle(W, H, pattern, precision):
    """A handle that knows n, m and the factors.  Its matrix is the cheapest the library takes: a sparse one with the given stored
    pattern (values 1; only the pattern is ever read) -- the EMPTY n x m pattern when there is none, m + 1 column pointers."""
    n, m = W.shape[0], H.shape[1]
    h = _lib.Handle(int(os.environ.get("NNLM_DEVICE", "0") or 0), _env_precision() if precision is None else precision)
    try:
        if pattern is None:
            h.set_matrix_csc(np.zeros(m + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), (n, m))
        else:
            h.set_matrix_csc(pattern.indptr, pattern.indices, np.ones(pattern.indices.size), (n, m))
        h.set_factors(W.shape[1], W, H)
    except BaseException:
        h.close()
        raise
    return h


def predict_entries(fit, rows, cols, precision=None):
    """(W H)[rows[e], cols[e]] of an nnmf() result as a float64 array, computed on the device from the factors alone: W H is never
    formed.  rows / cols: integer arrays of equal length, 0-based.  The scores are fp64 sums in both arithmetic modes (``precision``:
    nnlm_amd.PREC_F32 / PREC_F64, default NNLM_PRECISION's)."""
    W, H = _fit_factors(fit, "predict_entries")
    r, c = _index_arg(rows, "rows", W.shape[0]), _index_arg(cols, "cols", H.shape[1])
    if r.size != c.size:
        raise NnlmStop("rows and cols must have the same length (got %d and %d)." % (r.size, c.size))
    with _scoring_handle(W, H, None, precision) as h:
        return h.predict_entries(r, c)


def top_n(fit, n_top, by="column", lines=None, seen=None):
    """The n_top best-scoring rows of every listed column of W H (by = "column") or columns of every listed row (by = "row"), from the
    factors alone: (idx int32 [L, n_top], score float64 [L, n_top]), best first, equal scores by ascending index, (-1, NaN) behind a line
    with fewer candidates.  lines = None: every line of that side.  ``seen``: an object with tocsc() of the shape of W H -- typically the
    training matrix -- whose STORED entries are not candidates (stored zeros included); without it nothing is excluded."""
    W, H = _fit_factors(fit, "top_n")
    n, m = W.shape[0], H.shape[1]
    if by not in _lib.BY:
        raise NnlmStop("by must be 'column' or 'row' (got %r)." % (by,))
    n_top = int(n_top)
    if not 1 <= n_top <= _lib.TOPN_MAX:
        raise NnlmStop("n_top must be in 1 .. %d (got %d)." % (_lib.TOPN_MAX, n_top))
    ln = None if lines is None else _index_arg(lines, "lines", m if by == "column" else n)
    pattern = None
    if seen is not None:
        _refuse_device(seen, "top_n", "seen")
        if not is_sparse(seen):
            raise NnlmStop("seen must be a sparse matrix (an object with tocsc()): its stored entries are what is excluded.")
        if tuple(int(v) for v in seen.shape) != (n, m):
            raise NnlmStop("Dimension of seen %s does not match the fit (%d x %d)." % (tuple(seen.shape), n, m))
        pattern = as_csc(seen)
    with _scoring_handle(W, H, pattern, None) as h:
        return h.top_n(n_top, by=by, lines=ln, exclude=pattern is not None)


# ------------------------------------------------------------------------------------------------
# ranking evaluation of the top-n lists against held-out entries (nnlm_top_n_eval)
# ------------------------------------------------------------------------------------------------
def _csc_transposed(c):
    """The CSR of a canonical CSC as (pointers int64 [n + 1], column indices int32, ascending inside a row) and the permutation that
    takes the CSC's entries there."""
    n, m = c.shape
    cols = np.repeat(np.arange(m, dtype=np.int64), np.diff(c.indptr))
    order = np.argsort(np.asarray(c.indices, dtype=np.int64), kind="stable")  # (columns ascend inside a row: the sort is stable)
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(np.asarray(c.indices, dtype=np.int64), minlength=n), out=ptr[1:])
    return ptr, cols[order].astype(np.int32), order


def _cutoffs_arg(n_top):
    try:
        cut = _lib.index_array(np.atleast_1d(np.asarray(n_top)), "n_top")
    except ValueError as e:
        raise NnlmStop(str(e)) from None
    if not 1 <= cut.size <= _lib.TOPN_EVAL_MAX_CUT:
        raise NnlmStop("n_top must be one cutoff or 1 .. %d ascending cutoffs (got %d)." % (_lib.TOPN_EVAL_MAX_CUT, cut.size))
    if cut.min() < 1 or cut.max() > _lib.TOPN_MAX:
        raise NnlmStop("n_top must be in 1 .. %d (got %s)." % (_lib.TOPN_MAX, cut.tolist()))
    if np.any(np.diff(cut) <= 0):
        raise NnlmStop("n_top must hold strictly ascending cutoffs (got %s)." % (cut.tolist(),))
    return cut


def evaluate_top_n(fit, heldout, n_top=10, by="column", lines=None, seen=None, per_line=False):
    """Precision, recall, hit rate, NDCG, MAP and MRR at n_top of the lists top_n(fit, n_top, by, lines, seen) would return, against the
    entries of ``heldout`` -- computed on the device from the factors: neither W H nor the lists reach the host.  n_top: an int or up
    to 8 strictly ascending cutoffs in 1 .. 128.  heldout / seen: objects with tocsc() of the shape of W H; only the stored PATTERN of
    heldout is read, and it must not overlap seen (such an entry could never be listed).  A line is evaluated iff it is listed and holds
    a held-out entry.  Returns dict(cutoffs, n_evaluated, precision, recall, hit_rate, ndcg, map, mrr) -- each metric a float64 array
    over the cutoffs, the mean over the evaluated lines (NaN without any) -- and with per_line=True also lines, n_heldout, first_hit
    (-1: none), hits, dcg and ap (the line's average precision; NaN on a line that is not evaluated), arrays over the listed lines."""
    W, H = _fit_factors(fit, "evaluate_top_n")
    n, m = W.shape[0], H.shape[1]
    if by not in _lib.BY:
        raise NnlmStop("by must be 'column' or 'row' (got %r)." % (by,))
    cut = _cutoffs_arg(n_top)
    side = m if by == "column" else n
    ln = None if lines is None else _index_arg(lines, "lines", side)
    patterns = {}
    for name, x in (("heldout", heldout), ("seen", seen)):
        if x is None and name == "seen":
            continue
        _refuse_device(x, "evaluate_top_n", name)
        if not is_sparse(x):
            raise NnlmStop("%s must be a sparse matrix (an object with tocsc()): its stored entries are what is %s." %
                           (name, "held out" if name == "heldout" else "excluded"))
        if tuple(int(v) for v in x.shape) != (n, m):
            raise NnlmStop("Dimension of %s %s does not match the fit (%d x %d)." % (name, tuple(x.shape), n, m))
        patterns[name] = as_csc(x)
    held, pattern = patterns["heldout"], patterns.get("seen")
    hp, hi = (held.indptr, held.indices) if by == "column" else _csc_transposed(held)[:2]
    with _scoring_handle(W, H, pattern, None) as h:
        try:
            out = h.top_n_eval(cut, by=by, lines=ln, exclude=pattern is not None, held_ptr=hp, held_idx=hi, per_line=per_line)
        except _lib.NnlmError as e:
            if e.code == _lib.ERR_ARG and "is stored in the resident matrix" in str(e):
                raise NnlmStop("heldout overlaps seen: %s" % (e,)) from None
            raise
    if per_line:
        t = out["n_heldout"]
        with np.errstate(divide="ignore", invalid="ignore"):
            out["ap"] = out.pop("apn") / np.minimum(cut[None, :], t[:, None])
        out["lines"] = np.arange(side, dtype=np.int32) if ln is None else ln.copy()
    return out


def holdout_split(A, per_line=1, by="column", min_keep=1, rng=None):
    """Leave-some-out split of a sparse A for ranking evaluation, on the host: (train, heldout), two CSC with disjoint patterns whose union
    is A's (values kept).  Every line (column for by = "column", row for "row") with more than min_keep stored entries gives up
    min(per_line, stored - min_keep) of them, drawn without replacement from ``rng`` (a numpy Generator, a seed, or None); lines with at
    most min_keep entries keep everything.  The same rng state gives the same split.  train is what one fits and passes as seen=."""
    if not is_sparse(A):
        raise NnlmStop("A must be a sparse matrix (an object with tocsc()).")
    if by not in _lib.BY:
        raise NnlmStop("by must be 'column' or 'row' (got %r)." % (by,))
    per_line, min_keep = int(per_line), int(min_keep)
    if per_line < 1 or min_keep < 0:
        raise NnlmStop("per_line must be >= 1 and min_keep >= 0 (got %d and %d)." % (per_line, min_keep))
    c = as_csc(A)
    rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
    if by == "column":
        ptr, where = c.indptr, None
    else:
        ptr, _, where = _csc_transposed(c)  # (where: the CSC position of each entry in row order)
    out = np.zeros(c.indices.size, dtype=bool)
    counts = np.diff(ptr)
    for l in np.flatnonzero(counts > min_keep):  # (lines in ascending order: the draws are a function of the rng state alone)
        take = int(min(per_line, counts[l] - min_keep))
        e = ptr[l] + rng.choice(int(counts[l]), size=take, replace=False)
        out[e if where is None else where[e]] = True
    cols = np.repeat(np.arange(c.shape[1], dtype=np.int64), np.diff(c.indptr))

    def part(keep):
        indptr = np.zeros(c.shape[1] + 1, dtype=np.int64)
        np.cumsum(np.bincount(cols[keep], minlength=c.shape[1]), out=indptr[1:])
        return CSC(indptr, np.ascontiguousarray(c.indices[keep]), np.ascontiguousarray(c.data[keep]), c.shape)
    return part(~out), part(out)
