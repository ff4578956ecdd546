"""Reference for per-entry weights on a sparse A (nnlm_set_matrix_csc_weighted), shared by test_weighted_host.py and
test_gpu_sparse_weighted.py.

The loss is 1/2 sum over the observed entries of c (a - (WH))^2 + the reference's penalties.  Column j of a half-step is therefore the
reference's update() / update_with_missing() on the one-column problem whose rows are scaled by sqrt(c_ij): x' = diag(sqrt(c_j)) Y,
y' = sqrt(c_j) * a_j.  half_step() calls the C oracle (oracle.ref.update) on exactly that, column by column: NaN at the absent rows and
missing = True for absent = "missing"; the dense column with weight 1 at the absent rows for absent = "zero".  c_nnmf() restates the
outer loop of nnlm_oracle.c_nnmf around that half-step, with the weighted traces (N = nnz or n m; eps = TINY):
  mse = sum_obs c (a - wh)^2 / N,   mkl = kl_const_w + sum_obs c (-(a + eps) log(wh + eps) + wh) / N,
  kl_const_w = (sum_stored c ((a + eps) log(a + eps) - a) + [absent = zero: (n m - nnz) eps log eps]) / N,
  target = mse / 2 + add_penalty(..., N).
Small matrices only: everything here is dense."""
import math

import numpy as np

from oracle import nnlm_oracle, ref

TINY = nnlm_oracle.TINY_NUM


class Csc:
    """numpy-only duck-typed sparse matrix (what api.nnmf accepts from scipy)."""

    def __init__(self, csc):
        self.indptr, self.indices, self.data, self.shape = csc

    def tocsc(self):
        return self

    @property
    def T(self):
        return Csc(transpose(self.indptr, self.indices, self.data, self.shape))


def csc_from_flat(flat, vals, n, m):
    """CSC from sorted, unique column-major flat indices j * n + i."""
    flat = np.asarray(flat, dtype=np.int64)
    cols, rows = flat // n, flat % n
    indptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=m), out=indptr[1:])
    return indptr, rows.astype(np.int32), np.asarray(vals, dtype=np.float64), (n, m)


def rand_csc(n, m, density, rng):
    nnz = int(round(density * n * m))
    flat = np.sort(rng.choice(n * m, size=nnz, replace=False)) if nnz < n * m else np.arange(n * m)
    return csc_from_flat(flat, rng.random(flat.size), n, m)


def transpose(indptr, idx, val, shape):
    """Canonical CSC of the transpose."""
    n, m = shape
    cols = np.repeat(np.arange(m, dtype=np.int64), np.diff(indptr))
    rows = np.asarray(idx, dtype=np.int64)
    order = np.lexsort((cols, rows))
    return csc_from_flat(rows[order] * m + cols[order], np.asarray(val)[order], m, n)


def dense_parts(S, weights, absent):
    """(A, C, obs) of a weighted sparse matrix: A n x m with 0 at the absent entries, C the weight of every entry (the stored ones' own,
    an absent one's 1 for absent = "zero" and 0 for "missing"), obs the observed entries (the stored ones, or all of them)."""
    indptr, idx, val, (n, m) = S
    cols = np.repeat(np.arange(m), np.diff(indptr))
    A = np.zeros((n, m))
    A[idx, cols] = val
    stored = np.zeros((n, m), dtype=bool)
    stored[idx, cols] = True
    C = np.full((n, m), 1.0 if absent == "zero" else 0.0)
    C[idx, cols] = weights
    obs = np.ones((n, m), dtype=bool) if absent == "zero" else stored
    return A, C, obs


def half_step(H, Wt, A, C, obs, mask, reg, max_iter, rel_tol, method, missing, counts=None):
    """One half-step for H (k x m) with Wt (k x n) fixed: the C oracle on the sqrt(c)-scaled one-column problem of every column.
    Returns (H_new, sweeps).  counts: a list that receives the sweeps of every column."""
    H = np.array(H, dtype=np.float64, copy=True)
    Wt = np.asarray(Wt, dtype=np.float64)
    total = 0
    for j in range(H.shape[1]):
        sc = np.sqrt(C[:, j])
        y = sc * A[:, j]
        if missing:
            y = np.where(obs[:, j], y, np.nan)
        mj = None if mask is None else np.asarray(mask)[:, j:j + 1]
        hj, it = ref.update(H[:, j:j + 1], Wt * sc[None, :], y[:, None], mj, reg, max_iter, rel_tol, method, missing=missing)
        H[:, j] = hj[:, 0]
        total += it
        if counts is not None:
            counts.append(int(it))
    return H, total


def kl_const(S, weights, absent):
    indptr, idx, val, (n, m) = S
    w = np.asarray(weights, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = float(np.sum(w * ((val + TINY) * np.log(val + TINY) - val)))
    if absent == "zero":
        return (s + (float(n) * m - val.size) * (TINY * math.log(TINY))) / (float(n) * m)
    return s / val.size


def errors(A, C, obs, Wt, H, N):
    """(mse, the variable part of mkl) of the weighted loss."""
    Ahat = Wt.T @ H
    with np.errstate(divide="ignore", invalid="ignore"):
        d = A - Ahat
        mse = float(np.sum((C * d * d)[obs])) / N
        kl = float(np.sum((C * (-(A + TINY) * np.log(Ahat + TINY) + Ahat))[obs])) / N
    return mse, kl


def c_nnmf(S, weights, absent, k, W, H, Wm, Hm, alpha, beta, max_iter, rel_tol, inner_max_iter, inner_rel_tol, method, trace,
           show_warning=False):
    """The loop of nnlm_oracle.c_nnmf (src/nnmf.cpp:4-220) around half_step(), W (n x k) and H (k x m) given."""
    A, C, obs = dense_parts(S, weights, absent)
    n, m = A.shape
    missing = absent == "missing"
    N = float(S[2].size) if missing else float(n) * m
    trace = max(int(trace), 1)
    err_len = int(math.ceil(float(max_iter) / float(trace))) + 1
    mse_err, terr, ave_epoch = np.zeros(err_len), np.zeros(err_len), np.zeros(err_len)
    mkl_err = np.full(err_len, kl_const(S, weights, absent))
    Wmt = None if Wm is None or np.size(Wm) == 0 else np.ascontiguousarray(np.asarray(Wm).T)
    Hmm = None if Hm is None or np.size(Hm) == 0 else np.asarray(Hm)
    Wt = np.array(np.asarray(W, dtype=np.float64).T, order="C", copy=True)
    Hc = np.array(H, dtype=np.float64, copy=True)
    At, Ct, obst = np.ascontiguousarray(A.T), np.ascontiguousarray(C.T), np.ascontiguousarray(obs.T)
    rel_err, terr_last = rel_tol + 1.0, 1e99
    total_raw_iter = i = i_e = 0

    def error_block(i_e, total_raw_iter, terr_last):
        mse, kl = errors(A, C, obs, Wt, Hc, N)
        mse_err[i_e] = mse
        mkl_err[i_e] += kl
        ave_epoch[i_e] = float(total_raw_iter) / (n + m)
        t = nnlm_oracle.add_penalty(0.5 * mse_err[i_e], Wt, Hc, N, alpha, beta)
        terr[i_e] = t
        return 2 * (terr_last - t) / (terr_last + t + TINY), t

    while i < max_iter and abs(rel_err) > rel_tol:
        Wt, it = half_step(Wt, Hc, At, Ct, obst, Wmt, alpha, inner_max_iter, inner_rel_tol, method, missing)
        total_raw_iter += it
        Hc, it = half_step(Hc, Wt, A, C, obs, Hmm, beta, inner_max_iter, inner_rel_tol, method, missing)
        total_raw_iter += it
        if i % trace == 0:
            rel_err, terr_last = error_block(i_e, total_raw_iter, terr_last)
            total_raw_iter = 0
            i_e += 1
        i += 1
    if ((i - 1) & 0xFFFFFFFF) % trace != 0:  # unsigned arithmetic, src/nnmf.cpp:164
        rel_err, terr_last = error_block(i_e, total_raw_iter, terr_last)
        i_e += 1
    return dict(W=Wt.T.copy(), H=Hc, mse_error=mse_err[:i_e].copy(), mkl_error=mkl_err[:i_e].copy(), target_error=terr[:i_e].copy(),
                average_epoch=ave_epoch[:i_e].copy(), n_iteration=i, warning=bool(show_warning and rel_err > rel_tol))
