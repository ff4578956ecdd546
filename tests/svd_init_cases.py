"""Numpy restatement of the library's truncated SVD (randomised subspace iteration, Gram-based orth run twice) and NNDSVD start, and
the test matrices of tests/test_svd_init_host.py and tests/test_gpu_svd_init.py.

The restatement follows include/nnlm_mi355x.h (nnlm_svd, nnlm_set_factors_nndsvd) step by step on the same sketch matrix omega; it has
numpy.linalg.eigh where the library has its host Jacobi.  Factors are kept as the handle keeps them: one ROW per component.
`rnd` rounds every cross-product operand (A, and the factor that multiplies it); the identity restates the strict mode, round22 emulates
the 22 significant bits of the split-fp16 copies of the fp32-operand mode."""
from collections import namedtuple

import numpy as np

DROP = 1e-12  # a direction whose Gram eigenvalue is at most DROP * the largest is dropped (orth) / has sigma = 0 (last step)


def round22(x):
    """x rounded to 22 significant bits (hi + lo 2^-11 of two fp16 numbers)."""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(np.round(m * 2.0 ** 22) / 2.0 ** 22, e)


def _eigh_desc(G):
    lam, E = np.linalg.eigh((G + G.T) / 2)
    return lam[::-1], E[:, ::-1]


def orth(X):
    """(orth(X), directions kept by the second pass)."""
    kept = 0
    for _ in range(2):
        lam, E = _eigh_desc(X @ X.T)
        keep = (lam > DROP * lam[0]) & (lam[0] > 0)
        d = np.where(keep, 1.0 / np.sqrt(np.where(keep, lam, 1.0)), 0.0)
        X = (d[:, None] * E.T) @ X
        kept = int(keep.sum())
    return X, kept


def rsvd(A, omega, q, rnd=None):
    """(U l x n, sigma l, Vt l x m, kept) of A from the l x m sketch matrix omega and q power iterations."""
    rnd = rnd or (lambda x: x)
    Ar = rnd(A)
    Q, kept = orth(rnd(omega) @ Ar.T)
    for _ in range(q):
        Z, _ = orth(rnd(Q) @ Ar)
        Q, kept = orth(rnd(Z) @ Ar.T)
    B = rnd(Q) @ Ar
    lam, E = _eigh_desc(B @ B.T)
    pos = (lam > DROP * lam[0]) & (lam[0] > 0)
    sig = np.where(pos, np.sqrt(np.where(pos, lam, 0.0)), 0.0)
    U = E.T @ Q
    Vt = np.where(pos[:, None], (E.T @ B) / np.where(pos, sig, 1.0)[:, None], 0.0)
    return U, sig, Vt, kept


def nndsvd(U, sig, Vt, k, fill=0.0):
    """NNDSVD (Boutsidis & Gallopoulos 2008) of the first k triplets (rows of U and Vt) -> (W n x k, H k x m); fill replaces every exact
    zero (nndsvda: fill = mean(A))."""
    n, m = U.shape[1], Vt.shape[1]
    W, H = np.zeros((n, k)), np.zeros((k, m))
    W[:, 0], H[0] = np.sqrt(sig[0]) * np.abs(U[0]), np.sqrt(sig[0]) * np.abs(Vt[0])
    for j in range(1, k):
        up, un, vp, vn = np.maximum(U[j], 0), np.maximum(-U[j], 0), np.maximum(Vt[j], 0), np.maximum(-Vt[j], 0)
        nup, nun, nvp, nvn = (np.sqrt((x * x).sum()) for x in (up, un, vp, vn))
        if nup * nvp >= nun * nvn:
            pu, pv, nu, nv = up, vp, nup, nvp
        else:
            pu, pv, nu, nv = un, vn, nun, nvn
        st = sig[j] * nu * nv
        if st > 0:
            W[:, j], H[j] = np.sqrt(st) / nu * pu, np.sqrt(st) / nv * pv
    if fill:
        W[W == 0], H[H == 0] = fill, fill
    return W, H


def exact_nndsvd(A, k, fill=0.0):
    u, s, vt = np.linalg.svd(A, full_matrices=False)
    return nndsvd(u.T, s, vt, k, fill)


def align(U, Vt, Uref, Vtref):
    """U, Vt with the joint sign of every triplet turned to that of the reference."""
    sg = np.sign(np.einsum("ij,ij->i", U, Uref) + np.einsum("ij,ij->i", Vt, Vtref))
    sg[sg == 0] = 1.0
    return U * sg[:, None], Vt * sg[:, None]


def _edges(g, total, parts):
    """parts contiguous non-empty blocks of range(total) with random edges."""
    cuts = np.sort(g.choice(np.arange(1, total), size=parts - 1, replace=False))
    return np.concatenate([[0], cuts, [total]])


Case = namedtuple("Case", "name n m k l blocks noise A Wc Hc omega")


def make_case(name, n, m, k, blocks=None, noise=0.0, oversample=10, seed=0):
    """A = sum_j s_j a_j b_j^T on `blocks` disjoint row and column blocks (default k), a_j, b_j > 0 of unit norm, s_j = 1.06^-j: the
    singular triplets are (s_j, a_j, b_j), and the NNDSVD of the first k is W[:, j] = sqrt(s_j) a_j, H[j] = sqrt(s_j) b_j (Wc, Hc),
    W H = A exactly when blocks = k.  noise: + noise * U(0, 1).  omega: the l x m sketch matrix, l = min(k + oversample, n, m)."""
    blocks = blocks or k
    g = np.random.default_rng([seed, n, m, k, blocks])
    re, ce = _edges(g, n, blocks), _edges(g, m, blocks)
    A, Wc, Hc = np.zeros((n, m)), np.zeros((n, k)), np.zeros((k, m))
    for j in range(blocks):
        a, b = g.uniform(0.5, 1.5, re[j + 1] - re[j]), g.uniform(0.5, 1.5, ce[j + 1] - ce[j])
        a, b = a / np.sqrt((a * a).sum()), b / np.sqrt((b * b).sum())
        s = 1.06 ** -j
        A[re[j]:re[j + 1], ce[j]:ce[j + 1]] = s * np.outer(a, b)
        if j < k:
            Wc[re[j]:re[j + 1], j], Hc[j, ce[j]:ce[j + 1]] = np.sqrt(s) * a, np.sqrt(s) * b
    if noise:
        A = A + noise * g.random((n, m))
    l = min(k + oversample, n, m)
    omega = (2.0 * g.random(l * m) - 1.0).reshape((l, m), order="F")
    return Case(name, n, m, k, l, blocks, noise, A, Wc, Hc, omega)


# Shapes against the paddings (rows to 256, columns to 128, rank to 16); 300 x 200 at k 60 has l = 70: the rank > 64 launches
SHAPES = [("150x90_k6", 150, 90, 6, None), ("257x129_k17", 257, 129, 17, None), ("515x131_k50", 515, 131, 50, None),
          ("300x200_k60", 300, 200, 60, None), ("300x200_k12of40", 300, 200, 12, 40)]
_cache = {}


def case(name, noise=0.0):
    key = (name, noise)
    if key not in _cache:
        nm, n, m, k, blocks = next(s for s in SHAPES if s[0] == name)
        _cache[key] = make_case(nm + ("_noisy" if noise else ""), n, m, k, blocks, noise)
    return _cache[key]


def all_cases():
    """Every shape noise-free and with 1e-4 U(0, 1) added."""
    return [case(s[0], noise) for s in SHAPES for noise in (0.0, 1e-4)]


def wide_case():
    """The noisy 300 x 200, k 60 matrix with a sketch of width 150 (padded to 160): 32 columns of X and all of T no longer fit 64 KB of
    LDS, so the rotation kernel takes T's rows in chunks under the large LDS grant -- the form every width from about 100 on runs."""
    key = ("wide", 1e-4)
    if key not in _cache:
        _cache[key] = make_case("300x200_k60_noisy_l150", 300, 200, 60, None, 1e-4, oversample=90)
    return _cache[key]


def csc_of(A):
    """(indptr int64, indices int32, data, shape) of the non-zeros of the dense A."""
    n, m = A.shape
    nz = A.T != 0  # [m][n]: column after column
    cols, rows = np.nonzero(nz)
    indptr = np.concatenate([[0], np.cumsum(nz.sum(axis=1))]).astype(np.int64)
    return indptr, rows.astype(np.int32), np.ascontiguousarray(A.T[nz]), (n, m)


class SparseCSC:
    """The least a sparse object needs for the Python routes: tocsc() yielding indptr, indices, data, shape."""

    def __init__(self, A):
        self.indptr, self.indices, self.data, self.shape = csc_of(A)

    def tocsc(self):
        return self


_ref = {}


def reference(c, q=2):
    """The strict restatement of case c, computed once: dict(U, s, Vt, kept, W, H)."""
    key = (c.name, q)
    if key not in _ref:
        U, s, Vt, kept = rsvd(c.A, c.omega, q)
        W, H = nndsvd(U, s, Vt, c.k)
        _ref[key] = dict(U=U, s=s, Vt=Vt, kept=kept, W=W, H=H)
    return _ref[key]


def deviation(W, H, Wref, Href):
    """max |X - Xref| / max |Xref| over both factors."""
    return max(np.abs(W - Wref).max() / np.abs(Wref).max(), np.abs(H - Href).max() / np.abs(Href).max())


# The fp32-operand mode's bar on that deviation: ten times the worst deviation of the restatement with every cross-product operand
# rounded to 22 bits from the unrounded restatement, over all cases at q = 2 (tests/test_svd_init_host.py measures it and asserts that it
# stays below F32_EMULATED; the factor ten covers the summation order and the fp32 partial sums the emulation does not model).
F32_EMULATED = 4.6e-7  # measured 1.9e-7 .. 4.51e-7 (worst: 300 x 200, k 60, noisy, relative gap 1.7e-3)
F32_BAR = 10 * F32_EMULATED
