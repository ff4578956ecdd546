"""Cases for the error block of a sparse A (tests/test_gpu_sparse_error_block.py) and the conditions on them
(tests/test_sparse_err_cases_host.py): numpy only, importable without a GPU, deterministic in (family, n, m, k).

errors_launch() (nnlm_mi355x.hip) forms mse_error and the variable part of mkl_error of a sparse handle from sums over the stored entries
(k_sparse.h), one worker of LW lanes per about 64 stored entries, LW = 16 / 32 / 64 at KP = 16 / 32 / more:
  sp_errors_kernel<T, LW, MISS>       doors "zero" (set_matrix_csc) and "missing" (set_matrix_csc_missing)   2 types x 3 LW x 2 = 12
  sp_errors_weighted_kernel<T, LW>    doors "weighted_zero" and "weighted_missing"                           2 types x 3 LW     =  6
and, when an absent entry is a zero, the zeros' share from the Grams of the factors and their sums (launch_gram_partial,
sp_rowsum_partial_kernel, sp_err_final_kernel / sp_err_final_weighted_kernel; absent = missing: sp_err_final_missing_kernel or the
other branch of the weighted one).  form_of() restates which form a (mode, door, rank) reaches.

Families, following err_cases.py.  "ones" and "planted": W and H integers in {1, 2, 3} with one zero row of W and one zero column of H,
weights integers in {0, 1, 2, 3, 5}, every stored a = wh + 1, respectively a = wh except at up to 11 stored entries where
a = wh + 2^t, t = 0 .. 10 -- the first and the last stored entry of worker ranges (sparse_cases.sp_workers / split_of at the rank's KP),
on both sides of a worker boundary, a wavefront boundary and a workgroup boundary.  Every quantity a kernel forms is then an integer
below 2^53 (below 2^24 where a kernel holds it in fp32: the stored values and weights of the fp32-operand mode and the operands of its
Gram), so the sum of squares is EXACTLY
  absent = missing:  sum over the stored entries of c (r = 1)  /  of c 4^t over the planted ones
  absent = zero:     that sum + the sum over the absent entries of wh^2
and mse == float(that integer) / N to the bit (nnlm_errors divides the sum once by n_non_missing: the stored entries, or n m).  An
entry dropped, counted twice or weighted wrongly moves the sum by at least 1.  "uniform" rounds and is held to a long double reference
(ld_errors: weighted_cases.errors with long double terms and sums)."""
import collections
import functools

import numpy as np

import err_cases as ec
import sparse_cases as spc
import weighted_cases as wc
import weighted_form_cases as wf

DOORS = ("zero", "missing", "weighted_zero", "weighted_missing")
ABSENT = {"zero": "zero", "missing": "missing", "weighted_zero": "zero", "weighted_missing": "missing"}
WEIGHTED = {"zero": False, "missing": False, "weighted_zero": True, "weighted_missing": True}
MODES = ("f64", "f32")
MAIN = ec.MAIN
SHAPES_OTHER = ((1, 1), (63, 65), (257, 70))
RANKS_ALL, RANKS_FEW, RANKS_GENERIC = ec.RANKS_ALL, ec.RANKS_FEW, ec.RANKS_GENERIC
FAMILIES = ("ones", "planted", "uniform")
EXACT = ("ones", "planted")
EXACT_WEIGHTS = (0, 1, 2, 3, 5)
DENSITY = 0.3
KQ_MAX = 64


def accepts(door, k):
    """Only set_matrix_csc takes a rank above 64 (nnlm_set_factors refuses it on the other three doors)."""
    return door == "zero" or k <= KQ_MAX


def form_of(mode, door, k):
    """The template instantiation that sums over the stored entries."""
    T, LW = wf.TYPE_OF[mode], spc.sp_lanes(spc.kp_of(k))
    if WEIGHTED[door]:
        return ("sp_errors_weighted_kernel", T, LW)
    return ("sp_errors_kernel", T, LW, ABSENT[door] == "missing")


def all_forms():
    out = {("sp_errors_weighted_kernel", T, LW) for T in ("double", "float") for LW in (16, 32, 64)}
    return out | {("sp_errors_kernel", T, LW, miss) for T in ("double", "float") for LW in (16, 32, 64) for miss in (False, True)}


def groups():
    """[(shape, k)] of the GPU test: every rank at MAIN (and 65, 70, which only the zero door takes), RANKS_FEW at the other shapes."""
    return [(MAIN, k) for k in RANKS_ALL + RANKS_GENERIC] + [(s, k) for s in SHAPES_OTHER for k in RANKS_FEW]


def pattern(n, m, rng):
    """About 30 % stored; the first and the last column and one row empty (shapes that have three lines to spare)."""
    P = rng.random((n, m)) < DENSITY
    if m >= 3:
        P[:, 0] = False
        P[:, m - 1] = False
    if n >= 9:
        P[7, :] = False
    if not P.any():
        P[n - 1, m // 2] = True
    return P


def planted_positions(nnz, k):
    """[(stored entry e in CSC order, t)]: a = wh + 2^t at e.  The entries are the last of worker w - 1 and the first of worker w for the
    second worker, the first worker of the second wavefront and of the second workgroup and the last worker, then the last and the first
    entry of all and the first of a middle worker."""
    KP = spc.kp_of(k)
    nw = spc.sp_workers(nnz, KP)
    _, ranges = spc.split_of(nnz, nw)
    ng = 64 // spc.sp_lanes(KP)
    pos = []
    last = max(w for w in range(nw) if ranges[w][0] < ranges[w][1]) if nnz else 0   # (rounding the share up can leave the last workers empty)
    for w in sorted({1, ng, 4 * ng, last}):
        if 0 < w < nw and ranges[w][0] < ranges[w][1]:
            pos += [ranges[w][0] - 1, ranges[w][0]]
    pos += [nnz - 1, 0, ranges[nw // 2][0]]
    out = []
    for p in pos:
        if 0 <= p < nnz and p not in [q for q, _ in out] and len(out) < 11:
            out.append((p, len(out)))
    return out


Case = collections.namedtuple("Case", "family n m k")


@functools.lru_cache(maxsize=8)
def make_case(family, n, m, k):
    """dict(S the CSC, W, H, w the weights of the weighted doors, planted [(e, t)])."""
    rng = np.random.default_rng([31, FAMILIES.index(family), n, m, k])
    P = pattern(n, m, rng)
    planted = []
    if family in EXACT:
        W = rng.integers(1, 4, (n, k)).astype(np.float64)
        H = rng.integers(1, 4, (k, m)).astype(np.float64)
    else:
        W, H = rng.random((n, k)), rng.random((k, m))
    if n >= 3:
        W[n // 2, :] = 0.0
    if m >= 3:
        H[:, m // 2] = 0.0
    if family in EXACT:
        S = spc.csc_from_pattern(P, W @ H)
        val = S[2].copy()
        if family == "ones":
            val += 1.0
        else:
            planted = planted_positions(val.size, k)
            for e, t in planted:
                val[e] += 2.0 ** t
        S = (S[0], S[1], val, S[3])
        w = rng.choice(EXACT_WEIGHTS, val.size).astype(np.float64)
    else:
        S = spc.csc_from_pattern(P, rng.random((n, m)))
        w = None
    return dict(S=S, W=W, H=H, w=w, planted=planted, P=P)


def weights_of(c, door, family):
    """The weights a door is given: None for the unweighted doors."""
    if not WEIGHTED[door]:
        return None
    if family in EXACT:
        return c["w"]
    return wf.draw_weights(door, c["S"][2].size, np.random.default_rng(c["S"][2].size + DOORS.index(door)))


def dense_of(c, door, family):
    """(A, C, obs) of weighted_cases.dense_parts: the unweighted doors weigh every stored entry 1."""
    w = weights_of(c, door, family)
    return wc.dense_parts(c["S"], np.ones(c["S"][2].size) if w is None else w, ABSENT[door])


def n_observed(c, door):
    n, m = c["S"][3]
    return c["S"][2].size if ABSENT[door] == "missing" else n * m


def exact_sum(c, door, family):
    """The sum of squares of an exact family as a Python int."""
    A, C, obs = dense_of(c, door, family)
    wh = np.rint(c["W"] @ c["H"]).astype(np.int64)
    r = np.rint(A).astype(np.int64) - wh
    stored = c["P"]
    total = int((np.rint(C).astype(np.int64) * r * r)[stored].sum())
    if ABSENT[door] == "zero":
        total += int((wh * wh)[~stored].sum())
    return total


def integer_bounds(c, door, family):
    """(largest integer any sum reaches in fp64, largest number a kernel holds in fp32) of an exact family."""
    A, C, obs = dense_of(c, door, family)
    W, H = c["W"], c["H"]
    wh = W @ H
    GW, GH = W.T @ W, H @ H.T
    sums = [float((C * (A - wh) ** 2)[obs].sum()), float((wh * wh).sum()), float((C * wh)[c["P"]].sum()), float(wh.sum()), float((GW * GH).sum()),
            float(W.sum(axis=0) @ H.sum(axis=1))]
    held32 = [float(A.max()), float(C.max()), float(GW.max()), float(GH.max()), float(W.max()), float(H.max())]
    return max(sums), max(held32)


Ref = collections.namedtuple("Ref", "s2 kl abs2 abskl N")
LD = ec.LD


def ld_errors(A, C, obs, W, H, N):
    """weighted_cases.errors with long double terms and sums: Ref(sum of c (a - wh)^2, sum of c (-(a + eps) log(wh + eps) + wh), the sums of
    |term| of both, N) over the observed entries."""
    integer = np.array_equal(W, np.rint(W)) and np.array_equal(H, np.rint(H))
    wh = (W @ H).astype(LD) if integer else np.einsum("iq,qj->ij", W.astype(LD), H.astype(LD))
    a, c, wh = A[obs].astype(LD), C[obs].astype(LD), wh[obs]
    d = a - wh
    t2 = c * d * d
    tiny = LD(ec.TINY)
    tk = c * (-(a + tiny) * np.log(wh + tiny) + wh)
    return Ref(t2.sum(dtype=LD), tk.sum(dtype=LD), np.abs(t2).sum(dtype=LD), np.abs(tk).sum(dtype=LD), N)


_REFS = {}


def ref_of(case, door):
    """ld_errors of a case through a door (scalars only are kept; both modes and the host test share one evaluation)."""
    key = (case, door)
    if key not in _REFS:
        c = make_case(*case)
        A, C, obs = dense_of(c, door, case.family)
        _REFS[key] = ld_errors(A, C, obs, c["W"], c["H"], n_observed(c, door))
    return _REFS[key]
