"""Cases for the ingest of a sparse matrix WITH per-entry weights that both live in device memory (nnlm_set_matrix_sparse_device_weighted,
k_sparse_ingest.h): cases only, no tests.  The matrices are sparse_device_cases' (the smallest shapes at which a stage of the ingest can go
wrong); this module adds the weights of each case, numpy's restatement of the ten resident arrays, the statistics the host entry's loop
accumulates, and the malformed weights of the refusal tests.  numpy alone."""
import numpy as np

import sparse_device_cases as sdc

FP32_MAX = 3.4028234663852886e38
FP32_FLOOR = 7.8886090522101181e-31
TINY = 1e-16  # NNLM_TINY (common.h)
ABSENT = ("missing", "zero")
WEIGHT_DTYPES = sdc.VAL_DTYPES


def case_names(share, tile):
    """sparse_device_cases' names without the fourth-pass case (2^24 + 1 lines: pointer-array memory only, no payload path of its own)."""
    return [c for c in sdc.case_names(share, tile) if c != "lines_16777217"]


def weights(name, nnz):
    """One weight per stored entry, seeded from the case's name: a quarter each of 1 + 40 u (not representable in the narrow types, nor is
    its product with the value), multiples of 1 / 8 below 8 (exact everywhere), weight 1 and weight 0."""
    rng = np.random.default_rng([ord(ch) for ch in name + ":weights"])
    kind = rng.integers(0, 4, size=nnz)
    w = 1.0 + 40.0 * rng.random(nnz)
    w[kind == 1] = rng.integers(0, 64, size=nnz)[kind == 1] / 8.0
    w[kind == 2] = 1.0
    w[kind == 3] = 0.0
    return w


def order_of_other_side(S):
    """The permutation that takes the stored entries of the CSC S to the order of its rows (stable: columns ascending within a row)."""
    return np.argsort(S[1], kind="stable")


def mode_round(x, f64):
    return x if f64 else x.astype(np.float32).astype(np.float64)


def resident(S, w, f64):
    """numpy's restatement of the ten resident arrays: per side (ptr, idx, val, weights, weights * values), the last three rounded to the
    mode's type; the product is formed in fp64 BEFORE the rounding, once per entry."""
    ptr, idx, val, _ = S
    rptr, cidx, rval = sdc.other_side(S)
    o = order_of_other_side(S)
    wa = w * val
    return ((ptr, idx, mode_round(val, f64), mode_round(w, f64), mode_round(wa, f64)),
            (rptr, cidx, mode_round(rval, f64), mode_round(w[o], f64), mode_round(wa[o], f64)))


def loop_statistics(val, w):
    """(over, max |(float) a|, max |(float)(c a)|, weighted KL sum) entry by entry, as the host entry's loop accumulates them."""
    over = mx = wmx = klc = 0.0
    for v, c in zip(val.tolist(), w.tolist()):
        if abs(v) > FP32_MAX:
            over += 1.0
        mx = max(mx, abs(float(np.float32(v))))
        ca = c * v
        if abs(v) <= FP32_MAX and (abs(ca) > FP32_MAX or c > FP32_MAX):
            over += 1.0
        with np.errstate(over="ignore"):  # (a product beyond fp32 becomes +-Inf, as the host's cast makes it)
            wmx = max(wmx, abs(float(np.float32(ca))))
        klc += c * ((v + TINY) * np.log(v + TINY) - v)
    return over, mx, wmx, klc


def direct_statistics(val, w):
    """The same four numbers from whole-array expressions."""
    with np.errstate(over="ignore", invalid="ignore"):
        ca = w * val
        over = np.count_nonzero((np.abs(val) > FP32_MAX) | (np.abs(ca) > FP32_MAX) | (w > FP32_MAX))
        mx = float(np.abs(val.astype(np.float32)).max(initial=0.0))
        wmx = float(np.abs(ca.astype(np.float32)).max(initial=0.0))
        klc = float(np.sum(w * ((val + TINY) * np.log(val + TINY) - val)))
    return float(over), mx, wmx, klc


# ---- malformed weights: values in valid arrays, never addresses -------------------------------------------------------------------------------
OFFENCES = {"nan": np.nan, "inf": np.inf, "minus_one": -1.0}
LEGAL = {"minus_zero": -0.0}


def offence_positions(nnz, share):
    """The first entry, the last one and both sides of the first boundary between two check blocks."""
    assert nnz > share + 1
    return {"first": 0, "below_share": share - 1, "at_share": share, "last": nnz - 1}


def with_weight(w, e, value):
    out = w.copy()
    out[e] = value
    return out


def range_rule_inputs(S):
    """name -> (values, weights, what the fp32 mode says): the three ways the weights alone can trip the fp32 range rules."""
    val = S[2]
    nnz = val.size
    mid = nnz // 2
    ones = np.ones(nnz)
    v0 = val.copy()
    v0[mid] = 0.0
    c_alone = (v0, with_weight(ones, mid, 1e39), "1 entries of A (or their weights, or weight * A) exceed the fp32 range")
    v1 = val.copy()
    v1[mid] = 1e20
    ca_alone = (v1, with_weight(ones, mid, 1e20), "1 entries of A (or their weights, or weight * A) exceed the fp32 range")
    floor = (np.full(nnz, 1e-15), np.full(nnz, 1e-20), "max |weight * A| = 1e-35 is too close to the bottom of the fp32 range")
    return {"c_alone": c_alone, "ca_alone": ca_alone, "wmx_floor": floor}


def pattern_changes(S):
    """name -> ((ptr, idx) of a weights pattern that differs from S's, nnz of it, the first line that differs): one index changed, one
    entry moved to the next line with nnz unchanged, one entry dropped."""
    ptr, idx, _, (n, m) = S
    lens = np.diff(ptr)
    out = {}
    # one index changed: the last entry of a line that does not end at row n - 1 moves one row down
    for j in range(m // 2, m):
        if lens[j] and idx[ptr[j + 1] - 1] < n - 1:
            i2 = idx.copy()
            i2[ptr[j + 1] - 1] += 1
            out["index_changed"] = ((ptr, i2), idx.size, j)
            break
    # one entry moved to the next line: line j loses its last entry, line j + 1 gains a first one
    for j in range(m // 3, m - 1):
        if lens[j] and lens[j + 1] and idx[ptr[j + 1]] > 0:
            p2, i2 = ptr.copy(), idx.copy()
            p2[j + 1] -= 1
            i2[p2[j + 1]] = 0
            out["entry_moved"] = ((p2, i2), idx.size, j)
            break
    # a different nnz: line j loses its last entry
    for j in range(m // 4, m):
        if lens[j]:
            p2 = ptr.copy()
            p2[j + 1:] -= 1
            out["other_nnz"] = ((p2, np.delete(idx, ptr[j + 1] - 1)), idx.size - 1, j)
            break
    assert len(out) == 3
    return out
