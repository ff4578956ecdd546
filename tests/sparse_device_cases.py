"""Cases for the ingest of sparse matrices that live in device memory (nnlm_set_matrix_sparse_device, k_sparse_ingest.h): cases only, no
tests.  Every case is a canonical CSC (indptr int64, indices int32, data fp64, (n, m)) built from numpy alone; values are multiples of
1 / 64 below 4 -- exact in fp64, fp32, fp16 and bf16 -- and zero is among them, so the missing doors see explicit stored zeros.

The shapes are the smallest at which a stage of the ingest can go wrong.  `share` and `tile` are the entries per workgroup of the entry
check and of a radix pass: the callers read them from the library (nnlm_get_info "sp_ingest_check_share" / "sp_ingest_sort_tile") or from
the kernel header's defines, never from a copy here.  Cases are built on demand (build(name, share, tile)): the widest one carries a
pointer array of 2^24 + 2 entries."""
import os
import re

import numpy as np

from sparse_cases import _empty_lines, _heavy, _powerlaw, csc_from_flat, csc_from_pattern

DOORS = {  # name -> (absent, kl, batch), the host entry of Handle
    "plain": ("zero", False, False), "batch": ("zero", False, True), "kl": ("zero", True, False), "kl_batch": ("zero", True, True),
    "missing": ("missing", False, False), "missing_batch": ("missing", False, True),
}
HOST_ENTRY = {"plain": "set_matrix_csc", "batch": "set_matrix_csc_batch", "kl": "set_matrix_csc_kl", "kl_batch": "set_matrix_csc_kl_batch",
              "missing": "set_matrix_csc_missing", "missing_batch": "set_matrix_csc_missing_batch"}
INT_DTYPES = ("int32", "int64")
VAL_DTYPES = ("float64", "float32", "float16", "bfloat16")
LAYOUTS = ("csc", "csr")


def header_constants():
    """(share, tile) from the defines of k_sparse_ingest.h (what nnlm_get_info answers on a device)."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "nnlm_amd", "csrc", "k_sparse_ingest.h")
    src = open(path).read()
    env = {}
    for name, expr in re.findall(r"^#define (SPI_[A-Z_]+) ([^/\n]+)", src, flags=re.M):
        expr = expr.strip()
        if re.fullmatch(r"[\dA-Z_ ()*+]+", expr) and all(w in env for w in re.findall(r"[A-Z_]+", expr)):
            env[name] = int(eval(expr, {}, env))  # (integer products of earlier defines)
    return env["SPI_CHECK_SHARE"], env["SPI_SORT_TILE"]


def exact_values(size, rng):
    return rng.integers(0, 256, size=size).astype(np.float64) / 64.0


def from_coords(rows, cols, n, m, rng):
    """Canonical CSC of the distinct (row, column) pairs."""
    flat = np.unique(np.asarray(cols, dtype=np.int64) * n + np.asarray(rows, dtype=np.int64))
    return csc_from_flat(flat, exact_values(flat.size, rng), n, m)


def random_nnz(n, m, nnz, rng):
    flat = np.sort(rng.choice(n * m, size=nnz, replace=False))
    return csc_from_flat(flat, exact_values(nnz, rng), n, m)


def scattered(n, m, count, rng):
    """About `count` entries anywhere in an n x m matrix that may be far too large to enumerate."""
    return from_coords(rng.integers(0, n, size=count), rng.integers(0, m, size=count), n, m, rng)


def transposed(S):
    """The CSC of the transposed matrix (stable argsort: the columns of a row come out ascending)."""
    indptr, idx, val, (n, m) = S
    cols = np.repeat(np.arange(m, dtype=np.int64), np.diff(indptr))
    order = np.argsort(idx, kind="stable")
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(idx, minlength=n), out=ptr[1:])
    return ptr, cols[order].astype(np.int32), val[order], (m, n)


def other_side(S):
    """(rowptr, colidx, rowval) of the CSC S: what the host's counting sort and the device's radix sort must both leave."""
    ptr, cidx, rval, _ = transposed(S)
    return ptr, cidx, rval


def _pattern(P, rng):
    return csc_from_pattern(P, exact_values(P.shape, rng).reshape(P.shape))


def _builders(share, tile):
    b = {}
    counts = sorted({0, 1, 63, 64, 65, share - 1, share, share + 1, tile - 1, tile, tile + 1, 2 * share + 1, 2 * tile + 1})
    for c in counts:  # stored entries around a wavefront, a check block's share and a sort block's tile
        b["nnz_%d" % c] = (lambda c=c: lambda rng: random_nnz(97, 61, c, rng))()
    # radix passes: ceil(log2(lines of the built side) / 8): 1 -> none, 256 -> one, 257 -> two, 65536 -> two, 65537 -> three
    for L in (1, 255, 256, 257, 65535, 65536, 65537):
        w = 7 if L == 1 else 29
        cnt = 7 if L == 1 else 3000
        b["lines_%d" % L] = (lambda L=L, w=w, cnt=cnt: lambda rng: scattered(L, w, cnt, rng) if L > 1 else random_nnz(1, w, cnt, rng))()
    b["lines_16777217"] = lambda rng: scattered((1 << 24) + 1, 3, 300, rng)  # the fourth pass; pointer-array memory only
    # heavy duplication of one key
    b["one_row"] = lambda rng: random_nnz(1, 300, 300, rng)
    b["one_col"] = lambda rng: random_nnz(300, 1, 300, rng)

    def full_column(rng):
        P = np.zeros((3000, 5), dtype=bool)
        P[:, 2] = True
        return _pattern(P, rng)

    def row_everywhere(rng):
        P = rng.random((50, 3000)) < 0.01
        P[17, :] = True
        return _pattern(P, rng)

    def dominant_line(rng):
        P = rng.random((4000, 40)) < 0.006
        P[:3000, 7] = True
        return _pattern(P, rng)

    b["full_column"] = full_column
    b["row_everywhere"] = row_everywhere
    b["dominant_line"] = dominant_line
    b["empty_lines"] = lambda rng: _pattern(_empty_lines(80, 60, rng), rng)
    b["powerlaw"] = lambda rng: _pattern(_powerlaw(120, 90, rng, False), rng)
    b["small"] = lambda rng: _pattern(rng.random((37, 29)) < 0.3, rng)
    # fits: long and short lines on both sides (a full row and a full column over a thin background)
    b["fit_heavy"] = lambda rng: _pattern(_heavy(300, 280, rng), rng)
    b["fit_heavy_long"] = lambda rng: _pattern(_heavy(2100, 2060, rng), rng)
    return b


def case_names(share, tile):
    return list(_builders(share, tile))


def build(name, share, tile):
    """The CSC of a case (deterministic: the generator is seeded from the name)."""
    rng = np.random.default_rng([ord(ch) for ch in name])
    return _builders(share, tile)[name](rng)


# which layouts a case is ingested in: the wide pass-edge cases once per layout (as CSC the built side has `lines` rows; as CSR the
# transposed matrix is given, so the built side is again the long one)
def big(name):
    return name.startswith("lines_") and int(name.split("_")[1]) >= 65535
