"""Cases for the error block (tests/test_gpu_error_block.py) and the conditions on them (tests/test_err_cases_host.py): numpy only,
importable without a GPU, deterministic in (family, n, m, k, missing).

The error block evaluates, for the current factors, the sum of (a - wh)^2 and of -(a + 1e-16) log(wh + 1e-16) + wh over the finite
entries of A (mse_error, the variable part of mkl_error; src/nnmf.cpp:121-126,135-140) and the six sums add_penalty() needs.  Five
kernel families do it (nnlm_amd/csrc):
  errors64_kernel<HAS_MISS>            k_errors.h    strict fp64, k <= 64: 64 x 64 tiles, a block walks a chunk of j-tiles     2
  errors_f32_kernel<HAS_MISS>          k_errors.h    fp32 operands, k <= 64: one 128 x 128 tile per block                      2
  errors_kernel<double | float>        k_errors.h    k > 64, both modes: 64 x 64 tiles, no LDS                                  2
  xprod16_err_kernel<NKQ, HAS_MISS>    k_xprod16.h   fp32 operands, k <= 64, inside the speculative W half-step of a trace
                                                     iteration of nnlm_run: 128 rows x stages of 64 columns                     8
  penalty_kernel                       k_errors.h    fp64 in both modes
errors_launch() (nnlm_mi355x.hip) picks the kernel from the mode, the rank, whether A has missing entries and -- in nnlm_run -- whether a
W half-step follows.  The rule is restated here (kernel_of, tiles, strict_chunks, shard) so that a test can say what a case reaches.

Families (make_case): "ones" and "planted" have integer factors in {1, 2, 3} and A = W H + 1, respectively A = W H except at up to 11
entries on the tile edges of all kernels where A = W H + 2^t, t = 0 .. 10.  Every number any kernel forms from them -- the fp32 copy of
A, its split-fp16 copy (22 bits), the products, the fp32 and fp64 partial sums -- is an integer below 2^24, so the sum of squares is
EXACTLY the number of finite entries, respectively the sum of 4^t over the planted entries that are finite (< 2^22): an entry dropped,
counted twice or counted although missing (A holds 0 there in the device copies, wh^2 >= 1) moves mse by at least 1 / N.  "uniform",
"zero_lines" (wh = 0 under a > 0 and under a = 0, in an interior and in the ragged last 64-row tile) and "scaled_up" / "scaled_down"
(the power-of-two exponents of the split copies) round, and are held to the reference err_ref() -- long double terms, long double sums."""
import collections
import functools

import numpy as np

TINY = 1e-16
PAD_N, PAD_M = 256, 128      # NNLM_PAD_N, NNLM_PAD_M (common.h): npad, mpad
KQ_MAX = 64                  # NNLM_KQ_MAX: the generic kernels take over beyond

MAIN = (150, 160)
SHAPES_OTHER = ((1, 1), (63, 65), (64, 64), (128, 128), (129, 127), (257, 70), (1153, 130))
SHAPES_SMALL = (MAIN,) + SHAPES_OTHER
LARGE, LARGE_K = (4100, 4101), 3
RANKS_ALL = tuple(range(1, 65))
RANKS_FEW = (1, 2, 3, 16, 17, 49, 50, 51, 63, 64)   # both ends of every NKQ, both parities of k2 = k rounded up to 2, k4 to 4
RANKS_ENDS = (1, 17, 64)
RANKS_GENERIC = (65, 70)

FAMILIES = ("ones", "planted", "uniform", "zero_lines", "scaled_up", "scaled_down")
EXACT = ("ones", "planted")
ROUNDING = FAMILIES[2:]
# missing variants: 10 % NaN; column 4 and row 7 wholly NaN; NaN on both sides of a mask word, in both directions, and in the last
# corner; (planted) one NaN directly beside every planted entry
MISSING = (None, "nan10", "lines", "word", "beside")
WORD_SIDES = ((31, 31), (31, 32), (32, 31))
EDGE_ROWS = (0, 15, 16, 31, 32, 63, 64, 127, 128)        # + n - 1
EDGE_COLS = (0, 15, 16, 31, 32, 47, 48, 63, 64, 127, 128)  # + m - 1

Case = collections.namedtuple("Case", "family n m k missing")


def missing_applies(n, m, missing, family="ones"):
    """A variant needs the entries it names, has to leave finite entries and has to make at least one entry missing."""
    if missing is None:
        return True
    if missing == "beside":
        return family == "planted" and n * m >= 2
    if missing == "nan10":
        return n * m >= 40
    if missing == "lines":
        return n > 8 and m > 5
    return n > 32 and m > 32   # "word"


def planted_entries(n, m, k):
    """[(i, j, t)]: entry (i, j) of A is W H + 2^t; rows and columns from the tile edges of all kernels, turned by the rank so that the
    ranks of a shape reach every pair of lists."""
    rows = sorted({r for r in EDGE_ROWS + (n - 1,) if r < n})
    cols = sorted({c for c in EDGE_COLS + (m - 1,) if c < m})
    out, seen = [], set()
    for t in range(11):
        ij = (rows[(t + k) % len(rows)], cols[(t + 3 * k) % len(cols)])
        if ij not in seen:
            seen.add(ij)
            out.append(ij + (t,))
    return out


def _beside(n, m, i, j, taken):
    for ij in ((i, j + 1), (i, j - 1), (i + 1, j), (i - 1, j)):
        if 0 <= ij[0] < n and 0 <= ij[1] < m and ij not in taken:
            return ij
    return None


def zero_lines_of(n, m):
    """(zero rows of W, zero column of H): row 5 lies in the first 64-row tile (interior when n >= 64), row n - 1 in the last (ragged
    unless 64 divides n)."""
    return sorted({min(5, n - 1), n - 1}), m // 2


def make_case(family, n, m, k, missing=None):
    """dict(A, W, H, exact, planted): exact = the sum of squares as an int for the exact families, None otherwise."""
    assert missing_applies(n, m, missing, family), (family, n, m, missing)
    rng = np.random.default_rng([FAMILIES.index(family), n, m, k, MISSING.index(missing)])
    planted = []
    if family in EXACT:
        W = rng.integers(1, 4, (n, k)).astype(np.float64)
        H = rng.integers(1, 4, (k, m)).astype(np.float64)
        A = W @ H
        if family == "ones":
            A += 1.0
        else:
            planted = planted_entries(n, m, k)
            for i, j, t in planted:
                A[i, j] += 2.0 ** t
    else:
        A, W, H = rng.random((n, m)), rng.random((n, k)), rng.random((k, m))
        if family == "zero_lines":
            rows, col = zero_lines_of(n, m)
            W[rows, :] = 0.0
            H[:, col] = 0.0
            A[rng.random((n, m)) < 0.3] = 0.0
        elif family == "scaled_up":
            A *= 2.0 ** 20
            W *= 2.0 ** 10
        elif family == "scaled_down":
            A *= 2.0 ** -20
            W *= 2.0 ** -10
    if missing == "nan10":
        A[rng.random((n, m)) < 0.1] = np.nan
        if not np.isfinite(A).any():
            A[0, 0] = (W @ H)[0, 0] + 1.0
    elif missing == "lines":
        A[:, 4] = np.nan
        A[7, :] = np.nan
    elif missing == "word":
        for i, j in WORD_SIDES + ((n - 1, m - 1),):
            A[i, j] = np.nan
    elif missing == "beside":
        taken = {(i, j) for i, j, _ in planted}
        for i, j, _ in planted:
            ij = _beside(n, m, i, j, taken)
            if ij is not None:
                taken.add(ij)
                A[ij] = np.nan
    fin = np.isfinite(A)
    assert fin.any() and (missing is None) == bool(fin.all())
    exact = None
    if family == "ones":
        exact = int(fin.sum())
    elif family == "planted":
        exact = sum(4 ** t for i, j, t in planted if fin[i, j])
    return dict(A=A, W=W, H=H, exact=exact, planted=planted)


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
Ref = collections.namedtuple("Ref", "s2 kl abs2 abskl N kl_const abs_const pen")
LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "err_ref() needs a long double wider than a double"


def _ldsum(x):
    """Long double sum; of an fp64 array (the large shape only): fp64 pairwise inside chunks of 4096, long double across them."""
    if x.dtype == LD or x.size < 8192:
        return x.sum(dtype=LD)
    x = x.ravel()
    cut = x.size - x.size % 4096
    return x[:cut].reshape(-1, 4096).sum(axis=1).sum(dtype=LD) + x[cut:].sum(dtype=LD)


def err_ref(A, W, H):
    """Ref(sum of squares, variable KL part, the sums of |term| of both, N, kl_const, its mean |term|, the six penalty sums) over the
    finite entries of A.  Up to 2^20 entries every term and every sum is formed in long double (64-bit significand), W H included unless
    the factors are integers (then the fp64 product is exact); beyond (the one large shape, rank 3) the terms are fp64 -- each within
    3e-16 of itself -- and only the sums across chunks of 4096 long double: five orders below the tightest bar on that shape.
    pen = (sum w^2, sum_i (sum_q w_iq)^2, sum w, the same three of H): src/nnmf.cpp:224-240."""
    fin = np.isfinite(A)
    T = LD if A.size <= 2 ** 20 else np.float64
    Wl, Hl = W.astype(LD), H.astype(LD)
    if T is not LD or (np.array_equal(W, np.rint(W)) and np.array_equal(H, np.rint(H))):
        wh = (W @ H).astype(T)
    else:
        wh = np.einsum("iq,qj->ij", Wl, Hl)
    a, wh = (A.ravel().astype(T), wh.ravel()) if fin.all() else (A[fin].astype(T), wh[fin])
    d = a - wh
    t2 = d * d
    tiny = T(TINY)
    tk = -(a + tiny) * np.log(wh + tiny) + wh
    tc = (a + tiny) * np.log(a + tiny) - a
    N = int(fin.sum())
    pen = []
    for X, axis in ((Wl, 1), (Hl, 0)):
        pen += [_ldsum(X * X), _ldsum(X.sum(axis=axis, dtype=LD) ** 2), _ldsum(X)]
    return Ref(_ldsum(t2), _ldsum(tk), _ldsum(np.abs(t2)), _ldsum(np.abs(tk)), N, _ldsum(tc) / N, _ldsum(np.abs(tc)) / N, tuple(pen))


_REFS = {}


def ref_of(case, c=None):
    """err_ref of a Case (scalars only are kept: the GPU tests of both modes and the host test share one evaluation); c = make_case(*case)
    if the caller has it."""
    if case not in _REFS:
        c = c or make_case(*case)
        _REFS[case] = err_ref(c["A"], c["W"], c["H"])
    return _REFS[case]


def dev(got, want, abs_sum, N):
    """|got - want| / (sum |term| / N) for a mean `got` and the reference's sum `want`: the bars are on this number."""
    scale = float(abs_sum) / N
    return abs(float(LD(got) - want / N)) / scale if scale > 0 else abs(float(got))


def fp32_emulation_s2(A, W, H):
    """The sum of squares as an fp32-operand kernel forms it: fp32 A and factors, fp32 products and sums over the rank, fp32 squares and
    an fp32 sum (shapes below 2^24 entries; the kernels fold into fp64 per tile or stage)."""
    fin = np.isfinite(A)
    A32 = np.where(fin, A, 0.0).astype(np.float32)
    W32, H32 = W.astype(np.float32), H.astype(np.float32)
    wh = np.zeros(A.shape, dtype=np.float32)
    for q in range(W.shape[1]):
        wh += W32[:, q:q + 1] * H32[q:q + 1, :]
    d = A32 - wh
    t2 = np.where(fin, d * d, np.float32(0))
    s = np.float32(0)
    for col in t2.T:           # (sequential over the columns, pairwise inside: every partial sum is an integer below 2^24)
        s = np.float32(s + col.sum(dtype=np.float32))
    return float(s)


# ---- the launch rule, restated ----------------------------------------------------------------------------------------------------------
def pads(n, m):
    return -(-n // PAD_N) * PAD_N, -(-m // PAD_M) * PAD_M


def kernel_of(mode, k, any_missing, sharded=False, fused=False):
    """The kernel that forms the two sums.  fused: the trace entry of an nnlm_run iteration that a W half-step follows (fp32-operand mode,
    square loss, k <= 64; across ranks only without missing entries); otherwise errors() and a run's last entry."""
    miss = "true" if any_missing else "false"
    if k > KQ_MAX:
        return "errors_kernel<double>" if mode == "f64" else "errors_kernel<float>"
    if mode == "f64":
        return f"errors64_kernel<{miss}>"
    if fused and not (sharded and any_missing):
        return f"xprod16_err_kernel<{(k + 15) // 16}, {miss}>"
    return f"errors_f32_kernel<{miss}>"


def tile_of(kernel):
    """(rows, columns) of the unit whose interior / edge form is block (or stage) uniform."""
    if kernel.startswith("errors_f32"):
        return 128, 128
    if kernel.startswith("xprod16_err"):
        return 128, 64
    return 64, 64


def tiles(kernel, n, m):
    """Which kinds of tile with entries a case has: {"interior", "row_edge", "col_edge"} (a corner tile counts as both edges)."""
    tr, tc = tile_of(kernel)
    kinds = set()
    for i0 in range(0, n, tr):
        for j0 in range(0, m, tc):
            re, ce = i0 + tr > n, j0 + tc > m
            if re:
                kinds.add("row_edge")
            if ce:
                kinds.add("col_edge")
            if not re and not ce:
                kinds.add("interior")
    return kinds


def shard(tile_cols, m, rank=0, nranks=1):
    """(first j-tile, j-tiles) of a rank's share of the error block (errors_launch: whole tiles of the mode's width)."""
    tj = pads(1, m)[1] // tile_cols
    if nranks == 1:
        return 0, tj
    per = -(-tj // nranks)
    jt0 = min(rank * per, tj)
    return jt0, min(jt0 + per, tj) - jt0


Chunks = collections.namedtuple("Chunks", "nit jt0 jcnt nchunks chunk last")


def strict_chunks(n, m, rank=0, nranks=1):
    """errors64_kernel's grid: nit i-tiles x nchunks chunks of `chunk` j-tiles (the last holds `last`); about eight rounds of the 512
    resident blocks."""
    nit = pads(n, m)[0] // 64
    jt0, jcnt = shard(64, m, rank, nranks)
    if jcnt <= 0:
        return Chunks(nit, jt0, 0, 0, 0, 0)
    nchunks = min(max((8 * 512 + nit // 2) // nit, 1), jcnt)
    chunk = -(-jcnt // nchunks)
    nchunks = -(-jcnt // chunk)
    return Chunks(nit, jt0, jcnt, nchunks, chunk, jcnt - (nchunks - 1) * chunk)


def f32_grid(n, m, rank=0, nranks=1):
    """(blocks launched, blocks with a tile) of errors_f32_kernel: 8 * ceil(nx / 8) block ids per j-tile, XCD-aware numbering."""
    nx = pads(n, m)[0] // 128
    _, jcnt = shard(128, m, rank, nranks)
    return 8 * (-(-nx // 8)) * jcnt, nx * jcnt


# ---- the case lists ---------------------------------------------------------------------------------------------------------------------
def _rot(k, family):
    """The missing variant of rank k in a full rank range: all of them in turn."""
    return ("nan10", "lines", "word")[k % 3] if family != "planted" else ("beside", "nan10", "lines", "word")[k % 4]


def _add(out, family, n, m, k, missing):
    if missing_applies(n, m, missing, family):
        out.append(Case(family, n, m, k, missing))


@functools.lru_cache(maxsize=None)
def plain_cases(shape, k):
    """The cases of (shape, k) for errors(): ranks 1 .. 64 + 65, 70 at MAIN, RANKS_FEW elsewhere, LARGE_K at LARGE.  The exact families
    and "uniform" without and with missing entries at every rank (all variants in turn over a full range, all at once at RANKS_FEW);
    "zero_lines" and the two "scaled" at the rank ends."""
    n, m = shape
    out = []
    few = k in RANKS_FEW or k in RANKS_GENERIC
    if shape == LARGE:   # (what only a large shape shows: chunks of two j-tiles, idle blocks, reductions over thousands of blocks)
        return (Case("ones", n, m, k, None), Case("ones", n, m, k, "nan10"), Case("uniform", n, m, k, None))
    for family in ("ones", "planted", "uniform"):
        _add(out, family, n, m, k, None)
        variants = MISSING[1:] if (few and shape == MAIN and family != "uniform") else (_rot(k, family),)
        for missing in variants:
            _add(out, family, n, m, k, missing)
    ends = RANKS_FEW + RANKS_GENERIC[:1] if shape == MAIN else RANKS_ENDS
    if k in ends:
        for family in ROUNDING[1:]:
            _add(out, family, n, m, k, None)
            _add(out, family, n, m, k, "nan10")
    return tuple(out)


def plain_groups():
    """[(shape, k)] of the plain-kernel test."""
    g = [(MAIN, k) for k in RANKS_ALL + RANKS_GENERIC]
    g += [(s, k) for s in SHAPES_OTHER for k in RANKS_FEW]
    return g + [(LARGE, LARGE_K)]


@functools.lru_cache(maxsize=None)
def fused_cases(shape, k):
    """The cases of (shape, k) for the frozen-factor runs: [(Case, methods)].  Fused entries exist at k <= 64 only."""
    out = []
    for c in plain_cases(shape, k):
        if c.k > KQ_MAX:
            continue
        both = c.family == "ones" or k in RANKS_ENDS
        out.append((c, (1, 2) if both else ((1,) if k % 2 else (2,))))
    return tuple(out)


def fused_groups():
    return [(MAIN, k) for k in RANKS_ALL] + [(s, k) for s in SHAPES_OTHER for k in RANKS_FEW]


def all_cases():
    seen = collections.OrderedDict()
    for shape, k in plain_groups():
        for c in plain_cases(shape, k):
            seen[c] = None
    return list(seen)
