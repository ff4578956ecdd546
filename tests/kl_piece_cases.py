"""Cases for the dense KL solvers at every instantiation and piece edge (tests/test_gpu_kl_pieces.py) and the conditions on them
(tests/test_kl_piece_cases_host.py): numpy only, importable without a GPU, deterministic, no plan calls at import.

kl_tile_kernel<EPT4, C, METHOD, ONEBUF> (fp32-operand mode) and kl_reg64_kernel<EPT2, C, METHOD> (strict mode) of nnlm_amd/csrc/k_kl.h keep
a column's state in registers as 16-byte slots (4 floats / 2 doubles): thread t of 512 owns slots t, t + 512, ... -- a PIECE is 512 slots
(2048 / 1024 elements), a WAVEFRONT PIECE 64 slots (256 / 128 elements).  The dispatch of launch_kl_tile() / launch_kl64() is restated here
(tile_plan, reg64_plan) so that a case can say which instantiation it reaches; the host test pins the restatement to nnlm_kl_plan, the GPU
test to what ran ("kl_form_*", "kl_pieces_*", "kl_cols_*" of nnlm_get_info).

A case is ONE half-step on ncols = 2 C + 1 columns (two full blocks and a ragged one) at rank 3 in the "contraction-major" form the oracle
takes: Ac p x ncols, the fixed factor Y 3 x p, the solved factor X0 3 x ncols, its mask or None --
ref.update(X0, Y, Ac, mask, REG, INNER, TOL, method).  Orientation "H" hands the GPU A = Ac (half_step(1) contracts over rows), "W" hands
it A = Ac^T (half_step(0) contracts over columns, through the transposed copy AT and What^T, whose leading dimension pads to 128 elements
where a tile row pads to 256: the upper half of one wavefront piece is then zero-filled and never loaded).

The rows of Ac and the columns of Y at the case's EDGE indices (edge_indices) are scaled by max(1, p / EDGE_DIV): each carries a few per
cent of every column's mass, so that one dropped or doubled boundary element moves every column far beyond the fp32 bar
(test_kl_piece_cases_host.py measures by how much)."""
import functools

import numpy as np

K = 3
REG = [0.01, 0.0, 0.02]
INNER, TOL = 3, 1e-9  # the recipe of test_kl_contraction_longer_than_32768
EDGE_DIV = 100.0      # an edge row weighs p / EDGE_DIV ordinary rows
EDGE_RATIO = 4.0      # and its data are 2 .. 4 times what the other rows' are: losing it moves every coordinate the same way

TILE2, TILE1, REG64, STREAM = 0, 1, 2, 3  # "kernel" of nnlm_kl_plan
TILE_PIECE, TILE_WPIECE, TILE_V = 2048, 256, 4
R64_PIECE, R64_WPIECE, R64_V = 1024, 128, 2
TILE_MAX_P = 40192  # the longest contraction kl_tile_kernel takes at rank 3, with or without a mask word (LDS: one row buffer of
                    # 10048 slots + 2224 .. 2232 bytes <= 160 KiB); the host test checks it against nnlm_kl_plan
TILE2_MAX_P = 20224  # the longest contraction its two-buffer forms take (2 x 5056 slots + 368 .. 384 bytes): 20225 .. 20480 are 10 pieces
                     # that fit neither two buffers nor the one-buffer forms' dispatch (11 .. 20 pieces) and go to kl_stream_kernel
R64_MAX_P = 20480   # 20 pieces of kl_reg64_kernel
R64_RUNGS = (1, 2, 3, 5, 7, 10, 12, 14, 16, 18, 20)
W_TILE_E = (1, 2, 3, 5, 6, 10, 11, 15, 20)  # W orientation: every C, both buffer counts, both ends of each
OWN_INIT_E = tuple(range(4, 11))            # two-buffer forms not yet run on their own starting states


# ---- the dispatch, restated ---------------------------------------------------------------------------------------------------------------
def tile_pieces(p):
    p4 = ((p + 3) // 4 + 63) // 64 * 64
    return (p4 + 511) // 512


def tile_plan(p):
    """(kernel, instantiated pieces, columns per block) of an fp32-operand half-step with contraction p at rank 3."""
    e = tile_pieces(p)
    if p > TILE_MAX_P or (e <= 10 and p > TILE2_MAX_P):
        return (STREAM, 0, 0)
    return (TILE2 if e <= 10 else TILE1, e, 8 if e <= 2 else 4 if e <= 5 else 2 if e <= 10 else 1)


def reg64_pieces(p):
    return ((p + 1) // 2 + 511) // 512


def reg64_plan(p):
    """The same in strict mode: exact piece counts round up to the next instantiated one."""
    if p > R64_MAX_P:
        return (STREAM, 0, 0)
    inst = next(r for r in R64_RUNGS if reg64_pieces(p) <= r)
    return (REG64, inst, 4 if inst <= 5 else 2 if inst <= 10 else 1)


def plan_of(kind, p):
    return tile_plan(p) if kind == "tile" else reg64_plan(p)


# ---- the lengths ---------------------------------------------------------------------------------------------------------------------------
def _j(e):
    return 1 + (5 * e) % 7  # 1 .. 7 wavefront-piece steps into the last piece, varying with e


def tile_lengths(e):
    """(p_lo, p_mid, p_hi) of tile piece count e: wavefront 0 alone owns the last piece and p mod 4 = 1 / some wavefronts own it and the
    last float4 is ragged / all eight own it and it is full (e = 10, e = 20: the longest contraction the two- / one-buffer forms take)."""
    base = TILE_PIECE * (e - 1)
    return (base + 1, base + TILE_WPIECE * _j(e) + 2 + e % 2, {10: TILE2_MAX_P, 20: TILE_MAX_P}.get(e, TILE_PIECE * e))


def reg64_lengths(e):
    """(p_lo, p_mid, p_hi) of exact reg64 piece count e: odd / a wavefront-piece step plus an odd remainder / full."""
    base = R64_PIECE * (e - 1)
    return (base + 1, base + R64_WPIECE * _j(e) + 1 + 2 * (e % 2), R64_PIECE * e)


def tile_w_lengths(e):
    """W orientation, 256 t + 127 and 256 t + 129 in piece e: the row ends in the lower half of a wavefront piece whose upper half lies
    beyond the 128-element leading dimension (zero-filled, never loaded) / just past it (the whole wavefront piece is loaded)."""
    t0 = TILE_PIECE * (e - 1) + TILE_WPIECE * ((5 * e) % 7 if e < 20 else 2)
    return (t0 + 127, t0 + 129)


def edge_indices(kind, p, orient):
    """Contraction indices at which the kernels branch: both ends, the ragged last slot, the first element of the last piece and of the
    last wavefront piece that exists and the element in front of each, the last element in front of the leading-dimension cut."""
    piece, wpiece, v = (TILE_PIECE, TILE_WPIECE, TILE_V) if kind == "tile" else (R64_PIECE, R64_WPIECE, R64_V)
    fp = (p - 1) // piece * piece
    fw = (p - 1) // wpiece * wpiece
    idx = [0, p - 1, p - 2, p - 3, fp, fp - 1, fw, fw - 1]
    if kind == "tile" and orient == "W":
        cut = (p + 127) // 128 * 128  # elements of a row of AT / What^T; a tile row pads to 256
        if cut % 256:
            idx.append(cut - 1)
    return sorted({i for i in idx if 0 <= i < p})


def probe_indices(c):
    """The edge indices the sensitivity test zeroes: p - 1, the first element of the last existing wavefront piece, the element in front of
    the last piece (row 0 where there is none)."""
    p = c["p"]
    wpiece, piece = (TILE_WPIECE, TILE_PIECE) if c["kind"] == "tile" else (R64_WPIECE, R64_PIECE)
    fp = (p - 1) // piece * piece
    return sorted({p - 1, (p - 1) // wpiece * wpiece, fp - 1 if fp > 0 else 0})


# ---- the table -----------------------------------------------------------------------------------------------------------------------------
def _case(kind, orient, p, method, tag, serial):
    plan = plan_of(kind, p)
    return dict(kind=kind, orient=orient, p=p, method=method, tag=tag, plan=plan, ncols=2 * plan[2] + 1 if plan[2] else 3,
                pieces_exact=0 if plan[0] == STREAM else (tile_pieces(p) if kind == "tile" else reg64_pieces(p)),
                nan_edge=bool(serial & 1), masked=bool(serial & 2),
                id="%s-%s-p%d-m%d-%s" % (kind, orient, p, method, tag))


def _build():
    h, w = [], []
    for kind, lengths, beyond in (("tile", tile_lengths, (TILE2_MAX_P + 1, 20480, TILE_MAX_P + 1)), ("reg64", reg64_lengths, (R64_MAX_P + 1,))):
        for e in range(1, 21):
            lo, mid, hi = lengths(e)
            for p, tag, methods in ((lo, "lo", (3, 4)), (mid, "mid", (3 + e % 2,)), (hi, "hi", (3, 4))):
                for method in methods:
                    h.append(_case(kind, "H", p, method, tag, len(h)))
        for i, p in enumerate(beyond):  # the first length past each switch point streams
            for method in ((3, 4) if p == beyond[-1] else (3 + i % 2,)):
                h.append(_case(kind, "H", p, method, "stream", len(h)))
    for e in W_TILE_E:
        for p, tag in zip(tile_w_lengths(e), ("cut-in", "cut-out")):
            w.append(_case("tile", "W", p, 3 + (e + (tag == "cut-out")) % 2, tag, len(w) + 1))
    for i, e in enumerate(R64_RUNGS):
        w.append(_case("reg64", "W", reg64_lengths(e)[1], 3 + i % 2, "mid", len(w) + 1))
    return tuple(h), tuple(w)


H_CASES, W_CASES = _build()
CASES = H_CASES + W_CASES
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)
# the two-buffer tile kernel on its own starting states (no room for the matrix-sized buffer): p_mid of 4 .. 10 pieces, both methods
OWN_INIT_CASES = tuple(dict(BY_ID["tile-H-p%d-m%d-mid" % (tile_lengths(e)[1], 3 + e % 2)], method=m,
                            id="tile-H-p%d-m%d-own" % (tile_lengths(e)[1], m)) for e in OWN_INIT_E for m in (3, 4))
BY_ID.update({c["id"]: c for c in OWN_INIT_CASES})


# ---- the data ------------------------------------------------------------------------------------------------------------------------------
def make_data(c, weight=None):
    """dict(Ac p x ncols, Y 3 x p, X0 3 x ncols, mask 3 x ncols bool or None, edges): uniform random, about 2 % of Ac missing, the edge rows
    weighted (and never missing by chance).  nan_edge: column j misses one weighted edge entry, on an edge the sensitivity test does not
    probe.  masked: about 30 % of X0's coordinates are masked and column 1 entirely.  Depends on (kind, orient, p, flags) only, not on the
    method, so that cases differing in the method alone share their data."""
    p, ncols = c["p"], c["ncols"]
    rng = np.random.default_rng([7, int(c["kind"] == "tile"), int(c["orient"] == "H"), p, int(c["nan_edge"]), int(c["masked"])])
    Ac = rng.random((p, ncols))
    Y = rng.random((K, p))
    X0 = rng.random((K, ncols))
    holes = rng.random((p, ncols)) < 0.02
    edges = edge_indices(c["kind"], p, c["orient"])
    holes[edges, :] = False
    Ac[holes] = np.nan
    wt = max(1.0, p / EDGE_DIV) if weight is None else weight
    Ac[edges, :] = (0.5 + 0.5 * Ac[edges, :]) * (EDGE_RATIO * wt)
    Y[:, edges] = (0.5 + 0.5 * Y[:, edges]) * wt
    if c["nan_edge"]:
        spare = [i for i in edges if i not in probe_indices(c)]
        for j in range(ncols if spare else 0):
            Ac[spare[j % len(spare)], j] = np.nan
    mask = None
    if c["masked"]:
        mask = rng.random((K, ncols)) < 0.3
        mask[:, 1] = True
        X0 = np.where(mask, 0.2 * X0, X0)  # (given values small enough that a column's free coordinates are not clamped to zero)
    return dict(Ac=Ac, Y=Y, X0=X0, mask=mask, edges=edges)


@functools.lru_cache(maxsize=None)
def oracle(ref, case_id):
    """(X 3 x ncols, sweeps) of the oracle's half-step on the case (computed once per case, shared, never written to)."""
    c = BY_ID[case_id]
    d = make_data(c)
    X, it = ref.update(d["X0"], d["Y"], d["Ac"], d["mask"], REG, INNER, TOL, c["method"])
    X.setflags(write=False)
    return X, int(it)


def col_err(X, Xref):
    """Relative error of every column (a column the reference leaves at exactly zero: 0 if equal, else inf)."""
    num, den = np.linalg.norm(X - Xref, axis=0), np.linalg.norm(Xref, axis=0)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num > 0, np.inf, 0.0))
