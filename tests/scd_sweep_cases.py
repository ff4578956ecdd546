"""Cases for every instantiation of the dense square-loss SCD sweep (tests/test_gpu_scd_forms.py) and the conditions on them
(tests/test_scd_sweep_cases_host.py): numpy only, importable without a GPU, deterministic in (k, variant).

Four kernel families solve the dense SCD half-step at ranks up to 64 (nnlm_amd/csrc):
  "q"   sweep_scd_q_kernel<NT, NB, HAS_MASK, true>    k_sweep_q.h / tu_sweepq.hip    strict fp64, plain form          16 NB x mask     = 32
  "qw"  sweep_scd_qw_kernel<NT, NB, HAS_MASK, true>   k_sweep_q.h / tu_sweepqw.hip   strict fp64, persistent form     16 NB x mask     = 32
  "f"   sweep_scd_f_kernel<NT, NB, HAS_MASK, NW>      k_sweep_f.h / tu_sweepf.hip    fp32 operands, matrix pipe       16 NB x mask x 2 = 64
  "r"   sweep_row_kernel<CPL, HAS_MASK, KR, NT, NW>   k_sweep_r.h / tu_sweepr.hip    fp32 operands, row form, k <= 50  4 CPL x mask x 2 = 16
launch_sweep_q() / launch_sweep_f() (nnlm_mi355x.hip) pick the family, the wavefronts per workgroup NW or the column groups per
workgroup G from the precision, the rank, the columns of the launch, the compute units the handle counts (nnlm_debug_set_cus) and the
inner iteration limit.  The rule is restated here (policy) so that a test can say which instantiation a case reaches;
test_gpu_scd_forms.py pins the restatement to what the library reports ("sweep_form_*", "sweep_groups_*", "cus" of nnlm_get_info).

A case is the W half-step of a 150 x 160 matrix, so the columns of the launch are the 150 rows of A: 150 = 9 * 16 + 6 = 2 * 64 + 22 =
4 * 32 + 22 is ragged for every workgroup shape, and a device "with" 1, 3, 5 or 10 compute units puts the same matrix through every
family.  The oracle sees it as ref.update(W0.T, H0, A.T, Wm.T, ...); the H half-step that follows on the same handle (160 columns, the
same family) is ref.update(H0, W.T, A, Hm, ...)."""
import collections
import functools

import numpy as np

N, M = 150, 160
KS = tuple(range(1, 65))
REG = (0.02, 0.01, 0.03)   # all three penalties: the r0 != r1 diagonal edit, the r1 off-diagonal edit, the r2 term of the gradient
NOREG = (0.0, 0.0, 0.0)    # the `r2 == 0` / `r1 == 0` branches
TIGHT = (30, 1e-9)         # (inner sweeps, inner tolerance): the main setting
# columns finish at different sweeps: TEST true / false steps, write_col on finishing, hand-over of finished columns.  At 1e-2 and below
# the oracle runs the whole budget on every column from k = 16 up; at 1e-1 it takes 12 % (k = 2) to 97 % (k = 56) of the budget
LOOSE = (30, 1e-1)
SETTINGS = (("tight", TIGHT), ("loose", LOOSE))

# both rank ends of every rank padding NT = 1 .. 4 and of the row form's last class (KR = 50 at k = 49, 50; 51 is the first rank beyond it)
NT_ENDS = (1, 16, 17, 32, 33, 48, 49, 50, 51, 64)
# variant -> (masked, penalties)
VARIANTS = collections.OrderedDict((("plain", (False, False)), ("masked", (True, True)), ("mask_nopen", (True, False)), ("pen_nomask", (False, True))))

SWEEPR_KMAX = 50           # tu_sweepq.h
WRAP_MAXG = 10             # SWEEPQ_WRAP_MAXG, k_sweep_q.h
LDS_LIMIT = 160 * 1024
FORM_CODE = {"q": 0, "qw": 1, "f": 2, "r": 3}   # "sweep_form_*" of nnlm_get_info

CUS_F64 = (1, 3)           # persistent with G = 5 (two workgroups); plain (three workgroups)
CUS_F32 = (1, 3, 5, 10)    # matrix pipe NW = 8, NW = 4; row form NW = 8, NW = 4 (k <= 50; above, 5 and 10 repeat the matrix pipe's NW = 4)

# the persistent form at every group count the policy can choose: (cus, columns) -> G, shapes of tests/test_gpu_wrap.py's parameter list
KS_FEW = (3, 22, 41, 60)   # NB = 1, 6, 11, 15
G_SHAPES = ((2, 150, 5), (3, 260, 6), (1, 112, 7), (1, 144, 9))
# inner limits below the persistent form's threshold of four: the plain form beyond one wavefront per SIMD (cus = 1: ten groups on four SIMDs)
INNER_LIMITS = (0, 1, 3)


# ---- the launch policy, restated ------------------------------------------------------------------------------------------------------------
Form = collections.namedtuple("Form", "family NB NT groups wgs")   # groups: NW (f, r), G (qw), 4 (q): "sweep_groups_*"


def sweepq_np(NB):
    """Operand pairs per step of the strict kernels (sweepq_np(NB, true))."""
    return (NB + 4) // 2


def sweepqw_lds_bytes(KP, NB, G):
    """LDS of one persistent workgroup in the strict mode (sweepqw_lds_bytes): x image of 16 G columns, operand image, three hand-over slots."""
    slot = (2 * NB + 1) * 64 + 64
    return (16 * G * (KP + 2) + NB * sweepq_np(NB) * 32 + 4 * NB + 3 * slot) * 8 + 64


def policy(prec, k, ncols, cus, inner):
    """Form of the launch that solves `ncols` columns at rank k <= 64 on a handle that counts `cus` compute units; prec "f64" / "f32"."""
    assert 1 <= k <= 64 and ncols > 0 and cus > 0
    NB, NT = (k + 3) // 4, (k + 15) // 16
    ngroups, simds = (ncols + 15) // 16, 4 * cus
    if prec == "f32":
        if k <= SWEEPR_KMAX and ncols <= 32 * cus:  # ONE round of the row form's wavefronts, at most two per SIMD
            NW = 4 if ncols <= 16 * cus else 8
            return Form("r", NB, NT, NW, (ncols + 4 * NW - 1) // (4 * NW))
        NW = 8 if ngroups > simds else 4
        return Form("f", NB, NT, NW, (ncols + 16 * NW - 1) // (16 * NW))
    G = 0
    if ngroups > simds and inner >= 4:
        best = (ngroups + simds - 1) // simds * 4  # the plain form, in quarter sweeps
        for g in range(5, WRAP_MAXG + 1):
            if sweepqw_lds_bytes(16 * NT, NB, g) > LDS_LIMIT:
                break
            wgs = (ngroups + g - 1) // g
            rounds = (wgs + cus - 1) // cus
            if rounds * g < best:  # (strictly less: a tie keeps the smaller G)
                best, G = rounds * g, g
    if G:
        return Form("qw", NB, NT, G, (ngroups + G - 1) // G)
    return Form("q", NB, NT, 4, (ncols + 63) // 64)


ROW_CLASSES = ((1, 16), (2, 32), (3, 48), (4, 50))   # (CPL, KR) of sweep_row_kernel (tu_sweepr.hip): k <= 16, 32, 48, 50


def instantiation(form, masked):
    """The template arguments a launch of `form` instantiates, as the tu_*.hip switch tables spell them."""
    if form.family == "r":
        return ("r",) + ROW_CLASSES[form.NT - 1] + (masked, form.groups)
    if form.family == "f":
        return ("f", form.NT, form.NB, masked, form.groups)
    return (form.family, form.NT, form.NB, masked)


def all_instantiations():
    """The 144 instantiations of the four switch tables."""
    out = set()
    for NB in range(1, 17):
        NT = (NB + 3) // 4
        for mk in (False, True):
            out.add(("q", NT, NB, mk))
            out.add(("qw", NT, NB, mk))
            for NW in (4, 8):
                out.add(("f", NT, NB, mk, NW))
    for cpl, kr in ROW_CLASSES:
        for mk in (False, True):
            for NW in (4, 8):
                out.add(("r", cpl, kr, mk, NW))
    return out


def variants_of(k):
    return tuple(VARIANTS) if k in NT_ENDS else ("plain", "masked")


def cus_of(prec, k):
    if prec == "f64":
        return CUS_F64
    return CUS_F32 if k <= SWEEPR_KMAX else CUS_F32[:2]


def case_name(k, variant, setting):
    return f"k{k}-{variant}-{setting}"


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
def masked_columns(n=N):
    """The fully masked columns of a masked case: column 3, the last column of the last full wavefront of 16 (q, qw, f) and of 4 (r),
    and the last column."""
    return sorted({3, n // 16 * 16 - 1, n // 4 * 4 - 1, n - 1})


@functools.lru_cache(maxsize=8)
def make_case(k, variant, n=N, m=M):
    """dict(A n x m, W0 n x k, H0 k x m, Wm, Hm (bool or None), reg): the fuzz's planted model of rank k + 3 plus noise plus an offset,
    a start near the planted factors.  The planted W has exact zeros whose rows of A have 0.3 of the coordinate's row of H taken out (8 %:
    the start is zero there and most of them stay zero in the solution) and the start has further zeros (5 %: they leave zero).  Masked variants: about 10 % of the entries of both factors, bit 0 and bit k - 1 somewhere,
    the columns of masked_columns() entirely; masked entries of the start hold values other than zero."""
    masked, pen = VARIANTS[variant]
    rng = np.random.default_rng(100000 * list(VARIANTS).index(variant) + 1000 * k + n)
    Wp, Hp = rng.random((n, k + 3)) ** 2 + 0.05, rng.random((k + 3, m)) ** 2 + 0.05
    S = rng.random((n, k)) < 0.08
    Wp[:, :k][S] = 0.0
    A = np.maximum((Wp - 0.3 * np.pad(S, ((0, 0), (0, 3)))) @ Hp, 0.0) / (k + 3) * 4 + 0.02 * rng.random((n, m)) + 0.01
    sc = 2.0 / np.sqrt(k + 3)
    W0, H0 = Wp[:, :k] * sc * (0.7 + 0.6 * rng.random((n, k))), Hp[:k, :] * sc * (0.7 + 0.6 * rng.random((k, m)))
    W0[rng.random((n, k)) < 0.05] = 0.0
    Wm = Hm = None
    if masked:
        Wm, Hm = rng.random((n, k)) < 0.10, rng.random((k, m)) < 0.10
        Wm[5, 0] = Wm[7, k - 1] = True
        Wm[masked_columns(n), :] = True
        W0[Wm] = 0.3 * W0[Wm] + 0.02
        H0[Hm] = 0.3 * H0[Hm] + 0.02
    for a in (A, W0, H0):
        a.setflags(write=False)
    return dict(k=k, n=n, m=m, variant=variant, A=A, W0=W0, H0=H0, Wm=Wm, Hm=Hm, reg=list(REG if pen else NOREG))


def live_columns(c):
    """Columns of the W half-step (rows of W) that are not masked entirely: the ones update() solves."""
    return c["n"] if c["Wm"] is None else int((~c["Wm"].all(axis=1)).sum())


def live_columns_h(c):
    return c["m"] if c["Hm"] is None else int((~c["Hm"].all(axis=0)).sum())


def oracle_w(ref, c, inner, tol, reverse=False):
    """(W n x k, sweeps) of the oracle's W half-step.  reverse: the contraction (the m columns of A and of H) in the opposite order -- the
    same sums in another order of addition."""
    A, H0 = (c["A"][:, ::-1], c["H0"][:, ::-1]) if reverse else (c["A"], c["H0"])
    Wt, it = ref.update(c["W0"].T, H0, A.T, None if c["Wm"] is None else c["Wm"].T, c["reg"], inner, tol, 1)
    return np.ascontiguousarray(Wt.T), int(it)


def oracle_h(ref, c, W, inner, tol, reverse=False):
    """(H k x m, sweeps) of the oracle's H half-step from the factor W; reverse: the n rows of A and of W in the opposite order."""
    A, W = (c["A"][::-1], W[::-1]) if reverse else (c["A"], W)
    H, it = ref.update(c["H0"], W.T, A, c["Hm"], c["reg"], inner, tol, 1)
    return np.ascontiguousarray(H), int(it)


@functools.lru_cache(maxsize=16)
def oracle_chain(ref, k, variant, w_setting, h_setting=None, reverse=False, n=N):
    """(W, sweeps of the W half-step, H, sweeps of the H half-step) of the oracle: the W half-step at w_setting = (inner, tol), then the H
    half-step from its result at h_setting (default: the same)."""
    c = make_case(k, variant, n)
    W, itw = oracle_w(ref, c, w_setting[0], w_setting[1], reverse)
    H, ith = oracle_h(ref, c, W, *(h_setting or w_setting), reverse=reverse)
    return W, itw, H, ith


def stop_slack(ref, c, which, X, X_ref, W_fixed, setting, bar, oracles=None):
    """For the fp32-operand mode at the LOOSE setting.  There the sweep at which a column stops is tolerance-only.  The
    quantity compared with the tolerance is the largest relative change of a sweep, max over the coordinates of 2 |d| / (x + x' + eps),
    and a coordinate that enters or leaves zero changes by 2 whatever its size: whether a coordinate at a thousandth of the column's
    scale crosses zero in this sweep or the next rides on the fp32 chain's error (1e-6 of that scale), and with it whether the column
    stops here -- at sweep 28 of k46-plain-loose the oracle's column 143 of H has such a crossing (change 2.0) and 0.042 a sweep later.
    A column that does not stop where the oracle's did runs on as the oracle's would have.  At a tolerance of 1e-1 one sweep moves a
    column by percents; no fp32 chain can promise otherwise.  So where a factor misses the bar against the oracle's result, every
    column (of the solved factor X; `which` = 0: rows of W, 1: columns of H) that misses it is held to the bar against the oracle's own
    trajectory -- the oracle's column after exactly t sweeps, t = 1 .. the limit -- at the sweep that fits best.
    Returns (relative Frobenius deviation under that allowance, the columns that took another sweep than the oracle's stopping sweep).
    oracles: (oracle_w, oracle_h) of another family of cases with the signatures of this module's (tests/na_solver_cases.py)."""
    inner, tol = setting
    ow, oh = oracles or (oracle_w, oracle_h)
    traj = []
    for t in range(inner + 1):  # the oracle's factor after exactly t sweeps of every live column (a negative tolerance never stops)
        traj.append(ow(ref, c, t, -1.0)[0] if which == 0 else oh(ref, c, W_fixed, t, -1.0)[0].T)
    G, R = (X, X_ref) if which == 0 else (X.T, X_ref.T)  # one column of the half-step per row
    total, flipped = 0.0, []
    for j in range(G.shape[0]):
        own = float(np.sum((G[j] - R[j]) ** 2))
        assert any(np.array_equal(traj[t][j], R[j]) for t in range(inner + 1)), ("the oracle's column is on its own trajectory", which, j)
        if own > bar * bar * float(np.sum(R[j] ** 2)):
            best = min(float(np.sum((G[j] - traj[t][j]) ** 2)) for t in range(1, inner + 1))
            if best < own:
                own = best
                flipped.append(j)
        total += own
    return float(np.sqrt(total) / np.linalg.norm(R)), flipped


# Loose-tolerance cases whose oracle sweep counts differ between the two summation orders (test_scd_sweep_cases_host.py asserts that this
# is the list, and that it holds at most 5 % of the cases): the strict GPU count is compared exactly everywhere else.
LOOSE_ORDER_DEPENDENT = frozenset()
