"""Cases of the batched KL factorisation on a sparse count matrix (nnlm_set_matrix_csc_kl_batch, k_sparse_kl_batch.h):
tests/test_gpu_sparse_kl_batch.py runs them on the GPU, tests/test_sparse_kl_batch_host.py shows the ones compared with the oracle well
posed from the oracle alone.  numpy only, deterministic; built on sparse_kl_cases.py and sparse_cases.py.

A batch case is a dict: S = the CSC tuple of sparse_cases (absent entries zeros), ks = the members' ranks, inits = [(W0_b, H0_b)], name.
The data are Poisson counts of ONE planted non-negative model of the largest rank (zeros leave the structure; on a designed pattern the
stored values are 1 + Poisson, which keeps the pattern); member b starts near the first k_b planted components, scaled to the level of
the data (structureless starts let factors die on the way, see sparse_cases.py)."""
import numpy as np

import sparse_cases as sc
import sparse_kl_cases as kc

Z3 = [0.0, 0.0, 0.0]
GROUPS = (1, 2, 4)  # the group sizes sp_kl_batch_kernel is built for ("sparse_kl_batch_group" is one of them)


def _starts(Wp, Hp, ks, level, rng):
    """One start per member: the first k_b planted components with 0.7 ... 1.3 relative noise, at the level `level` x the full model's."""
    full = float(np.mean(Wp @ Hp))
    inits = []
    for k in ks:
        W, H = Wp[:, :k], Hp[:k]
        f = np.sqrt(level * full / float(np.mean(W @ H)))
        n, m = W.shape[0], H.shape[1]
        inits.append((W * f * (0.7 + 0.6 * rng.random((n, k))), H * f * (0.7 + 0.6 * rng.random((k, m)))))
    return inits


def count_batch(n, m, ks, density, seed, mean=4.0):
    """Poisson counts of a planted model of rank max(ks) on a random pattern of the given density."""
    rng = np.random.default_rng(830000 + seed)
    Wp, Hp, _, _ = kc._planted(n, m, max(ks), rng, mean)
    keep = np.ones((n, m), dtype=bool) if density >= 1.0 else rng.random((n, m)) < density
    C = rng.poisson(Wp @ Hp) * keep
    S = sc.csc_from_pattern(C > 0, C.astype(np.float64))
    return dict(S=S, ks=list(ks), inits=_starts(Wp, Hp, ks, min(density, 1.0), rng), name="counts %dx%d d%g ks%s" % (n, m, density, list(ks)))


def pattern_batch(P, ks, seed, name):
    """1 + Poisson counts of a planted model of rank max(ks) at the entries of the boolean pattern P."""
    n, m = P.shape
    rng = np.random.default_rng(840000 + seed)
    Wp, Hp, _, _ = kc._planted(n, m, max(ks), rng, 3.0)
    V = 1.0 + rng.poisson(Wp @ Hp)
    return dict(S=sc.csc_from_pattern(P, V), ks=list(ks), inits=_starts(Wp, Hp, ks, max(float(P.mean()), 1e-3), rng), name=name)


def from_solo(c, ks, seed):
    """A batch on the matrix (and pattern) of the solo case c of sparse_kl_cases.py."""
    b = pattern_batch(sc.pattern_of(c["S"]), ks, seed, c["name"] + " ks%s" % list(ks))
    b["S"] = c["S"]  # (the solo case's own counts)
    return b


def line_cases(ks=(3, 5, 2)):
    """The designed line lengths (both orientations: the batched short kernel and the per-member long launches in one half-step), a line
    holding half of all entries (both orientations), and the four pattern families."""
    out = [from_solo(kc.lines_case(kc.THRESHOLD_COUNTS, 5, tr), ks, 10 + int(tr)) for tr in (False, True)]
    out += [from_solo(kc.half_case(700, 60, 6, tr), ks, 20 + int(tr)) for tr in (False, True)]
    out += [from_solo(kc.family_case(f), ks, 30 + i) for i, f in enumerate(("empty_lines", "powerlaw", "powerlaw_rows", "heavy"))]
    return out


def family_pattern(family, n, m, rng):
    if family == "uniform":
        return rng.random((n, m)) < 0.15
    if family == "empty_lines":
        return sc._empty_lines(n, m, rng)
    if family == "powerlaw":
        return sc._powerlaw(n, m, rng, by_rows=False)
    if family == "powerlaw_rows":
        return sc._powerlaw(n, m, rng, by_rows=True)
    if family == "heavy":
        return sc._heavy(n, m, rng)
    raise ValueError(family)


FUZZ_FAMILIES = ("uniform", "empty_lines", "powerlaw", "powerlaw_rows", "heavy")
# The first twelve seeds of the randomised loop, chosen on the CPU among 0 .. 89 so that every one has members that well_posed() accepts,
# over all five families, both methods and one to three Lee sweeps, and seed -> those members (tests/test_sparse_kl_batch_host.py checks
# the table against the oracle): they alone are compared with the oracle; every member of every seed is compared with its solo run bit
# for bit.  (SCD on the power-law and heavy-tailed patterns leaves rounding dust in every seed tried: those families meet the oracle
# with Lee.)  Further seeds (NNLM_FUZZ_SEEDS above its default) are 100, 101, ...: parity with the solo run only.
FUZZ_SEEDS = (60, 55, 85, 26, 31, 56, 27, 47, 23, 33, 9, 49)
FUZZ_WELL_POSED = {60: [0, 2, 3, 4, 5], 55: [0, 1, 2, 3, 4, 5, 6, 7], 85: [0, 1, 2, 3, 4, 5, 6, 7], 26: [0, 1, 2, 3, 5, 6],
                   31: [0, 1, 2, 3, 4, 5, 6, 7, 8], 56: [1, 3, 4, 5, 6], 27: [0, 1, 2, 3, 4, 5, 6, 7], 47: [3], 23: [0, 1, 2, 3], 33: [1, 6],
                   9: [0, 5, 6], 49: [5, 7]}


def fuzz_seed(i):
    """The seed of the i-th case of the randomised loop."""
    return FUZZ_SEEDS[i] if i < len(FUZZ_SEEDS) else 100 + i


def fuzz_case(seed):
    """Randomised parity: a pattern family, random ranks with a sum of at most 64, Lee or SCD -- all drawn from the seed."""
    rng = np.random.default_rng(850000 + seed)
    family = FUZZ_FAMILIES[seed % len(FUZZ_FAMILIES)]
    n, m = int(rng.integers(90, 330)), int(rng.integers(70, 300))
    B = int(rng.integers(1, 10))
    ks, left = [], 64
    for _ in range(B):
        if left < 1:
            break
        k = int(min(left, rng.integers(1, 12 if B > 3 else 30)))
        ks.append(k)
        left -= k
    c = pattern_batch(family_pattern(family, n, m, rng), ks, 1000 + seed, "fuzz %d %s %dx%d ks%s" % (seed, family, n, m, ks))
    c["method"] = 3 + seed % 2
    c["inner"] = 1 if c["method"] == 3 else int(rng.integers(1, 4))  # (SCD-KL with several inner sweeps is chaotic, test_sparse_kl_host.py)
    c["alpha"], c["beta"] = (list(kc.REGS["l2"]), list(kc.REGS["l1"])) if seed % 3 == 0 else (Z3, Z3)
    c["max_iter"] = 4
    return c


# ---- the cases the GPU file compares with the ORACLE (tests/test_sparse_kl_batch_host.py shows each of them well posed) -----------------
ORACLE_ITERS = 6
ORACLE_REG = ([0.01, 0, 0.01], [0, 0.01, 0.02])


def oracle_cases():
    """(case, method, inner): Lee with several inner sweeps, SCD with one (SCD-KL with more is chaotic on such data)."""
    a = count_batch(150, 110, [3, 4, 7], 0.5, 1)  # (seeds 2, 3: SCD leaves rounding dust in the rank-3 member's factors)
    b = count_batch(150, 110, [5, 2, 8, 3, 6], 1.0, 3)  # (seeds 1, 2: the same in the rank-2 member's)
    return [(a, 3, 1), (a, 4, 3), (b, 3, 1), (b, 4, 2)]


def perturbed(init, rng, size=1e-13):
    W, H = init
    return W * (1 + size * rng.standard_normal(W.shape)), H * (1 + size * rng.standard_normal(H.shape))


def oracle_run(ref, A, k, init, method, inner, iters=ORACLE_ITERS, reg=ORACLE_REG, rel_tol=-1.0, trace=1):
    W, H = init
    return ref.c_nnmf(A, k, W, H, None, None, reg[0], reg[1], iters, rel_tol, 1, 0, False, inner, 1e-9, method, trace)


def well_posed(ref, A, k, init, method, inner, iters=ORACLE_ITERS, reg=ORACLE_REG):
    """The conditions of test_sparse_kl_host.py on a whole run, from the oracle alone: finite, nothing dies, no rounding dust in the
    factors the next half-step has fixed (a live entry below 1e-7 of the largest), and the result moves by < 1e-11 under a 1e-13
    perturbation of the start.  Returns (ok, what failed)."""
    o = oracle_run(ref, A, k, init, method, inner, iters, reg)
    W, H = o["W"], o["H"]
    if not (np.all(np.isfinite(W)) and np.all(np.isfinite(H))):
        return False, "not finite"
    dw, dh = (W * W).sum(axis=0), (H * H).sum(axis=1)
    if not (dw.min() > 1e-8 * np.median(dw) and dh.min() > 1e-8 * np.median(dh)):
        return False, "a factor died"
    for X in (W, H):
        live = X[X > 0]
        if live.size and live.min() <= 1e-7 * X.max():
            return False, "dust %.3g" % float(live.min() / X.max())
    rng = np.random.default_rng(1)
    for _ in range(2):
        p = oracle_run(ref, A, k, perturbed(init, rng), method, inner, iters, reg)
        moved = max(sc.err(p["W"], W), sc.err(p["H"], H))
        if not moved <= 1e-11:
            return False, "moved %.3g" % moved
        if not np.array_equal(p["average_epoch"], o["average_epoch"]):
            return False, "sweep counts moved"
    return True, ""
