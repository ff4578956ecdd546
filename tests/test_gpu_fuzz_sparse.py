"""Randomised parity of the sparse (absent = zero: k_sparse.h), sparse-missing (absent = missing: k_sparse_na.h) and batched (k_batch.h)
flows against the fp64 oracle (oracle.ref) on the DENSIFIED matrix -- zeros at the absent entries for `csc`, NaN for `csc_missing` --,
with the case generators of sparse_cases.py.  NNLM_FUZZ_SEEDS (default 16) sets the number of seeds per test, as in test_gpu_fuzz.py.

Bars (all the project's existing ones).  Strict mode: factors 1e-9 relative Frobenius over whole runs (1e-8 over the up-to-80-iteration
runs of the stopping rule, 1e-10 over single half-steps), iteration counts, trace lengths and sweep counts exact; traces at rtol 1e-8
under absent = missing and, under absent = zero, mse within 1e-12 mean(A^2) + 1e-10 mse (its sum of squares is formed by a Gram
cancellation) and mkl within 1e-10 + 4e-15 (the 3.7e-15 per left-out zero of sp_err_final_kernel).  F32 mode: 1e-4 on factors, rtol 1e-3
on traces.  The only skips are degenerate() cases (a factor dies on the oracle's own way), decided by the oracle alone; under absent =
missing a non-empty line with fewer stored entries than k has a rank-deficient Gram, and there -- only there -- average_epoch is compared
with the dense fuzz's tolerance (2 inner + 1e-9) / (n + m) instead of equality."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_cases as sc  # noqa: E402
from helpers import relF  # noqa: E402
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib  # noqa: E402
from oracle import ref  # noqa: E402

pytestmark = pytest.mark.gpu

SEEDS = int(os.environ.get("NNLM_FUZZ_SEEDS", "16"))
MODES = ("f64", "f32")
PREC = {"f64": _lib.PREC_F64, "f32": _lib.PREC_F32}
NNMF = {"zero": _lib.c_nnmf_csc, "missing": _lib.c_nnmf_csc_missing}
NNLM = {"zero": _lib.c_nnlm_csc, "missing": _lib.c_nnlm_csc_missing}
SKIP = "a factor dies on the oracle's way: not reproducible (see make_case of test_gpu_fuzz.py)"


def set_matrix(h, c):
    (h.set_matrix_csc_missing if c["semantics"] == "missing" else h.set_matrix_csc)(*c["S"])


def run_both(c):
    return NNMF[c["semantics"]](*c["S"], *sc.nnmf_args(c)), ref.c_nnmf(sc.densify(c["S"], c["semantics"]), *sc.nnmf_args(c))


def check_traces(r, o, c, A, mode, d):
    """mse / mkl / target traces of a whole run against the oracle's."""
    for key in ("mse_error", "mkl_error", "target_error", "average_epoch"):
        assert r[key].shape == o[key].shape, (key, d)
    if mode == "f32":
        assert np.allclose(r["mse_error"], o["mse_error"], rtol=1e-3, atol=1e-12), d
        assert np.allclose(r["target_error"], o["target_error"], rtol=1e-3, atol=1e-9), d
        return
    if c["semantics"] == "missing":
        assert np.allclose(r["mse_error"], o["mse_error"], rtol=1e-8, atol=1e-13), d
        assert np.allclose(r["mkl_error"], o["mkl_error"], rtol=1e-8, atol=1e-11), d
        assert np.allclose(r["target_error"], o["target_error"], rtol=1e-8, atol=1e-11), d
        return
    bound = 1e-12 * np.mean(A * A) + 1e-10 * o["mse_error"]
    dm = np.abs(r["mse_error"] - o["mse_error"])
    assert np.all(dm <= bound), (float(np.max(dm / bound)), d)
    dk = np.abs(r["mkl_error"] - o["mkl_error"])
    assert np.all(dk <= 1e-10 * np.abs(o["mkl_error"]) + 4e-15), (float(dk.max()), d)
    dt = np.abs(r["target_error"] - o["target_error"])  # (methods 1, 2: the target is mse / 2 + the penalties)
    assert np.all(dt <= 0.5 * bound + 1e-10 * np.abs(o["target_error"])), (float(dt.max()), d)


def check_run(c, mode):
    if sc.degenerate(c, ref):
        pytest.skip(SKIP)
    r, o = run_both(c)
    d = sc.describe(c)
    ew, eh = relF(r["W"], o["W"]), relF(r["H"], o["H"])
    print(f"FUZZ {mode} {c['semantics']} seed {c['seed']} {c['family']}: W {ew:.3e} H {eh:.3e} nit {r['n_iteration']}/{o['n_iteration']}")
    assert r["n_iteration"] == o["n_iteration"] and r["warning"] == o["warning"], d
    A = sc.densify(c["S"], "zero")
    check_traces(r, o, c, A, mode, d)
    if mode == "f64":
        if sc.rank_deficient(c):
            n, m = c["S"][3]
            assert np.allclose(r["average_epoch"], o["average_epoch"], rtol=0, atol=(2.0 * c["inner"] + 1e-9) / (n + m)), d
        else:
            assert np.array_equal(r["average_epoch"], o["average_epoch"]), (r["average_epoch"], o["average_epoch"], d)
    tol = 1e-9 if mode == "f64" else 1e-4
    assert ew < tol and eh < tol, (ew, eh, d)
    if c["Wm"] is not None:
        assert np.all(r["W"][c["Wm"] != 0] == 0) and np.all(r["H"][c["Hm"] != 0] == 0), d


# ---- 1. whole runs of the one-shot entries -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(SEEDS))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("semantics", sc.SEMANTICS)
def test_random_sparse_driver_runs(monkeypatch, semantics, mode, seed):
    """nnlm_c_nnmf_csc / nnlm_c_nnmf_csc_missing against ref.c_nnmf: rel_tol = -1, 1..5 iterations, trace 1..3, inner 1..7, masks on a
    third of the seeds, the four penalty triples, every pattern family and K-padding form (rank > 64 under absent = zero)."""
    monkeypatch.setenv("NNLM_PRECISION", mode)
    check_run(sc.make_case(seed, semantics), mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("semantics", sc.SEMANTICS)
def test_worker_cap_case_runs(monkeypatch, semantics, mode):
    """More than 16 * 64 * 256 non-zeros: the cap of 16 wavefronts per CU binds and a worker's range is no longer about 64 non-zeros."""
    monkeypatch.setenv("NNLM_PRECISION", mode)
    check_run(sc.make_cap_case(semantics), mode)


# ---- 2. the boundary family: single half-steps, whole factors and line by line -----------------------------------------------------------
def flagged_lines(ptr, k, alloc_limit):
    """The lines of one orientation a boundary case is built for: those in more than one spmm worker's range, the empty ones, those of
    2048 / 2049 entries, every long one (several Gram segments) and whatever boundary_events names."""
    ptr = np.asarray(ptr)
    length = np.diff(ptr)
    ev = sc.boundary_events(ptr, k, alloc_limit=alloc_limit)
    lines = set(sc.straddling_lines(ptr, k)) | {int(j) for j in np.flatnonzero((length == 0) | (length >= sc.SPG_SEG))}
    for cols in ev.values():
        lines |= set(cols)
    return sorted(lines), length


def check_lines(X, R, lines, length, tol, what):
    """X, R: [k][lines] factor and the oracle's.  Max-abs deviation of each flagged non-empty line relative to the norm of the oracle's
    line (the empty ones: test_boundary_empty_lines_equal_the_oracle_exactly)."""
    worst = 0.0
    for j in lines:
        if length[j] == 0:
            continue
        dev = float(np.max(np.abs(X[:, j] - R[:, j]))) / float(np.linalg.norm(R[:, j]))
        worst = max(worst, dev)
        assert dev <= tol, (what, "line", j, "stored", int(length[j]), dev)
    return worst


# Penalties of the boundary half-steps.  Under absent = zero a line without stored entries has the exact solution 0, and without an L1
# term the coordinate descent leaves it at the rounding dust of G x / G_qq -- 1e-16 of the start, at coordinates decided by the summation
# order of the shared Gram, and with it the sweep counts (the degenerate regime of DESIGN 2: measured, 12 of 12 cases).  With an L1 term
# the step is negative before it is clamped: both sides land on exact zeros and the comparison is well posed.  Under absent = missing
# the Gram of an empty line is TINY I + the penalty in any order, so the L2-only triple of test_edge_structure_half_steps runs as well.
BOUNDARY_REGS = {"zero": ([0.02, 0.01, 0.03],), "missing": ([0.01, 0.0, 0.0], [0.02, 0.01, 0.03])}


def boundary_half_steps(c, mode, method, reg, inner=5):
    """One W and one H half-step of a boundary case on a fresh handle (under the case's allocation limit: several Gram chunks) and the
    oracle's -> W1, H1, sweeps of each, the oracle's W^T, H and sweeps."""
    A = sc.densify(c["S"], c["semantics"])
    miss = bool(np.isnan(A).any())
    k, W0, H0, reg = c["k"], c["W0"], c["H0"], list(reg)
    _lib.debug_alloc_limit(c["alloc_limit"])
    try:
        with nnlm_amd.Handle(0, PREC[mode]) as h:
            set_matrix(h, c)
            h.set_factors(k, W0, H0)
            h.half_step(0, reg, inner, 1e-9, method)
            W1, _ = h.get_factors()
            s1 = h.take_sweeps()
            h.half_step(1, reg, inner, 1e-9, method)
            _, H1 = h.get_factors()
            s2 = h.take_sweeps()
    finally:
        _lib.debug_alloc_limit(0)
    Wt_ref, it1 = ref.update(W0.T.copy(), H0, A.T.copy(), None, reg, inner, 1e-9, method, missing=miss)
    # (strict: the oracle's own W, as check_half_steps of test_gpu_sparse_missing.py -- sweep counts stay exact; fp32: the W this
    #  half-step actually had fixed)
    H_ref, it2 = ref.update(H0, Wt_ref if mode == "f64" else W1.T.copy(), A, None, reg, inner, 1e-9, method, missing=miss)
    return W1, H1, (s1, s2), Wt_ref, H_ref, (it1, it2)


BOUNDARY_NAMES = [c["name"] for c in sc.boundary_cases("zero")]


@pytest.mark.parametrize("case", range(len(BOUNDARY_NAMES)), ids=BOUNDARY_NAMES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("semantics", sc.SEMANTICS)
def test_boundary_structures_half_steps(semantics, mode, case):
    """One W and one H half-step on every boundary case (columns, segments and empty runs exactly on worker and chunk boundaries:
    test_sparse_cases_host.py) against ref.update on the densified matrix: whole factors at 1e-10 / 1e-4 with exact sweep counts in
    strict mode, and the lines the case was built for one by one -- a relative Frobenius error over a whole factor can hide one
    wrong column among thousands."""
    c = sc.boundary_cases(semantics)[case]
    tol, strict = (1e-10, True) if mode == "f64" else (1e-4, False)
    k = c["k"]
    csr_ptr = sc.transpose_csc(c["S"])[0]
    for method, reg in ((mt, rg) for mt in (1, 2) for rg in BOUNDARY_REGS[semantics]):
        W1, H1, sweeps, Wt_ref, H_ref, its = boundary_half_steps(c, mode, method, reg)
        what = f"{mode} {semantics} {c['name']} method {method} reg {reg}"
        ew, eh = sc.err(W1, Wt_ref.T), sc.err(H1, H_ref)
        lw, len_w = flagged_lines(csr_ptr, k, c["alloc_limit"])
        lh, len_h = flagged_lines(c["S"][0], k, c["alloc_limit"])
        print(f"BOUNDARY {what}: W {ew:.3e} H {eh:.3e} sweeps {sweeps} / {its}")
        ww = check_lines(W1.T, Wt_ref, lw, len_w, tol, what + " W")
        wh = check_lines(H1, H_ref, lh, len_h, tol, what + " H")
        print(f"BOUNDARY {what}: worst flagged line W {ww:.3e} ({len(lw)}) H {wh:.3e} ({len(lh)})")
        assert ew <= tol and eh <= tol, f"{what}: W {ew:.3e}, H {eh:.3e} (bound {tol:g})"
        assert np.all(W1 >= 0) and np.all(H1 >= 0)
        if strict:
            assert sweeps == its, what


@pytest.mark.parametrize("semantics", sc.SEMANTICS)
def test_boundary_empty_lines_equal_the_oracle_exactly(semantics):
    """Strict mode: the empty rows and columns of every boundary case (runs of them on worker boundaries, leading and trailing ones)
    must come out as the oracle's do, bit for bit (penalties: BOUNDARY_REGS)."""
    bad = []
    for c in sc.boundary_cases(semantics):
        rows, cols = sc.line_counts(c["S"])
        for method, reg in ((mt, rg) for mt in (1, 2) for rg in BOUNDARY_REGS[semantics]):
            W1, H1, _, Wt_ref, H_ref, _ = boundary_half_steps(c, "f64", method, reg)
            for X, R, empty, side in ((W1.T, Wt_ref, rows == 0, "W"), (H1, H_ref, cols == 0, "H")):
                assert empty.any(), (c["name"], side)
                if not np.array_equal(X[:, empty], R[:, empty]):
                    bad.append((c["name"], method, reg, side, float(np.max(np.abs(X[:, empty]))), float(np.max(np.abs(R[:, empty])))))
    print(f"EMPTY {semantics}: {len(bad)} factor(s) whose empty lines differ from the oracle's: {bad}")
    assert not bad, bad


def test_work_split_restatements_match_the_library():
    """sparse_cases.py restates nnlm_sp_workers, nnlm_spg_workers and the chunk plan of the per-column Grams to locate boundaries; the
    counts it predicts must be the handle's own, or the boundary family no longer sits where the host test says it does."""
    cases = sc.boundary_cases("missing") + [sc.make_cap_case("missing"), sc.make_case(2, "missing"), sc.make_case(8, "missing")]
    for c in cases:
        limit = c.get("alloc_limit", 0)
        _lib.debug_alloc_limit(limit)
        try:
            with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
                set_matrix(h, c)
                h.set_factors(c["k"], c["W0"], c["H0"])
                cus = int(h.get_info("cus"))
                for which, ptr in ((0, sc.transpose_csc(c["S"])[0]), (1, c["S"][0])):
                    h.half_step(which, [0.01, 0, 0], 1, 1e-9, 1)
                    got = {key: int(h.get_info(key)) for key in ("sp_workers", "sp_gram_workers", "sp_gram_chunks")}
                    assert got == sc.predicted_counts(ptr, c["k"], cus, limit), (c.get("name", c["family"]), which, got)
        finally:
            _lib.debug_alloc_limit(0)
    c = sc.make_cap_case("zero")
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
        set_matrix(h, c)
        h.set_factors(c["k"], c["W0"], c["H0"])
        assert int(h.get_info("sp_workers")) == 16 * int(h.get_info("cus")) == sc.sp_workers(c["S"][1].size, sc.kp_of(c["k"]), int(h.get_info("cus")))


# ---- 3. the stopping rule ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(max(1, SEEDS // 2)))  # (up to 80 iterations each)
@pytest.mark.parametrize("semantics", sc.SEMANTICS)
def test_random_sparse_stopping_rule(monkeypatch, semantics, seed):
    """The sparse twin of test_random_driver_stopping_rule: the strict mode stops at the oracle's iteration with its traces, warning
    flag, sweep counts and factors; the F32 mode within one trace interval.  Then the resident API to the same stop and nnlm_errors on
    the handle: the factors the handle holds are those of the last trace entry -- a speculative W half-step that was kept is caught here."""
    c = sc.make_stop_case(seed, semantics)
    if sc.degenerate(c, ref):
        pytest.skip(SKIP)
    A = sc.densify(c["S"], semantics)
    o = ref.c_nnmf(A, *sc.nnmf_args(c))
    d = dict(sc.describe(c), n_iteration=o["n_iteration"])
    monkeypatch.setenv("NNLM_PRECISION", "f64")
    r = NNMF[semantics](*c["S"], *sc.nnmf_args(c))
    print(f"STOP {semantics} seed {seed}: oracle stops at {o['n_iteration']} (trace {c['trace']}), strict at {r['n_iteration']}, "
          f"W {relF(r['W'], o['W']):.3e} H {relF(r['H'], o['H']):.3e}")
    assert r["n_iteration"] == o["n_iteration"] and r["warning"] == o["warning"], (r["n_iteration"], d)
    assert r["target_error"].shape == o["target_error"].shape and np.allclose(r["target_error"], o["target_error"], rtol=1e-7, atol=1e-12), d
    assert r["mse_error"].shape == o["mse_error"].shape and r["mkl_error"].shape == o["mkl_error"].shape, d
    if sc.rank_deficient(c):
        n, m = c["S"][3]
        assert np.allclose(r["average_epoch"], o["average_epoch"], rtol=0, atol=(2.0 * c["inner"] + 1e-9) / (n + m)), d
    else:
        assert np.array_equal(r["average_epoch"], o["average_epoch"]), d
    assert relF(r["W"], o["W"]) < 1e-8 and relF(r["H"], o["H"]) < 1e-8, (relF(r["W"], o["W"]), relF(r["H"], o["H"]), d)
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
        set_matrix(h, c)
        h.set_factors(c["k"], c["W0"], c["H0"], c["Wm"], c["Hm"])
        t = h.run(c["alpha"], c["beta"], c["max_iter"], c["rel_tol"], 0, False, c["inner"], 1e-9, c["method"], c["trace"])
        mse = h.errors()[0]
        W, H = h.get_factors()
    assert t["n_iteration"] == o["n_iteration"] and t["warning"] == o["warning"], (t["n_iteration"], d)
    assert len(t["mse_error"]) == len(o["mse_error"]), d
    assert np.isclose(mse, t["mse_error"][-1], rtol=1e-8, atol=0), (mse, t["mse_error"][-1], d)
    assert relF(W, o["W"]) < 1e-8 and relF(H, o["H"]) < 1e-8, (relF(W, o["W"]), relF(H, o["H"]), d)
    monkeypatch.setenv("NNLM_PRECISION", "f32")
    r = NNMF[semantics](*c["S"], *sc.nnmf_args(c))
    assert abs(r["n_iteration"] - o["n_iteration"]) <= c["trace"], (r["n_iteration"], d)
    if r["n_iteration"] == o["n_iteration"]:
        assert np.allclose(r["target_error"], o["target_error"], rtol=1e-3, atol=1e-9), d


# ---- 4. the one-shot nnlm entries --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(SEEDS))
@pytest.mark.parametrize("semantics", sc.SEMANTICS)
def test_random_sparse_nnlm_runs(monkeypatch, semantics, seed):
    """nnlm_c_nnlm_csc / nnlm_c_nnlm_csc_missing against ref.c_nnlm: the generator of test_random_nnlm_runs with methods 1, 2 and y
    sparsified by the pattern families; strict mode, sweep counts exact."""
    monkeypatch.setenv("NNLM_PRECISION", "f64")
    c = sc.make_nnlm_case(seed, semantics)
    d = sc.describe_nnlm(c)
    args = (c["alpha"], c["mask"], c["b0"], c["max_iter"], 1e-10, 1, c["method"])
    o = ref.c_nnlm(c["x"], sc.densify(c["S"], semantics), *args)
    if not np.isfinite(o["coefficient"]).all():
        pytest.skip("the oracle's own result is not finite")
    r = NNLM[semantics](c["x"], *c["S"], *args)
    e = relF(r["coefficient"], o["coefficient"])
    print(f"NNLM {semantics} seed {seed}: {e:.3e} sweeps {r['n_iteration']}/{o['n_iteration']}")
    assert e < 1e-9, (e, d)
    assert r["n_iteration"] == o["n_iteration"], (r["n_iteration"], o["n_iteration"], d)
    if c["mask"] is not None and c["b0"] is not None:
        assert np.all(r["coefficient"][c["mask"]] == 0)


# ---- 5. batches --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(SEEDS))
@pytest.mark.parametrize("mode", MODES)
def test_random_batch_runs(monkeypatch, mode, seed):
    """nnlm_c_nnmf_batch with random member counts, ranks (sum up to exactly 64, rank-1 members), methods, penalties, trace strides and
    stopping rules: every member against the oracle run on it alone -- a member frozen by its rule ends where the oracle's run ends."""
    monkeypatch.setenv("NNLM_PRECISION", mode)
    c = sc.make_batch_case(seed)
    d = sc.describe_batch(c)
    tail = (c["alpha"], c["beta"], c["max_iter"], c["rel_tol"], 1, 0, False, c["inner"], 1e-9, c["method"], c["trace"])
    refs = []
    for k, (W, H) in zip(c["ks"], c["inits"]):
        solo = dict(S=sc.csc_from_pattern(np.ones(c["A"].shape, dtype=bool), c["A"]), semantics="zero", k=k, W0=W, H0=H, Wm=None, Hm=None,
                    alpha=c["alpha"], beta=c["beta"], max_iter=c["max_iter"], rel_tol=c["rel_tol"], inner=c["inner"], method=c["method"], trace=c["trace"])
        if sc.degenerate(solo, ref):
            pytest.skip(SKIP)
        refs.append(ref.c_nnmf(c["A"], k, W, H, None, None, *tail))
    out = _lib.c_nnmf_batch(c["A"], c["ks"], [w for w, _ in c["inits"]], [x for _, x in c["inits"]], *tail)
    assert len(out) == len(c["ks"])
    for b, (r, o) in enumerate(zip(out, refs)):
        ew, eh = relF(r["W"], o["W"]), relF(r["H"], o["H"])
        print(f"BATCH {mode} seed {seed} member {b} rank {c['ks'][b]}: W {ew:.3e} H {eh:.3e} nit {r['n_iteration']}/{o['n_iteration']}")
        if mode == "f64":
            assert r["n_iteration"] == o["n_iteration"] and r["warning"] == o["warning"], (b, r["n_iteration"], o["n_iteration"], d)
            for key in ("mse_error", "mkl_error", "target_error"):
                assert r[key].shape == o[key].shape and np.allclose(r[key], o[key], rtol=1e-8, atol=1e-11), (b, key, d)
            assert np.array_equal(r["average_epoch"], o["average_epoch"]), (b, d)
            assert ew < 1e-9 and eh < 1e-9, (b, ew, eh, d)
        else:
            # (a stopping rule whose decisive quotient sits within the mode's 1e-4 of the threshold may fire one trace interval apart)
            assert abs(r["n_iteration"] - o["n_iteration"]) <= (c["trace"] if c["rel_tol"] > 0 else 0), (b, r["n_iteration"], o["n_iteration"], d)
            if r["n_iteration"] == o["n_iteration"]:
                assert len(r["mse_error"]) == len(o["mse_error"]), (b, d)
                assert ew < 1e-4 and eh < 1e-4, (b, ew, eh, d)
                assert np.allclose(r["mse_error"], o["mse_error"], rtol=1e-3, atol=1e-12), (b, d)
    if c["rel_tol"] > 0 and len(c["ks"]) > 1 and mode == "f64":
        print(f"BATCH seed {seed}: members stop at {[r['n_iteration'] for r in out]}")
