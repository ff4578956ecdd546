"""Batched factorisation on a sparse A whose absent entries are MISSING (nnlm_set_matrix_csc_missing_batch + the batch entries,
nnlm_c_nnmf_csc_missing_batch, api.nnmf_batch / api.nnmf_cv with sparse_batch = "missing") on the MI355X: every member against the fp64
oracle on the NaN-filled matrix and against the same member run alone on the sparse-missing path; the edges of the stack; bit-identity
(the per-column Grams of a member are the solo Grams, whatever the stack, the worker count and the chunking); segments and chunks;
stopping and frozen members; one launch per phase; the hold-out set; the API.  Run with `pytest -m gpu`.

Bounds (the project's own): strict fp64 mode 1e-10 with equal iteration and sweep counts; fp32-operand mode max(1e-4, the solo fp32
run's own distance) against the oracle and 1e-5 against the solo fp32 run; held-out sums against numpy 1e-12 (strict) / 1e-3 (fp32).
Every case is shown well posed from the oracle alone by tests/test_sparse_missing_batch_host.py: nothing is skipped here.

Traces: the error sums of a batch come from sp_batch_errors_kernel, whose summation order is not the solo error kernel's, so a batch
member's traces agree with its solo run's to 1e-10, not to the bit; factors and sweep counts are compared bit for bit where the stacked
padded rank is the member's own (the SpMM then splits the stored entries alike)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import relF  # noqa: E402
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402
from oracle import ref  # noqa: E402
import cv_cases as cv  # noqa: E402
import sparse_cases as sc  # noqa: E402
import sparse_missing_batch_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = [("f64", _lib.PREC_F64, 1e-10), ("f32", _lib.PREC_F32, 1e-4)]
ERR_ARG, ERR_UNSUPPORTED = 1, 5
Z3 = [0.0, 0.0, 0.0]
PROF = ("spmm_h", "spmm_w", "sp_gram", "sweep_h", "sweep_w", "sp_batch_errors", "sp_errors", "batch_errors", "errors", "gram", "xprod_h", "xprod_w")
TRACES = ("mse_error", "mkl_error", "target_error")


@pytest.fixture(autouse=True)
def _default_precision(monkeypatch):
    monkeypatch.delenv("NNLM_PRECISION", raising=False)


def handle(prec, cus=0):
    if cus:
        _lib.debug_set_cus(cus)
    try:
        return nnlm_amd.Handle(0, prec)
    finally:
        _lib.debug_set_cus(0)


def run_args(c, method):
    return (c["alpha"], c["beta"], c["max_iter"], c["rel_tol"], 0, True, c["inner"], 1e-9, method, c["trace"])


def batch(prec, c, method, cus=0, limit=0, prof=False, holdout=None, ks=None, inits=None):
    ks = c["ks"] if ks is None else ks
    inits = c["inits"] if inits is None else inits
    _lib.debug_alloc_limit(limit)
    try:
        with handle(prec, cus) as h:
            h.set_matrix_csc_missing_batch(*c["S"], holdout=holdout)
            h.set_factors_batch(ks, [w for w, _ in inits], [x for _, x in inits])
            if prof:
                h.profile_enable(True)
            t = h.run_batch(*run_args(c, method))
            f = h.get_factors_batch()
            info = {key: int(h.get_info(key)) for key in ("sp_gram_batch_pairs", "sp_gram_chunks", "sp_gram_workers")}
            if prof:
                info["prof"] = {nm: h.profile_get(nm) for nm in PROF}
            if holdout is not None:
                info["holdout"] = h.holdout_errors()
    finally:
        _lib.debug_alloc_limit(0)
    for o, (W, H) in zip(t, f):
        o["W"], o["H"] = W, H
    return t, info


def solo(prec, c, b, method, door=False, S=None):
    with handle(prec) as h:
        S = c["S"] if S is None else S
        h.set_matrix_csc_missing_batch(*S) if door else h.set_matrix_csc_missing(*S)
        h.set_factors(c["ks"][b], *c["inits"][b])
        t = h.run(*run_args(c, method))
        t["W"], t["H"] = h.get_factors()
    return t


def oracle(c, b, method, A=None):
    A = sc.densify(c["S"], "missing") if A is None else A
    return ref.c_nnmf(A, c["ks"][b], *c["inits"][b], None, None, c["alpha"], c["beta"], c["max_iter"], c["rel_tol"], 1, 0, True, c["inner"], 1e-9,
                      method, c["trace"])


def dist(a, b):
    return sc.err(a, b)


def trace_gap(a, b):
    """(relF, largest absolute gap) of two traces; entries that are NaN in both (the mean over no stored entry at all: 0 / 0 in the
    oracle and in the library alike) count as equal."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    both = np.isnan(a) & np.isnan(b)
    a, b = np.where(both, 0.0, a), np.where(both, 0.0, b)
    return relF(a, b), float(np.max(np.abs(a - b), initial=0.0))


def check_member(o, r, tol, strict, solo_run=None):
    """o = batch member, r = reference run (oracle or solo); fp32 with solo_run: the bound is the solo fp32 path's own distance to r, at
    least tol.
    mkl_error: the library forms it as kl_const + (S3 + S2) / nnz, a difference of two numbers of the size of kl_const (here O(1)), each
    good to a few 1e-16; the oracle sums per-entry terms.  On a near-exact fit (the boundary family's planted products: mkl = 1e-6) the
    difference cancels six digits and the relative bound means nothing; the absolute term of test_gpu_sparse_batch.py / test_gpu_sparse.py
    (1e-10 |ref| + 4e-15) decides there, as it does in those files."""
    if solo_run is not None and not strict:
        tol = max(tol, 1.01 * dist(solo_run["W"], r["W"]), 1.01 * dist(solo_run["H"], r["H"]))
    dw, dh = dist(o["W"], r["W"]), dist(o["H"], r["H"])
    print("member k=%d: W %.3e H %.3e (bound %.3g)" % (o["W"].shape[1], dw, dh, tol))
    assert dw < tol and dh < tol, (dw, dh, tol)
    assert o["n_iteration"] == r["n_iteration"] and len(o["mse_error"]) == len(r["mse_error"])
    if strict:
        assert np.array_equal(o["average_epoch"], r["average_epoch"]), (o["average_epoch"], r["average_epoch"])
        for key in TRACES:
            rel, gap = trace_gap(o[key], r[key])
            print("  %s %.3e (largest gap %.3e)" % (key, rel, gap))
            assert rel < tol or (key == "mkl_error" and gap <= 4e-15), (key, rel, gap)


def check_batch(pname, prec, tol, c, method, **kw):
    """Every member against the oracle on the NaN-filled matrix and against the solo sparse-missing run from the same init."""
    strict = pname == "f64"
    A = sc.densify(c["S"], "missing")
    t, info = batch(prec, c, method, **kw)
    for b in range(len(c["ks"])):
        o, s = oracle(c, b, method, A), solo(prec, c, b, method)
        check_member(t[b], o, tol, strict, solo_run=s)
        check_member(t[b], s, tol if strict else 1e-5, strict)
    return t, info


def same_bits(a, b, keys=("W", "H", "average_epoch") + TRACES):
    for x, y in zip(a, b):
        assert x["n_iteration"] == y["n_iteration"]
        for key in keys:
            assert np.array_equal(x[key], y[key], equal_nan=True), (key, relF(x[key], y[key]))


MEMBERS, STACKS, CONTENTS, BOUNDARY = mc.member_cases(), mc.stack_edge_cases(), mc.content_cases(), mc.boundary_cases()


# ---- 1. member = oracle = solo sparse-missing run ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("case", range(len(MEMBERS)), ids=[c["name"] for c in MEMBERS])
def test_member_equals_oracle_and_solo_run(pname, prec, tol, method, case):
    """Densities 0.01, 0.2 and 1.0 (every entry stored: the shared-Gram half-step) x the three rank lists."""
    c = MEMBERS[case]
    _, info = check_batch(pname, prec, tol, c, method)
    full = c["S"][1].size == c["S"][3][0] * c["S"][3][1]
    assert info["sp_gram_batch_pairs"] == (0 if full else len(mc.tile_pairs(c["ks"])[0]))


# ---- 2. edges of the stack ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("case", range(len(STACKS)), ids=[c["name"] for c in STACKS])
def test_edges_of_the_stack(pname, prec, tol, method, case):
    """Member blocks on, ending at and straddling tile boundaries at every NT; the mask the kernel ran with is the restated rule's."""
    c = STACKS[case]
    _, info = check_batch(pname, prec, tol, c, method)
    assert info["sp_gram_batch_pairs"] == len(mc.tile_pairs(c["ks"])[0])


def test_pair_counts_of_the_three_named_stacks():
    got = {}
    for c in STACKS:
        if c["ks"] in ([8] * 8, list(range(1, 11)), [1]):
            _, info = batch(_lib.PREC_F64, dict(c, max_iter=1), 1)
            got[len(c["ks"])] = info["sp_gram_batch_pairs"]
    assert got == {8: 4, 10: 7, 1: 1}, got


# ---- 3. contents -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("case", range(len(CONTENTS)), ids=[c["name"] for c in CONTENTS])
def test_contents(pname, prec, tol, method, case):
    """Explicit stored zeros are observations; empty rows and columns; nothing stored; a column with one entry; the three penalties."""
    t, _ = check_batch(pname, prec, tol, CONTENTS[case], method)
    for o in t:
        assert np.all(np.isfinite(o["W"])) and np.all(np.isfinite(o["H"])) and np.all(o["W"] >= 0) and np.all(o["H"] >= 0)


def test_stored_zeros_are_not_absent_entries():
    c = CONTENTS[0]
    assert c["name"] == "stored_zeros" and (c["S"][2] == 0).sum() > 100
    keep = c["S"][2] != 0
    dropped = mc.split(c["S"], np.flatnonzero(~keep))[0]
    a, _ = batch(_lib.PREC_F64, c, 1)
    b, _ = batch(_lib.PREC_F64, dict(c, S=dropped), 1)
    assert min(relF(x["H"], y["H"]) for x, y in zip(a, b)) > 1e-3


# ---- 4. segments and chunks --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("case", range(len(BOUNDARY)), ids=[c["name"] for c in BOUNDARY])
def test_boundary_family_as_batches(pname, prec, tol, case):
    """Columns and rows of 2047 .. 4097 stored entries, long columns first and last of a chunk (nnlm_debug_alloc_limit), 64 compute
    units instead of 256: against the oracle and the solo run, and -- strict mode -- chunked = unchunked and 64 CUs = 256 CUs bit for
    bit (the traces of another CU count at 1e-10: the error kernel's wavefront count follows it)."""
    c = BOUNDARY[case]
    strict = pname == "f64"
    limit = mc.alloc_limit_of(c)
    for method in (1, 2):
        t, info = check_batch(pname, prec, tol, c, method, limit=limit)
        slot = mc.goff_of(c["ks"])[-1]
        chunks = mc.gram_chunks_of_slot(c["S"][0], slot, limit)  # (the H half-step's: the last one)
        assert info["sp_gram_chunks"] == len(chunks)
        assert info["sp_gram_workers"] == sum(sc.spg_workers(int(c["S"][0][c1] - c["S"][0][c0])) for c0, c1 in chunks)
        whole, iw = batch(prec, c, method)
        small, ism = batch(prec, c, method, cus=64, limit=limit)
        assert iw["sp_gram_chunks"] == 1
        if strict:
            same_bits(t, whole)
            same_bits(t, small, keys=("W", "H", "average_epoch"))
            for x, y in zip(t, small):
                for key in TRACES:
                    rel, gap = trace_gap(x[key], y[key])
                    assert rel < 1e-10 or (key == "mkl_error" and gap <= 4e-15), (key, rel, gap)
        else:
            for other in (whole, small):
                for x, y in zip(t, other):
                    assert relF(x["W"], y["W"]) < 1e-6 and relF(x["H"], y["H"]) < 1e-6
    lens = np.concatenate([np.diff(c["S"][0]), np.bincount(c["S"][1], minlength=c["S"][3][0])])
    print("longest line", lens.max(), "chunks", len(chunks), "workers", info["sp_gram_workers"], ism["sp_gram_workers"])


def test_worker_count_follows_the_compute_units():
    """More than 64 x 16 x 256 stored entries: 64 compute units cap the Gram workers below what 256 give; the factors keep their bits."""
    rng = np.random.default_rng(31)
    n, m, ks = 700, 600, [3, 6, 2]
    S = sc.csc_from_pattern(rng.random((n, m)) < 0.7, rng.random((n, m)) + 0.5 * rng.random((n, 6)) @ rng.random((6, m)))
    c = mc.case("cap", S, ks, [(rng.random((n, k)), rng.random((k, m))) for k in ks], max_iter=2, trace=1, inner=5)
    a, ia = batch(_lib.PREC_F64, c, 1)
    b, ib = batch(_lib.PREC_F64, c, 1, cus=64)
    nnz = S[1].size
    assert ia["sp_gram_workers"] == sc.spg_workers(nnz) and ib["sp_gram_workers"] == 1024 < ia["sp_gram_workers"], (nnz, ia, ib)
    same_bits(a, b, keys=("W", "H", "average_epoch"))


# ---- 5. bit-identity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("k", [5, 16, 33])
def test_one_member_is_the_solo_run_bit_for_bit(method, k):
    """Strict mode.  A solo run on the door's handle is the solo sparse-missing run, traces included.  A batch of ONE member ends with
    the factors and sweep counts of that run, bit for bit (same SpMM split, bit-equal Grams, the same solver launch); its traces come
    from the batch's error kernel (another summation order): 1e-10."""
    S, inits = mc.sbc.thinned(170, 150, 0.2, [k], 40 + k)
    c = mc.case("one", S, [k], inits, max_iter=6)
    plain, door = solo(_lib.PREC_F64, c, 0, method), solo(_lib.PREC_F64, c, 0, method, door=True)
    same_bits([door], [plain])
    t, _ = batch(_lib.PREC_F64, c, method)
    same_bits(t, [plain], keys=("W", "H", "average_epoch"))
    for key in TRACES:
        assert trace_gap(t[0][key], plain[key])[0] < 1e-10


@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [1, 2])
def test_independence_of_members(pname, prec, tol, method):
    """Permuting the members, or adding one that leaves the stacked padded rank at 32, leaves every member bit-identical in strict mode
    (fp32: 1e-6); two runs give the same bits in both modes."""
    ks = [4, 7, 1, 9]
    S, inits = mc.sbc.thinned(160, 150, 0.2, ks + [5], 8)
    c = mc.case("indep", S, ks, inits[:4], max_iter=6)
    base, _ = batch(prec, c, method)
    again, _ = batch(prec, c, method)
    same_bits(base, again)
    perm = [2, 0, 3, 1]
    tp, _ = batch(prec, c, method, ks=[ks[p] for p in perm], inits=[inits[p] for p in perm])
    t5, _ = batch(prec, c, method, ks=ks + [5], inits=inits)
    for b in range(4):
        for other in (tp[perm.index(b)], t5[b]):
            if pname == "f64":
                same_bits([other], [base[b]])
            else:
                assert relF(other["W"], base[b]["W"]) < 1e-6 and relF(other["H"], base[b]["H"]) < 1e-6
                assert other["n_iteration"] == base[b]["n_iteration"]


# ---- 6. stopping and frozen members ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("method", [1, 2])
def test_each_member_stops_where_its_solo_run_stops(pname, prec, tol, method):
    c = mc.stop_case()
    t, _ = batch(prec, c, method)
    its = []
    for b in range(len(c["ks"])):
        s = solo(prec, c, b, method)
        assert t[b]["n_iteration"] == s["n_iteration"] and t[b]["warning"] == s["warning"]
        check_member(t[b], s, tol if pname == "f64" else 1e-5, pname == "f64")
        if pname == "f64":
            check_member(t[b], oracle(c, b, method), tol, True)
        its.append(t[b]["n_iteration"])
    print("iterations", its)
    assert len(set(its)) >= 3 and max(its) == c["max_iter"] and min(its) < c["max_iter"], its


@pytest.mark.parametrize("method", [1, 2])
def test_frozen_members_do_not_move_bit_for_bit(method):
    """Strict mode, stacked padded rank 16 = every member's own: each member ends with the bits of its solo run -- the ones that stopped
    early sat frozen while the others went on."""
    c = mc.frozen_case()
    t, _ = batch(_lib.PREC_F64, c, method)
    its = [o["n_iteration"] for o in t]
    assert min(its) < max(its), its
    for b in range(len(c["ks"])):
        s = solo(_lib.PREC_F64, c, b, method)
        assert s["n_iteration"] == its[b] and s["warning"] == t[b]["warning"]
        same_bits([t[b]], [s], keys=("W", "H", "average_epoch"))
    short, _ = batch(_lib.PREC_F64, dict(c, max_iter=min(its)), method)
    first = int(np.argmin(its))
    same_bits([short[first]], [t[first]], keys=("W", "H"))


@pytest.mark.parametrize("method", [1, 2])
def test_the_mask_shrinks_with_the_active_members(method):
    """[8, 8, 8, 8]: two tile pairs while all run; the members still active in the last iteration decide the last half-step's mask."""
    c = mc.mask_case()
    one, i1 = batch(_lib.PREC_F64, dict(c, max_iter=1), method)
    assert i1["sp_gram_batch_pairs"] == 2
    t, info = batch(_lib.PREC_F64, c, method)
    its = [o["n_iteration"] for o in t]
    active = [v == max(its) for v in its]
    print("iterations", its)
    assert info["sp_gram_batch_pairs"] == len(mc.tile_pairs(c["ks"], active)[0]) == 1, (its, info)
    for b in range(4):
        assert its[b] == solo(_lib.PREC_F64, c, b, method)["n_iteration"]


# ---- 7. one launch per phase -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("B", [1, 3, 8])
def test_one_launch_per_phase(pname, prec, tol, B):
    ks = [8] * B
    S, inits = mc.sbc.thinned(200, 150, 0.2, ks, 4)
    T = 6
    c = mc.case("phase", S, ks, inits, max_iter=T)
    for limit_slots in (0, 60):
        t, info = batch(prec, c, 1, prof=True, limit=limit_slots * mc.goff_of(ks)[-1] * 8)
        p = info["prof"]
        ntr = len(t[0]["mse_error"])
        assert ntr == 4  # iterations 0, 2, 4 and the closing entry
        ch = [len(mc.gram_chunks_of_slot(ptr, mc.goff_of(ks)[-1], limit_slots * mc.goff_of(ks)[-1] * 8)) for ptr in (sc.transpose_csc(S)[0], S[0])]
        assert (ch == [1, 1]) == (limit_slots == 0) and info["sp_gram_chunks"] == ch[1]
        assert p["spmm_h"][1] == T and p["spmm_w"][1] == T, p
        assert p["sp_gram"][1] == T * (ch[0] + ch[1]), p            # one Gram scope per half-step and chunk, whatever B is
        assert p["sweep_w"][1] == T * ch[0] and p["sweep_h"][1] == T * ch[1], p
        assert p["sp_batch_errors"][1] == ntr, p
        for nm in ("sp_errors", "batch_errors", "errors", "gram", "xprod_h", "xprod_w"):
            assert p[nm][1] == 0, (nm, p)


# ---- 8. the hold-out set -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,prec,tol", MODES)
def test_holdout_handle_is_the_upload_of_the_training_entries(pname, prec, tol):
    ks = [3, 5, 2]
    S, inits = mc.sbc.thinned(150, 130, 0.3, ks, 61)
    T, (hptr, hidx), hval = mc.held_out(S, 0.15, 5)
    c = mc.case("ho", S, ks, inits)
    with handle(prec) as h, handle(prec) as g:
        h.set_matrix_csc_missing_batch(*S, holdout=(hptr, hidx))
        g.set_matrix_csc_missing(*T)
        assert h.matrix_info() == g.matrix_info()
        for key in ("matrix_nnz", "matrix_bytes", "matrix_absent_missing"):
            assert h.get_info(key) == g.get_info(key), key
        assert h.get_info("sparse_batch") == 1 and g.get_info("sparse_batch") == 0
        assert h.get_info("matrix_holdout") == hidx.size and g.get_info("matrix_holdout") == -1
        with pytest.raises(_lib.NnlmError) as e:
            g.holdout_errors()  # (a set on another handle does not help this one)
        assert e.value.code == ERR_ARG
        res = []
        for x in (h, g):
            x.set_factors(ks[1], *inits[1])
            r = x.run(*run_args(c, 1))
            r["W"], r["H"] = x.get_factors()
            res.append(r)
        same_bits([res[0]], [res[1]])
        mse, mkl = h.holdout_errors()  # solo factors: one value
        A = sc.densify(S, "missing")
        check_sums(dict(W=res[0]["W"], H=res[0]["H"], holdout_mse=mse[0], holdout_mkl=mkl[0]), A, hptr, hidx, pname == "f64")
    # the batch on it: members = the batch on the plain training upload's door, held-out sums = numpy's on the returned factors
    t, info = batch(prec, c, 1, holdout=(hptr, hidx))
    u, _ = batch(prec, dict(c, S=T), 1)
    same_bits(t, u)
    for b in range(len(ks)):
        check_sums(dict(W=t[b]["W"], H=t[b]["H"], holdout_mse=info["holdout"][0][b], holdout_mkl=info["holdout"][1][b]), A, hptr, hidx, pname == "f64")


def check_sums(o, A, ptr, idx, strict):
    want = cv.numpy_holdout_errors(A, ptr, idx, o["W"], o["H"])
    for got, w in zip((o["holdout_mse"], o["holdout_mkl"]), want):
        assert abs(got - w) <= (1e-12 if strict else 1e-3) * abs(w), (got, w)


def test_empty_and_absent_holdout_sets():
    ks = [2, 3]
    S, inits = mc.sbc.thinned(60, 50, 0.3, ks, 2)
    c = mc.case("empty", S, ks, inits, max_iter=2)
    _, info = batch(_lib.PREC_F64, c, 1, holdout=(np.zeros(51, dtype=np.int64), np.zeros(0, dtype=np.int32)))
    assert np.isnan(info["holdout"][0]).all() and np.isnan(info["holdout"][1]).all()
    with handle(_lib.PREC_F64) as h:
        h.set_matrix_csc_missing_batch(*S, holdout=(np.zeros(51, dtype=np.int64), np.zeros(0, dtype=np.int32)))
        assert h.get_info("matrix_holdout") == 0 and h.get_info("matrix_nnz") == S[1].size
        h.set_matrix_csc_missing_batch(*S)
        assert h.get_info("matrix_holdout") == -1 and h.get_info("sparse_batch") == 1 and h.get_info("matrix_absent_missing") == 1
        h.set_factors_batch(ks, [w for w, _ in inits], [x for _, x in inits])
        with pytest.raises(_lib.NnlmError) as e:
            h.holdout_errors()
        assert e.value.code == ERR_ARG
    out = _lib.c_nnmf_csc_missing_batch(*S, ks, [w for w, _ in inits], [x for _, x in inits], *run_args(c, 1)[:4], 1, *run_args(c, 1)[4:])
    assert all(np.isnan(o["holdout_mse"]) and np.isnan(o["holdout_mkl"]) for o in out)


def test_bad_patterns_are_refused_by_the_library():
    S = sc.rand_csc(40, 30, 0.3, np.random.default_rng(1))
    ptr, idx = S[0], S[1]
    P = sc.pattern_of(S)
    i, j = (int(v[0]) for v in np.nonzero(~P))
    hp = np.zeros(31, dtype=np.int64)
    hp[j + 1:] = 1
    with handle(_lib.PREC_F64) as h:
        def refused(holdout, words):
            with pytest.raises(_lib.NnlmError) as e:
                h.set_matrix_csc_missing_batch(*S, holdout=holdout)
            assert e.value.code == ERR_ARG and words in str(e.value), str(e.value)
        refused((hp, np.array([i], dtype=np.int32)), "(row %d, column %d) is not a stored entry" % (i, j))
        refused((ptr, idx), "every stored entry is held out")
        rows = idx[ptr[0]:ptr[1]]
        hp2 = np.zeros(31, dtype=np.int64)
        hp2[1:] = 2
        refused((hp2, np.array([rows[1], rows[0]], dtype=np.int32)), "not strictly increasing")
        hp3 = hp2.copy()
        hp3[5] = 1
        refused((hp3, rows[:2].copy()), "decreases at column")


# ---- 9. the API --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname", ["f64", "f32"])
def test_nnmf_cv_names_the_planted_rank(monkeypatch, pname):
    monkeypatch.setenv("NNLM_PRECISION", pname)
    S, n, m = mc.planted()
    r = api.nnmf_cv(sc.Csc(S), mc.PLANTED_KS, holdout=0.15, rng=np.random.default_rng(mc.PLANTED_SEED), sparse_batch="missing", **mc.PLANTED_OPTS)
    print("held-out MSE", r["holdout_mse"])
    assert r["k"][r["best"]] == 3
    _, pos, _ = mc.planted_holdout()
    _, (hptr, hidx), _ = mc.split(S, pos)
    assert np.array_equal(r["holdout"]["indptr"], hptr) and np.array_equal(r["holdout"]["indices"], hidx)
    srt = np.sort(r["holdout_mse"])
    print("ratio to the runner-up %.3f (the oracle's: %.3f)" % (srt[0] / srt[1], mc.PLANTED_RATIO))


def test_two_batches_agree_with_one_and_the_one_shot_with_the_handle():
    S, n, m = mc.planted()
    A = sc.Csc(S)
    g = np.random.default_rng(3)
    init = [dict(W=g.random((n, k)), H=g.random((k, m))) for k in range(1, 13)]
    opts = dict(max_iter=10, rel_tol=1e-4, alpha=[0.01, 0, 0], beta=[0.01, 0, 0])
    two = api.nnmf_cv(A, list(range(1, 13)), holdout=0.15, rng=np.random.default_rng(1), init=init, sparse_batch="missing", **opts)
    one = api.nnmf_cv(A, list(range(1, 11)), holdout=two["holdout"], init=init[:10], sparse_batch="missing", **opts)
    assert np.array_equal(one["holdout"]["indices"], two["holdout"]["indices"])
    for b in range(10):
        for key in ("W", "H", "mse", "target_loss", "average_epochs"):
            assert np.array_equal(two["fits"][b][key], one["fits"][b][key]), (b, key)
        assert two["holdout_mse"][b] == one["holdout_mse"][b] and two["holdout_mkl"][b] == one["holdout_mkl"][b]
    assert np.all(np.isfinite(two["holdout_mse"][10:]))
    # the one-shot entry = the resident-handle route (members 1 .. 10)
    ho = (two["holdout"]["indptr"], two["holdout"]["indices"])
    ks = list(range(1, 11))
    out = _lib.c_nnmf_csc_missing_batch(*S, ks, [x["W"] for x in init[:10]], [x["H"] for x in init[:10]], opts["alpha"], opts["beta"], 10, 1e-4, 1,
                                        0, True, 50, 1e-9, 1, 2, holdout=ho)
    for b in range(10):
        assert np.array_equal(out[b]["W"], one["fits"][b]["W"]) and np.array_equal(out[b]["H"], one["fits"][b]["H"])
        assert out[b]["holdout_mse"] == one["holdout_mse"][b]
    # api.nnmf_batch: member b = nnmf(absent = 'missing') on the same A with the generator in the state member b found it
    res, best = api.nnmf_batch(A, [2, 3], nrun=2, rng=np.random.default_rng(17), sparse_batch="missing", **opts)
    g = np.random.default_rng(17)
    for b, k in enumerate([2, 2, 3, 3]):
        s = api.nnmf(A, k, rng=g, absent="missing", **opts)
        assert relF(res[b]["W"], s["W"]) < 1e-10 and relF(res[b]["H"], s["H"]) < 1e-10 and res[b]["n_iteration"] == s["n_iteration"]
        assert np.array_equal(res[b]["average_epochs"], s["average_epochs"])
    assert best == int(np.argmin([r["target_loss"][-1] for r in res]))


def test_refusals_under_the_door():
    rng = np.random.default_rng(0)
    S = sc.rand_csc(60, 50, 0.3, rng)
    W, H = [rng.random((60, 2)), rng.random((60, 3))], [rng.random((2, 50)), rng.random((3, 50))]

    def code(fn):
        with pytest.raises(_lib.NnlmError) as e:
            fn()
        return e.value.code

    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
        h.set_matrix_csc_missing_batch(*S)
        h.set_factors_batch([2, 3], W, H)
        for method in (3, 4):  # KL loss
            assert code(lambda: h.run_batch(Z3, Z3, 3, -1.0, 0, True, 1, 1e-9, method, 1)) == ERR_UNSUPPORTED
        big = [rng.random((60, 33)), rng.random((60, 32))], [rng.random((33, 50)), rng.random((32, 50))]
        assert code(lambda: h.set_factors_batch([33, 32], *big)) == ERR_UNSUPPORTED  # a rank sum of 65
        assert code(lambda: h.comm_init(None, 0, 2)) == ERR_UNSUPPORTED
        h.set_factors_batch([2, 3], W, H)
        h.run_batch(Z3, Z3, 2, -1.0, 0, True, 5, 1e-9, 1, 1)
        # the other sparse entries keep their refusals
        for load in (h.set_matrix_csc, h.set_matrix_csc_kl, h.set_matrix_csc_missing):
            load(*S)
            assert code(lambda: h.set_factors_batch([2, 3], W, H)) == ERR_UNSUPPORTED
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:  # a communicator first: the loader refuses
        h.comm_init(None, 0, 2)
        assert code(lambda: h.set_matrix_csc_missing_batch(*S)) == ERR_UNSUPPORTED
    assert code(lambda: _lib.c_nnmf_csc_missing_batch(*S, [2, 3], W, H, Z3, Z3, 3, -1.0, 1, 0, True, 1, 1e-9, 3, 1)) == ERR_UNSUPPORTED
    assert code(lambda: _lib.c_nnmf_csc_missing_batch(*S, [40, 25], None, None, Z3, Z3, 3, -1.0, 1, 0, True, 1, 1e-9, 1, 1)) == ERR_UNSUPPORTED
