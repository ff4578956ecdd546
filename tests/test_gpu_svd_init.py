"""nnlm_svd / nnlm_get_svd / nnlm_set_factors_nndsvd(_batch) and the Python routes over them on the MI355X, in both arithmetic modes, each
case dense and as CSC, against the numpy restatement of tests/svd_init_cases.py ON THE SAME sketch matrix (not against LAPACK: see
test_svd_init_host.py).  Run with `pytest -m gpu`.

Bars.  Strict mode: 1e-10, the project's strict bar.  fp32-operand mode: svd_init_cases.F32_BAR = 4.6e-6, ten times the deviation that
rounding A and every cross-product operand to 22 bits causes in the restatement (measured on the CPU, test_svd_init_host.py).  Both are
on max |X - Xref| / max |Xref|.  U U^T = I on the kept directions holds to 1e-12 in both modes (the second orth pass works on the fp64
masters).  The nndsvda fill is the mean of the RESIDENT values: A.mean() to 1e-14 in the strict mode; in the fp32-operand mode the
resident matrix is the fp32 rounding of A, and the fill is the fp64 mean of that to 1e-14."""
import os
import sys

import numpy as np
import pytest

try:  # (ahead of the library, as in test_gpu_device_io.py: the tensor library brings its own HIP runtime and has to load it first)
    import torch
except ImportError:
    torch = None

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import relF  # noqa: E402
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402
import svd_init_cases as S  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = [("f64", _lib.PREC_F64, 1e-10), ("f32", _lib.PREC_F32, S.F32_BAR)]
FORMS = ["dense", "csc"]
ERR_ARG, ERR_UNSUPPORTED = 1, 5
Z3 = [0.0, 0.0, 0.0]
CASES = S.all_cases()
IDS = [c.name for c in CASES]


@pytest.fixture(autouse=True)
def _default_precision(monkeypatch):
    monkeypatch.delenv("NNLM_PRECISION", raising=False)


def load(h, c, form, door="set_matrix_csc"):
    if form == "dense":
        h.set_matrix(c.A)
    else:
        getattr(h, door)(*S.csc_of(c.A))


_runs = {}


def gpu(c, prec, form):
    """One decomposition and both starts of case c per mode and form, shared by the tests below."""
    key = (c.name, prec, form)
    if key not in _runs:
        with nnlm_amd.Handle(0, prec) as h:
            load(h, c, form)
            h.svd(c.l, 2, c.omega)
            r = dict(kept=int(h.get_info("svd_kept")), width=int(h.get_info("svd_width")))
            r["U"], r["s"], r["Vt"] = h.get_svd(c.l)
            h.set_factors_nndsvd(c.k, "nndsvd")
            r["W"], r["H"] = h.get_factors()
            h.set_factors_nndsvd(c.k, "nndsvda")
            r["Wa"], r["Ha"] = h.get_factors()
        _runs[key] = r
    return _runs[key]


def code(f):
    with pytest.raises(_lib.NnlmError) as e:
        f()
    return e.value.code, str(e.value)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_svd_equals_the_restatement(c, pname, prec, tol, form):
    r, ref = gpu(c, prec, form), S.reference(c)
    k = c.k
    ds = np.abs(r["s"][:k] - ref["s"][:k]).max() / ref["s"][0]
    U, Vt = S.align(r["U"].T[:k], r["Vt"][:k], ref["U"][:k], ref["Vt"][:k])
    dv = S.deviation(U, Vt, ref["U"][:k], ref["Vt"][:k])
    kept = r["kept"]
    Uk = r["U"].T[:kept]
    do = np.abs(Uk @ Uk.T - np.eye(kept)).max()
    print("%s %s %s: sigma %.2e vectors %.2e orthonormality %.2e kept %d / %d (restatement %d)" % (c.name, pname, form, ds, dv, do, kept, c.l, ref["kept"]))
    assert r["width"] == c.l and np.all(np.diff(r["s"]) <= 0) and np.all(r["s"] >= 0)
    assert ds <= tol and dv <= tol
    assert do <= 1e-12
    if pname == "f64":
        assert kept == ref["kept"]
    assert k <= kept <= c.l


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_nndsvd_equals_the_restatement(c, pname, prec, tol, form):
    r, ref = gpu(c, prec, form), S.reference(c)
    W, H, k = r["W"], r["H"], c.k
    d = S.deviation(W, H, ref["W"], ref["H"])
    print("%s %s %s: nndsvd deviation %.2e (bar %.1e)" % (c.name, pname, form, d, tol))
    assert W.shape == (c.n, k) and H.shape == (k, c.m) and (W >= 0).all() and (H >= 0).all()
    assert d <= tol
    # exact zeros where the restatement has them (entries of the side not taken, beyond the reach of rounding)
    away_u, away_v = np.abs(ref["U"][:k].T) > 100 * tol, np.abs(ref["Vt"][:k]) > 100 * tol
    assert not W[(ref["W"] == 0) & away_u].any() and not H[(ref["H"] == 0) & away_v].any()
    if c.noise and pname == "f64":  # (a noisy triplet has entries of both signs: the check above is not empty)
        assert ((ref["W"] == 0) & away_u).any() and ((ref["H"] == 0) & away_v).any()
    # nndsvda: the same start with every exact zero replaced by mean(A) of the resident values
    resident = c.A if pname == "f64" else c.A.astype(np.float32).astype(np.float64)
    fills = np.unique(np.concatenate([r["Wa"][W == 0], r["Ha"][H == 0]]))
    assert fills.size == 1 and abs(fills[0] - resident.mean()) <= 1e-14 * resident.mean()
    assert np.array_equal(r["Wa"], np.where(W == 0, fills[0], W)) and np.array_equal(r["Ha"], np.where(H == 0, fills[0], H))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("c", [c for c in CASES if not c.noise and c.blocks == c.k], ids=lambda c: c.name)
def test_noise_free_blocks_are_reproduced_and_a_run_stops_at_once(c, pname, prec, tol, form):
    r = gpu(c, prec, form)
    d = np.abs(r["W"] @ r["H"] - c.A).max() / np.abs(c.A).max()
    assert S.deviation(r["W"], r["H"], c.Wc, c.Hc) <= tol and d <= 4 * tol, d
    with nnlm_amd.Handle(0, prec) as h:
        load(h, c, form)
        h.svd(c.l, 2, c.omega)
        h.set_factors_nndsvd(c.k, 0)
        t = h.run(Z3, Z3, 50, 1e-4, 0, True, 50, 1e-9, 1, 1)
    print("%s %s %s: W H - A %.2e, run: %d iterations, mse %s" % (c.name, pname, form, d, t["n_iteration"], t["mse_error"]))
    # The start is a fixed point up to rounding: the error is at the mode's rounding level at the first trace point and at the last, the
    # run ends by its own rule well inside max.iter and without the warning.  WHICH trace point ends it is not a property of the start:
    # the rule compares two rounding-level errors (strict: 1e-35, fp32-operand mode: 5e-18), and a sweep that ends on inner.rel.tol = 1e-9
    # may leave the factors off by 1e-10 for an iteration (measured: 2.96e-20 at the second trace point of 300 x 200, k 60, CSC, strict,
    # back at 1.3e-35 at the third).  Measured iterations: strict 2 (4 in that case), fp32-operand mode 3 .. 8; a start that merely
    # converged would need far more than the 10 allowed here.
    level = (4 * tol * np.abs(c.A).max()) ** 2
    assert not t["warning"] and t["n_iteration"] <= 10
    assert t["mse_error"][0] <= level and t["mse_error"][-1] <= level
    assert t["mse_error"].max() <= max(level, (10 * 1e-9 * np.abs(c.A).max()) ** 2)


_wide = {}


@pytest.mark.parametrize("rot", [-1, 16, 8, 0])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("pname,prec,tol", MODES)
def test_a_wide_sketch_through_every_form_of_the_rotation(pname, prec, tol, form, rot):
    """l = 150 (padded to 160): 32 columns of X and all of T need 245 KB, so the width's own form (rot = -1) is the 32-column tile with
    T's rows in chunks of 96 under the 160 KB LDS grant; the hook then puts the same decomposition through the 16- and 8-column tiles
    (112 and 120 rows of T at a time) and the out-of-place kernel, the forms of widths beyond 512, 848 and 1280.  Every form against the
    restatement, and all of them bit for bit the same."""
    c = S.wide_case()
    ref = S.reference(c, 1)
    _lib.debug_set_svd_rotate(rot)
    try:
        with nnlm_amd.Handle(0, prec) as h:
            load(h, c, form)
            h.svd(c.l, 1, c.omega)
            ran, kept = int(h.get_info("svd_rotate_form")), int(h.get_info("svd_kept"))
            U, s, Vt = h.get_svd(c.l)
            h.set_factors_nndsvd(c.k, "nndsvd")
            W, H = h.get_factors()
    finally:
        _lib.debug_set_svd_rotate(-1)
    assert ran == (32 if rot == -1 else rot) and kept == c.l
    k = c.k
    ds = np.abs(s[:k] - ref["s"][:k]).max() / ref["s"][0]
    Ua, Va = S.align(U.T[:k], Vt[:k], ref["U"][:k], ref["Vt"][:k])
    dv, dw = S.deviation(Ua, Va, ref["U"][:k], ref["Vt"][:k]), S.deviation(W, H, ref["W"], ref["H"])
    do = np.abs(U.T @ U - np.eye(c.l)).max()
    print("wide %s %s form %d: sigma %.2e vectors %.2e nndsvd %.2e orthonormality %.2e" % (pname, form, ran, ds, dv, dw, do))
    assert ds <= tol and dv <= tol and dw <= tol and do <= 1e-12
    first = _wide.setdefault((pname, form), (U, s, Vt, W, H))
    for a, b in zip(first, (U, s, Vt, W, H)):
        assert np.array_equal(a, b)


def test_the_rotation_hook_refuses_other_values():
    for v in (-2, 4, 64):
        assert code(lambda: _lib.debug_set_svd_rotate(v))[0] == ERR_ARG


@pytest.mark.parametrize("form,door", [("dense", None), ("csc", "set_matrix_csc_batch")])
@pytest.mark.parametrize("pname,prec,tol", MODES)
def test_batch_members_are_the_leading_components_of_one_svd(pname, prec, tol, form, door):
    c, ks = S.case("257x129_k17", 1e-4), [3, 6, 17]
    args = (Z3, Z3, 8, -1.0, 0, True, 50, 1e-9, 1, 2)
    with nnlm_amd.Handle(0, prec) as h:
        load(h, c, form, door)
        h.svd(c.l, 2, c.omega)
        h.set_factors_nndsvd(17, "nndsvd")
        W17, H17 = h.get_factors()
        h.set_factors_nndsvd_batch(ks, "nndsvd")
        start = h.get_factors_batch()
        for (W, H), k in zip(start, ks):  # bit for bit: component j depends on triplet j alone
            assert np.array_equal(W, W17[:, :k]) and np.array_equal(H, H17[:k])
        tb = h.run_batch(*args)
        fb = h.get_factors_batch()
        for b, k in enumerate(ks):
            h.set_factors_nndsvd(k, "nndsvd")
            ts = h.run(*args)
            Ws, Hs = h.get_factors()
            bar = tol if pname == "f64" else 1e-5  # (test_gpu_batch.py's bars of a member against the same member alone)
            assert relF(fb[b][0], Ws) < bar and relF(fb[b][1], Hs) < bar, (relF(fb[b][0], Ws), relF(fb[b][1], Hs))
            assert tb[b]["n_iteration"] == ts["n_iteration"] and relF(tb[b]["mse_error"], ts["mse_error"]) < max(bar, 1e-10)
        assert code(lambda: h.set_factors_nndsvd_batch([3, c.l + 1], 0))[0] == ERR_ARG
        assert code(lambda: h.set_factors_nndsvd_batch([20, 20, 20, 20], 0))[0] == ERR_UNSUPPORTED  # (rank sum 80 > 64)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("pname,prec,tol", MODES)
def test_two_calls_give_identical_bits_and_the_handle_is_left_without_factors(pname, prec, tol, form):
    c = S.case("300x200_k60", 1e-4)  # (l = 70: the launches beyond rank 64)
    first = gpu(c, prec, form)
    with nnlm_amd.Handle(0, prec) as h:
        load(h, c, form)
        h.set_factors(5, np.ones((c.n, 5)), np.ones((5, c.m)))
        h.svd(c.l, 2, c.omega)
        U, s, Vt = h.get_svd(c.l)
        assert np.array_equal(U, first["U"]) and np.array_equal(s, first["s"]) and np.array_equal(Vt, first["Vt"])
        # no factors, as after set_matrix
        assert code(lambda: h.run(Z3, Z3, 2, -1.0, 0, True, 50, 1e-9, 1, 1))[0] == ERR_ARG
        assert code(lambda: h.half_step(1, Z3, 50, 1e-9, 1))[0] == ERR_ARG
        h.k = c.k
        assert code(lambda: h.get_factors())[0] == ERR_ARG
        # a new matrix drops the decomposition
        load(h, c, form)
        assert h.get_info("svd_width") == -1 and h.get_info("svd_kept") == -1
        assert code(lambda: h.set_factors_nndsvd(3, 0))[0] == ERR_ARG


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("pname,prec,tol", MODES)
@pytest.mark.parametrize("variant", ["nndsvd", "nndsvda"])
def test_the_state_is_that_of_set_factors(pname, prec, tol, form, variant):
    c = S.case("515x131_k50", 1e-4)
    with nnlm_amd.Handle(0, prec) as h, nnlm_amd.Handle(0, prec) as g:
        load(h, c, form)
        load(g, c, form)
        h.svd(c.l, 1, c.omega)
        h.set_factors_nndsvd(c.k, variant)
        W0, H0 = h.get_factors()
        g.set_factors(c.k, W0, H0)
        for which in (1, 0, 1):
            h.half_step(which, [0.0, 0.01, 0.0], 20, 1e-9, 1)
            g.half_step(which, [0.0, 0.01, 0.0], 20, 1e-9, 1)
        for a, b in zip(h.get_factors(), g.get_factors()):
            assert np.array_equal(a, b)
        assert h.errors()[0] == g.errors()[0]


@pytest.mark.parametrize("pname,prec,tol", MODES)
def test_device_ingest_gives_the_host_routes_bits(pname, prec, tol):
    assert torch is not None, "the device tensors of this test need torch"
    c = S.case("257x129_k17", 1e-4)
    dev = torch.device("cuda", 0)
    ptr, idx, val, shape = S.csc_of(c.A)
    with nnlm_amd.Handle(0, prec) as h:
        h.set_matrix_device(torch.from_numpy(np.ascontiguousarray(c.A)).to(dev))
        h.svd(c.l, 2, c.omega)
        for a, b in zip(h.get_svd(c.l), (gpu(c, prec, "dense")[x] for x in ("U", "s", "Vt"))):
            assert np.array_equal(a, b)
        h.set_matrix_sparse_device(torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev), torch.from_numpy(val).to(dev), shape)
        h.svd(c.l, 2, c.omega)
        for a, b in zip(h.get_svd(c.l), (gpu(c, prec, "csc")[x] for x in ("U", "s", "Vt"))):
            assert np.array_equal(a, b)


def test_refusals_by_code_and_message():
    c = S.case("150x90_k6")
    csc = S.csc_of(c.A)
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:
        assert code(lambda: h.set_factors_nndsvd(3, 0))[0] == ERR_ARG  # no matrix
        bad = c.A.copy()
        bad[7, 9] = np.nan
        h.set_matrix(bad)
        rc, msg = code(lambda: h.svd(c.l, 2, c.omega))
        assert rc == ERR_UNSUPPORTED and "missing" in msg
        ptr = np.zeros(c.m + 1, dtype=np.int64)
        ptr[1:] = 2
        h.set_matrix_holdout(c.A, ptr, np.array([3, 5], dtype=np.int32))
        rc, msg = code(lambda: h.svd(c.l, 2, c.omega))
        assert rc == ERR_UNSUPPORTED and "hold-out" in msg
        for door in ("set_matrix_csc_missing", "set_matrix_csc_missing_batch"):
            getattr(h, door)(*csc)
            rc, msg = code(lambda: h.svd(c.l, 2, c.omega))
            assert rc == ERR_UNSUPPORTED and "absent entries are missing" in msg
        h.set_matrix(c.A)
        for l in (0, min(c.n, c.m) + 1):
            rc, msg = code(lambda: h.svd(l, 2, np.zeros((max(l, 1), c.m))))
            assert rc == ERR_ARG and "min(n, m)" in msg
        om = c.omega.copy()
        om[2, 3] = np.inf
        rc, msg = code(lambda: h.svd(c.l, 2, om))
        assert rc == ERR_ARG and "not finite" in msg
        rc, msg = code(lambda: _lib._check(h._lib.nnlm_svd(h._h, c.l, 2, None), h._h))
        assert rc == ERR_ARG and "omega is NULL" in msg
        rc, msg = code(lambda: h.set_factors_nndsvd(3, 0))
        assert rc == ERR_ARG and "nnlm_svd first" in msg
        rc, msg = code(lambda: h.get_svd(3))
        assert rc == ERR_ARG
        h.svd(c.l, 0, c.omega)
        assert h.get_info("svd_width") == c.l
        rc, msg = code(lambda: h.set_factors_nndsvd(c.l + 1, 0))
        assert rc == ERR_ARG and "exceeds the sketch width" in msg
        assert code(lambda: h.set_factors_nndsvd(0, 0))[0] == ERR_ARG
        for v in (-1, 2):
            rc, msg = code(lambda: h.set_factors_nndsvd(3, v))
            assert rc == ERR_ARG and "variant" in msg
        assert code(lambda: h.get_svd(c.l + 1))[0] == ERR_ARG
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:  # a communicator (virtual rank)
        h.set_matrix(c.A)
        h.comm_init(None, 0, 2)
        rc, msg = code(lambda: h.svd(c.l, 2, c.omega))
        assert rc == ERR_UNSUPPORTED and "communicator" in msg


@pytest.mark.parametrize("sparse", [False, True])
def test_api_nnmf_with_a_string_init(sparse):
    c = S.case("150x90_k6", 1e-4)
    A = S.SparseCSC(c.A) if sparse else c.A
    opts = dict(max_iter=6, rel_tol=-1.0)
    r1 = api.nnmf(A, c.k, init="nndsvd", rng=np.random.default_rng(3), **opts)
    r2 = api.nnmf(A, c.k, init="nndsvd", rng=np.random.default_rng(3), **opts)
    assert np.array_equal(r1["W"], r2["W"]) and np.array_equal(r1["H"], r2["H"]) and np.array_equal(r1["mse"], r2["mse"])
    assert r1["options"]["init"] == "nndsvd"
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:  # the exported start through the init dict
        load(h, c, "csc" if sparse else "dense")
        h.svd(16, 2, api._svd_omega(16, c.m, np.random.default_rng(3)))
        U, s, Vt = h.get_svd(c.k)
        h.set_factors_nndsvd(c.k, "nndsvd")
        W0, H0 = h.get_factors()
    r3 = api.nnmf(A, c.k, init={"W": W0, "H": H0}, **opts)
    assert np.array_equal(r1["W"], r3["W"]) and np.array_equal(r1["H"], r3["H"]) and np.array_equal(r1["mse"], r3["mse"])
    Ut, st, Vtt = api.truncated_svd(A, c.k, rng=np.random.default_rng(3), precision="f64")
    assert np.array_equal(Ut, U) and np.array_equal(st, s) and np.array_equal(Vtt, Vt)
    ra = api.nnmf(A, c.k, init="nndsvda", method="lee", rng=np.random.default_rng(3), **opts)
    assert (ra["W"] > 0).all() and (ra["H"] > 0).all() and ra["mse"][-1] < ra["mse"][0]


@pytest.mark.parametrize("door", [None, True, "kl"])
def test_api_nnmf_batch_with_a_string_init(door):
    c = S.case("150x90_k6", 1e-4)
    A = c.A if door is None else S.SparseCSC(c.A)
    kw = {} if door is None else dict(sparse_batch=door)
    if door == "kl":
        kw.update(loss="mkl", trace=1)
    init = "nndsvda" if door == "kl" else "nndsvd"
    res, best = api.nnmf_batch(A, [3, 6], init=init, rng=np.random.default_rng(4), max_iter=6, rel_tol=-1.0, **kw)
    assert len(res) == 2 and res[0]["W"].shape == (c.n, 3) and res[1]["H"].shape == (6, c.m) and 0 <= best < 2
    assert all(np.isfinite(r["W"]).all() and np.isfinite(r["mse"]).all() for r in res)
    key = "mkl" if door == "kl" else "mse"
    assert res[1][key][-1] < res[0][key][-1] and all(r[key][-1] < r[key][0] for r in res)
    with nnlm_amd.Handle(0, _lib.PREC_F64) as h:  # one decomposition at the top rank for both members
        load(h, c, "dense" if door is None else "csc", "set_matrix_csc_kl_batch" if door == "kl" else "set_matrix_csc_batch")
        h.svd(16, 2, api._svd_omega(16, c.m, np.random.default_rng(4)))
        h.set_factors_nndsvd_batch([3, 6], init)
        if door == "kl":  # (R's default for KL loss: one inner sweep)
            h.run_batch(Z3, Z3, 6, -1.0, 0, True, 1, 1e-9, 3, 1)
        else:
            h.run_batch(Z3, Z3, 6, -1.0, 0, True, 50, 1e-9, 1, 2)
        for r, (W, H) in zip(res, h.get_factors_batch()):
            assert np.array_equal(r["W"], W) and np.array_equal(r["H"], H)


@pytest.mark.parametrize("pname,prec,tol", MODES)
def test_the_solo_kl_door_takes_svd_and_nndsvda(pname, prec, tol, monkeypatch):
    """nnlm_set_matrix_csc_kl: the decomposition is the plain sparse door's bit for bit, the nndsvda start has no zero, KL half-steps run
    from it, and api.nnmf(loss = 'mkl', sparse_kl = True, init = 'nndsvda') is that route."""
    c = S.case("150x90_k6", 1e-4)
    with nnlm_amd.Handle(0, prec) as h:
        load(h, c, "csc", "set_matrix_csc_kl")
        assert h.get_info("sparse_kl") == 1
        h.svd(c.l, 2, c.omega)
        for a, b in zip(h.get_svd(c.l), (gpu(c, prec, "csc")[x] for x in ("U", "s", "Vt"))):
            assert np.array_equal(a, b)
        h.set_factors_nndsvd(c.k, "nndsvda")
        W0, H0 = h.get_factors()
        assert np.array_equal(W0, gpu(c, prec, "csc")["Wa"]) and np.array_equal(H0, gpu(c, prec, "csc")["Ha"])
        assert (W0 > 0).all() and (H0 > 0).all()
        t = h.run(Z3, Z3, 6, -1.0, 0, True, 1, 1e-9, 3, 1)
        assert np.isfinite(t["mkl_error"]).all() and t["mkl_error"][-1] < t["mkl_error"][0]
    monkeypatch.setenv("NNLM_PRECISION", pname)
    opts = dict(loss="mkl", sparse_kl=True, max_iter=6, rel_tol=-1.0, trace=1)
    r = api.nnmf(S.SparseCSC(c.A), c.k, init="nndsvda", rng=np.random.default_rng(9), **opts)
    with nnlm_amd.Handle(0, prec) as h:
        load(h, c, "csc", "set_matrix_csc_kl")
        h.svd(16, 2, api._svd_omega(16, c.m, np.random.default_rng(9)))
        h.set_factors_nndsvd(c.k, "nndsvda")
        t = h.run(Z3, Z3, 6, -1.0, 0, True, 1, 1e-9, 3, 1)
        W, H = h.get_factors()
    assert np.array_equal(r["W"], W) and np.array_equal(r["H"], H) and np.array_equal(r["mkl"], t["mkl_error"])
    assert r["options"]["init"] == "nndsvda" and r["mkl"][-1] < r["mkl"][0]
