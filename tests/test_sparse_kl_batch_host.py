"""Batched KL factorisation on a sparse count matrix, host side (no GPU): the two ABI exports, the refusals of the Python layer that are
raised before the library is called, and the conditions on the cases of tests/sparse_kl_batch_cases.py that
tests/test_gpu_sparse_kl_batch.py compares with the oracle -- each is shown well posed from the oracle alone, by the conditions of
tests/test_sparse_kl_host.py (no rounding dust carried into the next half-step, a 1e-13 perturbation of the start moves the oracle's
result by less than 1e-11 and no sweep count, SCD whole runs use one inner sweep).  No skip rule."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_cases as sc  # noqa: E402
import sparse_kl_cases as kc  # noqa: E402
import sparse_kl_batch_cases as kb  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402
from oracle import ref  # noqa: E402

ERR_ARG, ERR_UNSUPPORTED = 1, 5


def small():
    c = kc.count_case(40, 30, 3, 0.3, 5)
    return c, sc.Csc(c["S"])


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------
def test_abi_exports():
    hdr = open(os.path.join(ROOT, "include", "nnlm_mi355x.h")).read()
    lib = _lib.load()
    assert lib.nnlm_abi_version() == 1 and "#define NNLM_ABI_VERSION 1" in hdr
    for name, like in (("nnlm_set_matrix_csc_kl_batch", "nnlm_set_matrix_csc_kl"), ("nnlm_c_nnmf_csc_kl_batch", "nnlm_c_nnmf_csc_batch")):
        assert name in _lib.EXPORTS and ("int " + name + "(") in hdr and hasattr(lib, name)
        assert getattr(lib, name).argtypes == getattr(lib, like).argtypes
    for key in ("sparse_kl_batch", "sparse_kl_batch_form_w", "sparse_kl_batch_form_h", "sparse_kl_batch_group"):
        assert '"' + key + '"' in hdr
    assert callable(_lib.c_nnmf_csc_kl_batch) and callable(_lib.Handle.set_matrix_csc_kl_batch)


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------------
def code_of(fn):
    with pytest.raises(_lib.NnlmError) as ei:
        fn()
    return ei.value.code, str(ei.value)


def test_refusals_before_the_library_is_called(monkeypatch):
    c, S = small()
    A = kc.dense_of(c)
    for name in ("c_nnmf_csc_kl_batch", "c_nnmf_csc_batch", "c_nnmf_batch", "c_nnmf_csc_missing_batch"):
        monkeypatch.setattr(_lib, name, lambda *a, **kw: pytest.fail("the library was called"))
    kl = dict(loss="mkl", sparse_batch="kl")
    assert code_of(lambda: api.nnmf_batch(A, [2, 3], **kl))[0] == ERR_UNSUPPORTED  # a dense A
    assert code_of(lambda: api.nnmf_batch(A, [2, 3], loss="mse", sparse_batch="kl"))[0] == ERR_UNSUPPORTED
    assert code_of(lambda: api.nnmf_batch(S, [2, 3], absent="missing", **kl))[0] == ERR_UNSUPPORTED
    assert code_of(lambda: api.nnmf_batch(S, [2, 3], mask={"W": np.ones((40, 2), dtype=bool)}, **kl))[0] == ERR_UNSUPPORTED
    assert code_of(lambda: api.nnmf_batch(S, [2], init=[{"W0": np.ones((40, 1))}], **kl))[0] == ERR_UNSUPPORTED
    assert code_of(lambda: api.nnmf_batch(S, [30, 35], check_k=False, **kl))[0] == ERR_UNSUPPORTED  # the ranks sum to 65
    for bad in ("KL", "mkl", "zero", ""):
        assert code_of(lambda: api.nnmf_batch(S, [2, 3], loss="mkl", sparse_batch=bad))[0] == ERR_ARG
        assert code_of(lambda: api.nnmf_cv(S, [2, 3], sparse_batch=bad))[0] == ERR_ARG
    # loss = 'mkl' without the door: today's message, whatever else the call says
    old = "nnmf_batch: loss = 'mkl' (KL) is not supported by the batched factorisation: square loss only"
    for kw in ({}, {"sparse_batch": True}, {"sparse_batch": "missing"}, {"sparse_batch": False}):
        code, msg = code_of(lambda: api.nnmf_batch(S, [2, 3], loss="mkl", **kw))
        assert code == ERR_UNSUPPORTED and msg.endswith(old), msg
    assert code_of(lambda: api.nnmf_batch(A, [2, 3], loss="mkl"))[1].endswith(old)
    # nnmf_cv has no such door
    for kw in ({}, {"loss": "mkl"}, {"loss": "mse"}):
        assert code_of(lambda: api.nnmf_cv(S, [2, 3], sparse_batch="kl", **kw))[0] == ERR_UNSUPPORTED
    assert code_of(lambda: api.nnmf_cv(A, [2, 3], sparse_batch="kl"))[0] == ERR_UNSUPPORTED
    # a negative stored value: nnmf(sparse_kl = True)'s refusal
    ptr, idx, val, shp = c["S"]
    v = val.copy()
    v[2] = -1.0
    with pytest.raises(api.NnlmStop, match="negative"):
        api.nnmf_batch(sc.Csc((ptr, idx, v, shp)), [2, 3], **kl)


def test_the_door_routes_to_the_new_entry(monkeypatch):
    c, S = small()
    n, m = S.shape
    called = []

    def fake(name):
        def f(indptr, indices, data, shape, ks, W, H, *a, **kw):
            called.append((name, a[9]))  # (the method code)
            return [dict(W=np.ones((n, k)), H=np.ones((k, m)), mse_error=[0.0], mkl_error=[0.0], target_error=[float(b)], average_epoch=[1.0],
                         n_iteration=1) for b, k in enumerate(ks)]
        return f

    for name in ("c_nnmf_csc_kl_batch", "c_nnmf_csc_batch"):
        monkeypatch.setattr(_lib, name, fake(name))
    res, best = api.nnmf_batch(S, [2, 3], nrun=2, loss="mkl", sparse_batch="kl", rng=np.random.default_rng(0))
    assert len(res) == 4 and best == 0 and all(r["options"]["loss"] == "mkl" for r in res)
    api.nnmf_batch(S, [2], loss="mkl", method="lee", sparse_batch="kl")
    api.nnmf_batch(S, [2], loss="mse", sparse_batch="kl")  # (square loss through this door: sparse_batch = True)
    api.nnmf_batch(S, [2], sparse_batch=True)
    assert called == [("c_nnmf_csc_kl_batch", 3), ("c_nnmf_csc_kl_batch", 4), ("c_nnmf_csc_batch", 1), ("c_nnmf_csc_batch", 1)]


# ---- the cases are well posed (the oracle alone) -------------------------------------------------------------------------------------------
ORACLE = kb.oracle_cases()


@pytest.mark.parametrize("i", range(len(ORACLE)), ids=["%s m%d i%d" % (c["name"], me, inn) for c, me, inn in ORACLE])
def test_oracle_cases_are_well_posed(i):
    c, method, inner = ORACLE[i]
    assert inner == 1 if method == 3 else inner > 1  # SCD whole runs use one inner sweep; Lee runs several
    _, _, val, _ = c["S"]
    assert np.all(val > 0) and np.all(val == np.rint(val))  # counts, zeros dropped from the structure
    A = sc.densify(c["S"], "zero")
    assert sum(c["ks"]) <= 64 and len(set(c["ks"])) == len(c["ks"]) >= 3  # a rank sweep: distinct ranks
    for b, k in enumerate(c["ks"]):
        assert c["inits"][b][0].shape == (A.shape[0], k) and c["inits"][b][1].shape == (k, A.shape[1])
        ok, why = kb.well_posed(ref, A, k, c["inits"][b], method, inner)
        assert ok, (c["name"], method, inner, b, why)
        o = kb.oracle_run(ref, A, k, c["inits"][b], method, inner)
        assert o["n_iteration"] == kb.ORACLE_ITERS and np.all(np.diff(o["target_error"]) < 0)


def test_fuzz_table_is_what_the_oracle_says():
    assert len(kb.FUZZ_SEEDS) == 12 and sorted(kb.FUZZ_WELL_POSED) == sorted(kb.FUZZ_SEEDS)
    assert [kb.fuzz_seed(i) for i in (0, 11, 12, 15)] == [kb.FUZZ_SEEDS[0], kb.FUZZ_SEEDS[11], 112, 115]
    assert {s % len(kb.FUZZ_FAMILIES) for s in kb.FUZZ_SEEDS} == set(range(len(kb.FUZZ_FAMILIES)))  # every pattern family
    methods = set()
    for seed in kb.FUZZ_SEEDS:
        c = kb.fuzz_case(seed)
        assert 1 <= len(c["ks"]) and sum(c["ks"]) <= 64 and min(c["ks"]) >= 1
        assert c["inner"] == 1 or c["method"] == 4
        methods.add(c["method"])
        A = sc.densify(c["S"], "zero")
        ok = [b for b, k in enumerate(c["ks"])
              if kb.well_posed(ref, A, k, c["inits"][b], c["method"], c["inner"], c["max_iter"], (c["alpha"], c["beta"]))[0]]
        assert set(kb.FUZZ_WELL_POSED[seed]) <= set(ok), (seed, ok)  # (what the table lists is well posed)
        assert kb.FUZZ_WELL_POSED[seed], seed  # no seed of the twelve goes without the oracle
    assert methods == {3, 4}


def test_line_cases_take_both_forms():
    cases = kb.line_cases()
    for c, tr in zip(cases[:2], (False, True)):
        assert kc.line_forms(c["S"]) == ((3, 1) if tr else (1, 3))  # the designed lines sit on both sides of the threshold
    for c, tr in zip(cases[2:4], (False, True)):
        assert kc.line_forms(c["S"])[0 if tr else 1] & kc.FORM_LONG
    assert len(cases) == 8 and all(sum(c["ks"]) <= 64 for c in cases)
