"""The batched factorisation on a sparse A without a GPU: the new exports, the argument checks of api.nnmf_batch(sparse_batch=True) --
raised before the library is touched --, one canonical CSC for all members, and the conditions on the boundary cases that
tests/test_gpu_sparse_batch.py runs."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from nnlm_amd import _lib, api  # noqa: E402
import sparse_cases as sc  # noqa: E402
import sparse_batch_cases as sbc  # noqa: E402

ERR_ARG, ERR_UNSUPPORTED = 1, 5


def duck(n=30, m=20, seed=0, density=0.4):
    return sc.Csc(sc.rand_csc(n, m, density, np.random.default_rng(seed)))


def fake_members(ks, W, H):
    return [dict(W=w, H=h, mse_error=np.ones(1), mkl_error=np.ones(1), target_error=np.full(1, float(len(ks) - b)), average_epoch=np.ones(1),
                 n_iteration=1, warning=False) for b, (w, h) in enumerate(zip(W, H))]


def test_the_four_new_exports_exist():
    hdr = open(os.path.join(ROOT, "include", "nnlm_mi355x.h")).read()
    for name in ("nnlm_set_matrix_csc_batch", "nnlm_c_nnmf_csc_batch"):
        assert name in _lib.EXPORTS and ("int " + name + "(") in hdr
    assert callable(_lib.c_nnmf_csc_batch) and callable(_lib.Handle.set_matrix_csc_batch)
    assert '"sparse_batch"' in hdr


@pytest.mark.parametrize("what", ["kl", "mask", "W0", "H0", "sum65", "missing"])
def test_unsupported_inputs_are_refused_under_the_door(what):
    A, k, kw = duck(), [2, 3], {}
    if what == "kl":
        kw["loss"] = "mkl"
    elif what == "mask":
        kw["mask"] = {"W": np.zeros((30, 2), dtype=bool)}
    elif what == "W0":
        kw["init"] = [{"W0": np.ones((30, 1))}, {}]
    elif what == "H0":
        kw["init"] = [{}, {"H0": np.ones((1, 20))}]
    elif what == "sum65":
        A, k = duck(80, 70), [33, 32]
    elif what == "missing":
        kw["absent"] = "missing"
    with pytest.raises(_lib.NnlmError) as e:
        api.nnmf_batch(A, k, sparse_batch=True, **kw)
    assert e.value.code == ERR_UNSUPPORTED
    assert "batch" in str(e.value)


def test_default_still_refuses_a_sparse_matrix():
    with pytest.raises(_lib.NnlmError) as e:
        api.nnmf_batch(duck(), [2, 3])
    assert e.value.code == ERR_UNSUPPORTED and "sparse" in str(e.value)
    with pytest.raises(_lib.NnlmError) as e:
        api.nnmf_batch(duck(), [2, 3], sparse_batch=False)
    assert e.value.code == ERR_UNSUPPORTED


def test_a_non_finite_stored_value_is_the_sparse_input_error():
    A = duck()
    A.data = A.data.copy()
    A.data[3] = np.nan
    with pytest.raises(api.NnlmStop) as solo:
        api._sparse_input(A, "A", "mse")
    with pytest.raises(api.NnlmStop) as batch:
        api.nnmf_batch(A, [2, 3], sparse_batch=True)
    assert str(batch.value) == str(solo.value)


def test_check_k_bound_is_the_smaller_dimension():
    with pytest.raises(api.NnlmStop):
        api.nnmf_batch(duck(30, 20), [2, 21], sparse_batch=True)


def test_a_dense_matrix_ignores_the_flag(monkeypatch):
    A = np.random.default_rng(1).random((30, 20))
    seen = []

    def fake_batch(A_, ks, W, H, *rest, callbacks=None):
        seen.append((A_, [w.copy() for w in W], rest))
        return fake_members(ks, W, H)

    def no_sparse_call(*a, **kw):
        raise AssertionError("a dense A must not reach c_nnmf_csc_batch")

    monkeypatch.setattr(_lib, "c_nnmf_batch", fake_batch)
    monkeypatch.setattr(_lib, "c_nnmf_csc_batch", no_sparse_call)
    r1, b1 = api.nnmf_batch(A, [2, 3], nrun=2, rng=np.random.default_rng(5), sparse_batch=True)
    r0, b0 = api.nnmf_batch(A, [2, 3], nrun=2, rng=np.random.default_rng(5))
    assert b1 == b0 and len(r1) == len(r0) == 4
    assert seen[0][0] is A and seen[1][0] is A and repr(seen[0][2]) == repr(seen[1][2])
    for w1, w0 in zip(seen[0][1], seen[1][1]):
        assert np.array_equal(w1, w0)


def test_the_matrix_is_canonicalised_once_for_all_members(monkeypatch):
    """One as_csc for the whole batch; every member and the C call see that one CSC (the arrays are handed on as they are)."""
    A = duck(30, 20, seed=2)
    made, seen = [], {}
    real = api.as_csc

    def counting(A_):
        made.append(real(A_))
        return made[-1]

    def fake_csc_batch(indptr, indices, data, shape, ks, W, H, *rest, callbacks=None):
        seen.update(indptr=indptr, indices=indices, data=data, shape=shape, W=W)
        return fake_members(ks, W, H)

    def no_dense_call(*a, **kw):
        raise AssertionError("a sparse A must not reach c_nnmf_batch")

    monkeypatch.setattr(api, "as_csc", counting)
    monkeypatch.setattr(_lib, "c_nnmf_csc_batch", fake_csc_batch)
    monkeypatch.setattr(_lib, "c_nnmf_batch", no_dense_call)
    res, best = api.nnmf_batch(A, [2, 3], nrun=3, rng=np.random.default_rng(0), sparse_batch=True)
    assert len(made) == 1
    assert seen["indptr"] is made[0].indptr and seen["indices"] is made[0].indices and seen["data"] is made[0].data
    assert tuple(seen["shape"]) == (30, 20)
    assert len(res) == 6 and best == 5 and [w.shape[1] for w in seen["W"]] == [2, 2, 2, 3, 3, 3]
    # the members drew their inits from the generator as nnmf() does, member after member
    g = np.random.default_rng(0)
    for b, k in enumerate([2, 2, 2, 3, 3, 3]):
        W, H = api._default_init((), (), (), (), 30, 20, k, g)
        assert np.array_equal(seen["W"][b], W)


def test_boundary_cases_hit_every_spmm_event_at_the_stacked_rank():
    """The boundary family run as batches (rank sum = the case's k, so the SpMM's worker split is the one the family was designed
    for): every SPMM event occurs in a counted case, and a counted case hits at least one."""
    hit = set()
    cases = sc.boundary_cases("zero")
    counted = 0
    for c in cases:
        ev = sbc.boundary_hits(c)
        if ev:
            counted += 1
            hit |= set(ev)
    assert hit == set(sc.SPMM_EVENTS), set(sc.SPMM_EVENTS) - hit
    batches = sbc.boundary_batch_cases()
    assert len(batches) == counted >= 6
    for c, b in zip([c for c in cases if sbc.boundary_hits(c)], batches):
        assert sum(b["ks"]) == c["k"] and np.array_equal(b["S"][0], c["S"][0]) and b["S"][3] == c["S"][3]


def test_pattern_edges_are_what_they_say():
    cases = {name: S for name, S, _ in sbc.pattern_edges()}
    for nnz in (0, 1, 63, 64, 65, 257):
        assert cases["nnz%d" % nnz][1].size == nnz
    ptr = cases["first_and_last_column_empty"][0]
    assert ptr[1] == 0 and ptr[-1] == ptr[-2] and ptr[-1] > 0
    assert (np.diff(cases["run_of_empty_columns"][0])[10:17] == 0).all()
    for name, axis in (("one_column_holds_half", 1), ("one_row_holds_half", 0)):
        counts = sc.line_counts(cases[name])[axis]
        assert 2 * counts.max() == counts.sum()
    assert cases["33x1"][3] == (33, 1) and cases["1x40"][3] == (1, 40)
    # (the wavefront split of the error kernel, restated: 257 non-zeros are two wavefronts -- of 192 and 65 entries, as the shares are
    #  whole rows of 64: in the second one lane holds two entries and 63 lanes one)
    assert sbc.spb_waves(0) == 1 and sbc.spb_waves(256) == 1 and sbc.spb_waves(257) == 2 and sbc.spb_waves(10 ** 9) == 4096
    assert sbc.spb_waves(10 ** 6, cus=1) == 16 and sbc.spb_waves(10 ** 6, cus=3) == 48
    fams = [c["name"].split("-")[0] for c in sbc.family_cases()]
    assert fams == ["empty_lines"] * 3 + ["powerlaw"] * 3 + ["heavy"] * 3
