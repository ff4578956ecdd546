"""The batched factorisation on a sparse A whose absent entries are missing, without a GPU: the new exports; the argument checks of
api.nnmf_batch / api.nnmf_cv (sparse_batch = "missing") -- raised before the library is touched --; the hold-out split of the stored
entries; the rules of sp_gram_batch_kernel's host side restated (tile-pair mask, slot layout); and, from the fp64 oracle alone, that
every case tests/test_gpu_sparse_missing_batch.py runs is well posed and that the planted-rank input of its nnmf_cv test has its lowest
held-out error at the planted rank."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from nnlm_amd import _lib, api  # noqa: E402
from oracle import ref  # noqa: E402
import sparse_cases as sc  # noqa: E402
import sparse_missing_batch_cases as mc  # noqa: E402

ERR_ARG, ERR_UNSUPPORTED = 1, 5
WELL_POSED = 1e-11  # (test_data_cases_host.py's bound on the oracle's own dependence on the summation order)


def duck(n=30, m=20, seed=0, density=0.5):
    return sc.Csc(sc.rand_csc(n, m, density, np.random.default_rng(seed)))


@pytest.fixture
def no_device(monkeypatch):
    """Any device call fails the test: the checks below must come before it."""
    def boom(*a, **k):
        raise AssertionError("a device call was reached")
    monkeypatch.setattr(_lib, "Handle", boom)
    monkeypatch.setattr(_lib, "load", boom)


# ---- exports -----------------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "nnlm_mi355x.h")).read()
    for name in ("nnlm_set_matrix_csc_missing_batch", "nnlm_c_nnmf_csc_missing_batch"):
        assert name in _lib.EXPORTS and ("int " + name + "(") in hdr
    assert "#define NNLM_ABI_VERSION 1" in hdr and '"sp_gram_batch_pairs"' in hdr
    assert callable(_lib.c_nnmf_csc_missing_batch) and callable(_lib.Handle.set_matrix_csc_missing_batch)


# ---- refusals before any device call -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["nnmf_batch", "nnmf_cv"])
@pytest.mark.parametrize("what", ["dense", "kl", "mask", "W0", "sum65", "absent_zero"])
def test_unsupported_inputs_are_refused_under_the_door(no_device, entry, what):
    A, k, kw = duck(), [2, 3], {}
    if what == "dense":
        A = np.random.default_rng(0).random((30, 20))
    elif what == "kl":
        kw["loss"] = "mkl"
    elif what == "mask":
        kw["mask"] = {"W": np.zeros((30, 2), dtype=bool)}
    elif what == "W0":
        kw["init"] = [{"W0": np.ones((30, 1))}, {}]
    elif what == "sum65":
        A, k = duck(80, 70), [33, 32]
    elif what == "absent_zero":
        kw["absent"] = "zero"
    fn = api.nnmf_batch if entry == "nnmf_batch" else api.nnmf_cv
    if entry == "nnmf_cv" and what == "sum65":
        k = [65]  # (nnmf_cv packs a rank sum beyond 64 into successive batches: what it refuses is a single rank beyond 64)
    with pytest.raises(_lib.NnlmError) as e:
        fn(A, k, sparse_batch="missing", **kw)
    assert e.value.code == ERR_UNSUPPORTED, str(e.value)
    assert "batch" in str(e.value)


def test_another_string_is_an_argument_error(no_device):
    for fn in (api.nnmf_batch, api.nnmf_cv):
        with pytest.raises(_lib.NnlmError) as e:
            fn(duck(), [2], sparse_batch="zero")
        assert e.value.code == ERR_ARG


def test_the_present_refusals_stay(no_device):
    """Without the new value of the flag everything is refused as it was."""
    with pytest.raises(_lib.NnlmError) as e:
        api.nnmf_batch(duck(), [2, 3], sparse_batch=True, absent="missing")
    assert e.value.code == ERR_UNSUPPORTED
    with pytest.raises(_lib.NnlmError) as e:
        api.nnmf_cv(duck(), [2, 3])
    assert e.value.code == ERR_UNSUPPORTED and "sparse" in str(e.value)


def test_bad_holdout_patterns_are_refused(no_device):
    A = duck(30, 20, seed=3)
    c = api.as_csc(A)
    P = sc.pattern_of((c.indptr, c.indices, c.data, c.shape))
    i, j = (int(v[0]) for v in np.nonzero(~P))  # an absent position
    ptr = np.zeros(21, dtype=np.int64)
    ptr[j + 1:] = 1
    with pytest.raises(_lib.NnlmError) as e:
        api.nnmf_cv(A, [2], holdout=dict(indptr=ptr, indices=np.array([i], dtype=np.int32)), sparse_batch="missing")
    assert e.value.code == ERR_ARG and "not a stored entry" in str(e.value) and "row %d, column %d" % (i, j) in str(e.value)
    with pytest.raises(_lib.NnlmError) as e:  # every stored entry held out
        api.nnmf_cv(A, [2], holdout=dict(indptr=c.indptr, indices=c.indices), sparse_batch="missing")
    assert e.value.code == ERR_ARG and "every stored entry" in str(e.value)
    rows = c.indices[c.indptr[0]:c.indptr[1]]
    assert rows.size >= 2
    ptr = np.zeros(21, dtype=np.int64)
    ptr[1:] = 2
    with pytest.raises(_lib.NnlmError) as e:  # not canonical: descending rows
        api.nnmf_cv(A, [2], holdout=dict(indptr=ptr, indices=np.array([rows[1], rows[0]], dtype=np.int32)), sparse_batch="missing")
    assert e.value.code == ERR_ARG and "canonical" in str(e.value)
    for f in (0.0, 1.0, np.ones((30, 20), dtype=bool)):
        with pytest.raises(_lib.NnlmError) as e:
            api.nnmf_cv(A, [2], holdout=f, sparse_batch="missing")
        assert e.value.code == ERR_ARG


# ---- the hold-out split ------------------------------------------------------------------------------------------------------------------
class Recorder:
    """Stands in for _lib.Handle: records what nnmf_cv uploads and returns canned members."""
    seen = None

    def __init__(self, *a):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def set_matrix_csc_missing_batch(self, indptr, indices, data, shape, holdout=None):
        Recorder.seen["matrix"] = (indptr, indices, data, shape, holdout)
        Recorder.seen["uploads"] = Recorder.seen.get("uploads", 0) + 1

    def set_factors_batch(self, ks, W, H):
        self.ks, self.W, self.H = list(ks), W, H
        Recorder.seen.setdefault("batches", []).append((list(ks), [w.copy() for w in W]))

    def run_batch(self, *a, callbacks=None):
        return [dict(mse_error=np.ones(1), mkl_error=np.ones(1), target_error=np.ones(1), average_epoch=np.ones(1), n_iteration=1, warning=False)
                for _ in self.ks]

    def get_factors_batch(self):
        return list(zip(self.W, self.H))

    def holdout_errors(self):
        Recorder.seen["holdout_calls"] = Recorder.seen.get("holdout_calls", 0) + 1
        return np.arange(len(self.ks), dtype=float)[::-1] + 1.0, np.ones(len(self.ks))


@pytest.fixture
def recorder(monkeypatch):
    Recorder.seen = {}
    monkeypatch.setattr(_lib, "Handle", Recorder)
    return Recorder.seen


@pytest.mark.parametrize("f", [0.1, 0.15, 0.5])
def test_holdout_split_of_the_stored_entries(recorder, f):
    """Training and held-out entries are disjoint and canonical, together they are the stored set, round(f nnz) are held out, and the
    positions are drawn from the generator BEFORE any init; one upload, one holdout_errors() per batch, members packed in order."""
    A = duck(60, 40, seed=5, density=0.5)
    c = api.as_csc(A)
    nnz = c.indices.size
    r = api.nnmf_cv(A, list(range(1, 13)), holdout=f, rng=np.random.default_rng(9), sparse_batch="missing", check_k=False)
    ptr, idx, val, shape, ho = recorder["matrix"]
    assert ptr is c.indptr or np.array_equal(ptr, c.indptr)  # (the whole stored set goes up: the library takes the held-out entries out)
    assert np.array_equal(idx, c.indices) and np.array_equal(val, c.data) and tuple(shape) == (60, 40)
    hptr, hidx = ho
    assert hptr[-1] == hidx.size == int(round(f * nnz))
    skey = np.repeat(np.arange(40), np.diff(c.indptr)) * 60 + c.indices
    hkey = np.repeat(np.arange(40), np.diff(hptr)) * 60 + hidx
    assert np.all(np.diff(hkey) > 0) and np.isin(hkey, skey).all()  # canonical, a subset of the stored pattern
    g = np.random.default_rng(9)
    pos = np.sort(g.choice(nnz, size=int(round(f * nnz)), replace=False))
    assert np.array_equal(hkey, skey[pos])  # drawn first
    train, (hp2, hi2) = api._split_stored(c, pos)
    tkey = np.repeat(np.arange(40), np.diff(train.indptr)) * 60 + train.indices
    assert np.all(np.diff(tkey) > 0) and not np.isin(tkey, hkey).any()
    assert np.array_equal(np.sort(np.concatenate([tkey, hkey])), skey)
    assert np.array_equal(hp2, hptr) and np.array_equal(hi2, hidx)
    assert np.array_equal(recorder["batches"][0][1][0], 0.01 * g.random(60).reshape((60, 1)))  # (member 0's W follows the positions)
    assert recorder["uploads"] == 1
    assert [b[0] for b in recorder["batches"]] == [list(range(1, 11)), [11, 12]] and recorder["holdout_calls"] == 2
    assert r["k"] == list(range(1, 13)) and r["best"] == 9 and np.array_equal(r["holdout"]["indptr"], hptr)
    again = api.nnmf_cv(A, [1, 2], holdout=r["holdout"], rng=np.random.default_rng(1), sparse_batch="missing")
    assert np.array_equal(again["holdout"]["indices"], hidx)


def test_check_k_runs_on_the_training_entries(recorder):
    """The bound of nnmf(absent = 'missing') -- the fewest stored entries of a line -- on what is left after the hold-out set."""
    S = sc.rand_csc(40, 30, 0.5, np.random.default_rng(2))
    ptr, idx, val, shape = S
    rows0 = idx[ptr[0]:ptr[1]]
    assert rows0.size >= 6
    hptr = np.zeros(31, dtype=np.int64)
    hptr[1:] = rows0.size - 3  # column 0 keeps three training entries
    ho = dict(indptr=hptr, indices=rows0[:rows0.size - 3])
    A = sc.Csc(S)
    api.nnmf_cv(A, [3], holdout=ho, sparse_batch="missing")
    with pytest.raises(api.NnlmStop):
        api.nnmf_cv(A, [4], holdout=ho, sparse_batch="missing")
    api.nnmf_cv(A, [4], holdout=ho, sparse_batch="missing", check_k=False)
    api.nnmf_cv(A, [4], holdout=0.01, rng=np.random.default_rng(0), sparse_batch="missing")


def test_nnmf_batch_takes_the_missing_bound_and_entry(monkeypatch, no_device):
    seen = {}

    def fake(indptr, indices, data, shape, ks, W, H, *rest, callbacks=None, holdout=None):
        seen.update(shape=shape, ks=list(ks), holdout=holdout)
        return [dict(W=w, H=h, mse_error=np.ones(1), mkl_error=np.ones(1), target_error=np.ones(1), average_epoch=np.ones(1), n_iteration=1,
                     warning=False, holdout_mse=float("nan"), holdout_mkl=float("nan")) for w, h in zip(W, H)]

    def wrong(*a, **k):
        raise AssertionError("absent entries are missing: not the entry of absent = zero")

    monkeypatch.setattr(_lib, "c_nnmf_csc_missing_batch", fake)
    monkeypatch.setattr(_lib, "c_nnmf_csc_batch", wrong)
    P = np.random.default_rng(4).random((30, 20)) < 0.6
    P[:, 3] = False
    P[:4, 3] = True  # column 3 stores four entries
    A = sc.Csc(sc.csc_from_pattern(P, np.random.default_rng(5).random((30, 20))))
    res, best = api.nnmf_batch(A, [2, 4], sparse_batch="missing", rng=np.random.default_rng(0))
    assert seen["ks"] == [2, 4] and seen["holdout"] is None and len(res) == 2
    api.nnmf_batch(A, [2, 4], sparse_batch="missing", absent="missing", rng=np.random.default_rng(0))
    with pytest.raises(api.NnlmStop):
        api.nnmf_batch(A, [2, 5], sparse_batch="missing")


# ---- the rules of the Gram kernel's host side, restated ------------------------------------------------------------------------------------
def test_tile_pair_mask_rule():
    pairs, total, tiles = mc.tile_pairs([8] * 8)
    assert (len(pairs), total, tiles) == (4, 10, [0, 1, 2, 3]) and pairs == {(t, t) for t in range(4)}
    pairs, total, tiles = mc.tile_pairs(list(range(1, 11)))
    assert (len(pairs), total) == (7, 10)  # the diagonal and the three neighbours a straddling member touches
    assert pairs == {(0, 0), (1, 1), (2, 2), (3, 3), (0, 1), (1, 2), (2, 3)}
    assert mc.tile_pairs([1]) == ({(0, 0)}, 1, [0])
    assert len(mc.tile_pairs([64])[0]) == 10 and len(mc.tile_pairs([16, 16, 16, 16])[0]) == 4
    assert mc.tile_pairs([30, 1, 33])[0] == {(0, 0), (0, 1), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)}
    # frozen members leave the mask: [8] * 8 with only member 5 active needs one pair and gathers one tile
    pairs, _, tiles = mc.tile_pairs([8] * 8, [b == 5 for b in range(8)])
    assert pairs == {(2, 2)} and tiles == [2]
    assert mc.tile_pairs([8, 9], [False, False])[0] == set()


def test_slot_layout():
    assert mc.goff_of([8] * 8) == [256 * b for b in range(9)]
    assert mc.goff_of([1, 16, 17, 64]) == [0, 256, 512, 512 + 1024, 512 + 1024 + 4096]
    ks = [30, 1, 33]
    goff = mc.goff_of(ks)
    assert goff == [0, 1024, 1280, 1280 + 48 * 48]
    assert mc.slot_word(ks, 0, 0) == 0 and mc.slot_word(ks, 29, 29) == 29 * 32 + 29
    assert mc.slot_word(ks, 30, 30) == 1024 and mc.slot_word(ks, 31, 63) == 1280 + 32
    assert mc.slot_word(ks, 29, 30) is None and mc.slot_word(ks, 30, 31) is None
    words = [mc.slot_word(ks, i, j) for i in range(64) for j in range(i, 64)]
    words = [w for w in words if w is not None]
    assert len(words) == len(set(words)) == sum(k * (k + 1) // 2 for k in ks) and max(words) < goff[-1]


def test_boundary_batches_are_cut_where_the_family_was_designed():
    """Under the case's allocation limit the batch's chunks (slot = sum of KP_b^2) are the solo run's (slot = KP^2), in both
    orientations: the long columns stay first and last of their chunks; every long-line count of the family is there."""
    lens = set()
    several = 0
    for c0, c in zip(sc.boundary_cases("missing"), mc.boundary_cases()):
        assert sum(c["ks"]) == c0["k"]
        slot = mc.goff_of(c["ks"])[-1]
        for ptr in (c["S"][0], sc.transpose_csc(c["S"])[0]):
            mine = mc.gram_chunks_of_slot(ptr, slot, mc.alloc_limit_of(c))
            assert mine == sc.gram_chunks(ptr, sc.kp_of(c0["k"]), c0["alloc_limit"])
            several += len(mine) > 1
            lens |= {int(v) for v in np.diff(ptr)}
    assert {2047, 2048, 2049, 4096, 4097} <= lens and several >= 6


# ---- well-posedness of every GPU case, from the oracle alone ---------------------------------------------------------------------------------
CASES = mc.all_cases()


def oracle(A, k, W, H, c, method):
    return ref.c_nnmf(A, k, W, H, None, None, c["alpha"], c["beta"], c["max_iter"], c["rel_tol"], 1, 0, True, c["inner"], 1e-9, method, c["trace"])


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_every_gpu_case_is_well_posed_for_the_oracle(case):
    """The oracle's run of every member and its run on the row- and column-reversed problem (another summation order) agree to 1e-11
    with equal iteration and sweep counts: what the GPU test compares at 1e-10 is decided by the problem, not by rounding."""
    c = CASES[case]
    A = sc.densify(c["S"], "missing")
    for method in (1, 2):
        for b, k in enumerate(c["ks"]):
            o = oracle(A, k, *c["inits"][b], c, method)
            Ar, Wr, Hr = mc.reversed_member(c, b)
            r = oracle(Ar, k, Wr, Hr, c, method)
            assert np.isfinite(o["W"]).all() and np.isfinite(o["H"]).all()
            dev = max(sc.err(r["W"][::-1, :], o["W"]), sc.err(r["H"][:, ::-1], o["H"]))
            assert dev <= WELL_POSED, (c["name"], method, b, dev)
            assert o["n_iteration"] == r["n_iteration"] and np.array_equal(o["average_epoch"], r["average_epoch"]), (c["name"], method, b)


def test_stop_cases_stop_at_different_iterations():
    for c in (mc.stop_case(), mc.frozen_case()):
        A = sc.densify(c["S"], "missing")
        for method in (1, 2):
            its = [oracle(A, k, *c["inits"][b], c, method)["n_iteration"] for b, k in enumerate(c["ks"])]
            assert min(its) < max(its), (c["name"], method, its)


# ---- the planted-rank case of nnmf_cv ------------------------------------------------------------------------------------------------------
def test_planted_rank_has_the_lowest_held_out_error_for_the_oracle():
    S, pos, g = mc.planted_holdout()
    n, m = S[3]
    assert (n, m) == (120, 90) and 0.35 < S[1].size / (n * m) < 0.45 and pos.size == int(round(0.15 * S[1].size))
    T, (hptr, hidx), hval = mc.split(S, pos)
    rows, cols = sc.line_counts(T)
    assert min(rows.min(), cols.min()) >= max(mc.PLANTED_KS)  # check_k lets every candidate rank through
    A = sc.densify(T, "missing")
    hcol = np.repeat(np.arange(m), np.diff(hptr))
    mse = []
    for k, (W, H) in zip(mc.PLANTED_KS, mc.planted_inits(g, n, m)):
        o = ref.c_nnmf(A, k, W, H, None, None, [0, 0, 0], [0, 0, 0], mc.PLANTED_OPTS["max_iter"], mc.PLANTED_OPTS["rel_tol"], 1, 0, True, 50, 1e-9,
                       1, 2)
        mse.append(float(np.mean(((o["W"] @ o["H"])[hidx, hcol] - hval) ** 2)))
    order = np.argsort(mse)
    ratio = mse[order[0]] / mse[order[1]]
    print("held-out MSE k = 1 .. 6:", mse, "ratio", ratio)
    assert mc.PLANTED_KS[order[0]] == 3
    assert ratio <= 0.8 and abs(ratio - mc.PLANTED_RATIO) < 2e-3
