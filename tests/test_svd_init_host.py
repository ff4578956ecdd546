"""The truncated SVD and the NNDSVD start without a GPU: the cases of tests/svd_init_cases.py are well posed from numpy alone (gap,
conditioning, agreement with the closed form and with the exact SVD where the method gives it), the bar of the fp32-operand mode is
measured here by emulation, the Python refusals fire before a device is touched, and the four entries are declared and bound."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from nnlm_amd import _lib, api  # noqa: E402
import svd_init_cases as S  # noqa: E402

ERR_ARG, ERR_UNSUPPORTED = 1, 5
CASES = S.all_cases()
IDS = [c.name for c in CASES]
NEW = ("nnlm_svd", "nnlm_get_svd", "nnlm_set_factors_nndsvd", "nnlm_set_factors_nndsvd_batch", "nnlm_debug_set_svd_rotate")


def restated(c, q, A=None, rnd=None):
    U, s, Vt, _ = S.rsvd(c.A if A is None else A, c.omega, q, rnd)
    return S.nndsvd(U, s, Vt, c.k)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_relative_gap_of_the_first_k_plus_one_singular_values(c):
    s = np.linalg.svd(c.A, compute_uv=False)
    gap = np.min(-np.diff(s[:c.k + 1])) / s[0]
    print(c.name, "gap %.3e" % gap)
    assert gap >= 1e-3  # (measured 1.7e-3 .. 4.5e-2)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_restatement_is_well_conditioned(c):
    ref = S.reference(c)
    g = np.random.default_rng(1)
    W, H = restated(c, 2, c.A * (1.0 + 1e-15 * g.uniform(-1, 1, c.A.shape)))
    d = S.deviation(W, H, ref["W"], ref["H"])
    print(c.name, "deviation under a 1e-15 perturbation %.1e" % d)
    assert d <= 1e-12  # (measured <= 1.1e-13)


@pytest.mark.parametrize("q", [1, 2])
@pytest.mark.parametrize("c", [c for c in CASES if not c.noise and c.blocks == c.k], ids=lambda c: c.name)
def test_noise_free_blocks_equal_the_closed_form_and_the_exact_svd(c, q):
    W, H = restated(c, q)
    We, He = S.exact_nndsvd(c.A, c.k)
    d = max(S.deviation(W, H, c.Wc, c.Hc), S.deviation(W, H, We, He))
    print(c.name, q, "%.1e" % d)
    assert d <= 1e-12  # (measured <= 4.4e-14)
    assert np.abs(c.Wc @ c.Hc - c.A).max() <= 1e-15
    assert S.reference(c)["kept"] == c.k < c.l  # (rank k below the sketch width: every orth drops directions)


@pytest.mark.parametrize("c", [c for c in CASES if c.noise and c.blocks == c.k], ids=lambda c: c.name)
def test_noisy_blocks_agree_with_the_exact_svd(c):
    ref = S.reference(c)
    We, He = S.exact_nndsvd(c.A, c.k)
    d = S.deviation(ref["W"], ref["H"], We, He)
    print(c.name, "%.1e" % d)
    assert d <= 1e-8  # (measured <= 2.0e-10)


@pytest.mark.parametrize("c", [c for c in CASES if c.blocks != c.k], ids=lambda c: c.name)
def test_a_sketch_narrower_than_the_rank_does_not_reach_the_exact_svd(c):
    """A fact of the method (flat spectrum, l = 22 < rank 40), and the reason the GPU tests compare with the restatement on the same
    omega and not with LAPACK."""
    ref = S.reference(c)
    We, He = S.exact_nndsvd(c.A, c.k)
    d = S.deviation(ref["W"], ref["H"], We, He)
    print(c.name, "%.1e" % d)
    assert d > 1e-4  # (measured 1.2e-2 and 1.6e-2)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_f32_bar_is_ten_times_the_emulated_rounding(c):
    """A and every cross-product operand rounded to the 22 bits of the split-fp16 copies, against the unrounded restatement."""
    ref = S.reference(c)
    W, H = restated(c, 2, rnd=S.round22)
    d = S.deviation(W, H, ref["W"], ref["H"])
    print(c.name, "emulated fp32-operand deviation %.2e" % d)
    assert d <= S.F32_EMULATED
    assert S.F32_BAR == 10 * S.F32_EMULATED <= 1e-3


def test_the_wide_sketch_case_is_the_same_matrix_and_within_the_same_bar():
    """l = 150 at q = 1 (tests/test_gpu_svd_init.py runs it through every form of the rotation kernel)."""
    c, base = S.wide_case(), S.case("300x200_k60", 1e-4)
    assert c.l == 150 and c.omega.shape == (150, 200) and np.array_equal(c.A, base.A)
    ref = S.reference(c, 1)
    assert ref["kept"] == 150
    g = np.random.default_rng(1)
    W, H = restated(c, 1, c.A * (1.0 + 1e-15 * g.uniform(-1, 1, c.A.shape)))
    d = S.deviation(W, H, ref["W"], ref["H"])
    W, H = restated(c, 1, rnd=S.round22)
    e = S.deviation(W, H, ref["W"], ref["H"])
    print("wide: conditioning %.1e, emulated fp32-operand deviation %.2e" % (d, e))
    assert d <= 1e-12 and e <= S.F32_EMULATED


def test_nndsvd_of_a_zero_component_is_zero_not_nan():
    U, Vt = np.eye(3, 5), np.eye(3, 4)
    W, H = S.nndsvd(U, np.array([2.0, 1.0, 0.0]), Vt, 3)
    assert np.isfinite(W).all() and np.isfinite(H).all() and not W[:, 2].any() and not H[2].any()
    Wa, Ha = S.nndsvd(U, np.array([2.0, 1.0, 0.0]), Vt, 3, fill=0.25)
    assert (Wa[W == 0] == 0.25).all() and (Ha[H == 0] == 0.25).all() and (Wa[W != 0] == W[W != 0]).all()


def test_the_four_entries_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "nnlm_mi355x.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS and ("int " + name + "(") in hdr
    for name in ("svd", "get_svd", "set_factors_nndsvd", "set_factors_nndsvd_batch"):
        assert callable(getattr(_lib.Handle, name))
    assert callable(api.truncated_svd) and '"svd_width"' in hdr and '"svd_kept"' in hdr


@pytest.fixture
def no_device(monkeypatch):
    """A Handle must not be made: the refusals below come before it."""
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "Handle", boom)


A0 = S.case("150x90_k6").A


@pytest.mark.parametrize("what", ["mask", "absent", "nan", "mkl_dense", "mkl_nndsvd", "mkl_sparse_plain", "name"])
def test_nnmf_refuses_by_name_with_a_string_init(no_device, what):
    A, kw, init = A0, {}, "nndsvd"
    if what == "mask":
        kw, word = dict(mask={"W": np.zeros((150, 6), dtype=bool) | True}), "masks"
    elif what == "absent":
        A, kw, word = S.SparseCSC(A0), dict(absent="missing"), "absent"
    elif what == "nan":
        A = A0.copy()
        A[3, 4] = np.nan
        word = "non-finite"
    elif what == "mkl_dense":
        kw, init, word = dict(loss="mkl"), "nndsvda", "dense"
    elif what == "mkl_nndsvd":
        A, kw, word = S.SparseCSC(A0), dict(loss="mkl", sparse_kl=True), "nndsvda"
    elif what == "mkl_sparse_plain":
        A, kw, init, word = S.SparseCSC(A0), dict(loss="mkl"), "nndsvda", "Sparse A"
    else:
        init, word = "svd", "'nndsvd'"
    with pytest.raises(api.NnlmStop) as e:
        api.nnmf(A, 6, init=init, **kw)
    assert word in str(e.value)


@pytest.mark.parametrize("what", ["nrun", "missing", "kl_nndsvd", "mask", "mkl", "sparse", "nan", "name"])
def test_nnmf_batch_refuses_with_a_string_init(no_device, what):
    A, k, kw, init, code = A0, [2, 3], {}, "nndsvd", ERR_UNSUPPORTED
    if what == "nrun":
        kw, code = dict(nrun=2), ERR_ARG
    elif what == "missing":
        A, kw = S.SparseCSC(A0), dict(sparse_batch="missing")
    elif what == "kl_nndsvd":
        A, kw = S.SparseCSC(A0), dict(sparse_batch="kl", loss="mkl")
    elif what == "mask":
        kw = dict(mask={"W": np.ones((150, 2), dtype=bool)})
    elif what == "mkl":
        kw = dict(loss="mkl")
    elif what == "sparse":
        A = S.SparseCSC(A0)
    elif what == "nan":
        A = A0.copy()
        A[0, 0] = np.inf
    else:
        with pytest.raises(api.NnlmStop):
            api.nnmf_batch(A, k, init="random")
        return
    with pytest.raises(_lib.NnlmError) as e:
        api.nnmf_batch(A, k, init=init, **kw)
    assert e.value.code == code


def test_nnmf_cv_and_truncated_svd_refuse_by_name(no_device):
    with pytest.raises(_lib.NnlmError) as e:
        api.nnmf_cv(A0, [2, 3], init="nndsvd")
    assert e.value.code == ERR_UNSUPPORTED and "nndsvd" in str(e.value) and "missing" in str(e.value)
    B = A0.copy()
    B[1, 1] = np.nan
    with pytest.raises(api.NnlmStop, match="non-finite"):
        api.truncated_svd(B, 3)
    for k in (0, 91):
        with pytest.raises(api.NnlmStop, match="min"):
            api.truncated_svd(A0, k)
    with pytest.raises(api.NnlmStop, match="precision"):
        api.truncated_svd(A0, 3, precision="bf16")
    with pytest.raises(_lib.NnlmError) as e:
        api.nnmf_batch(A0, [2, 3], svd_oversample=4)
    assert e.value.code == ERR_ARG


def test_the_sketch_matrix_is_drawn_in_the_fill_order_of_h():
    g1, g2 = np.random.default_rng(5), np.random.default_rng(5)
    om = api._svd_omega(4, 7, g1)
    flat = 2.0 * g2.random(28) - 1.0
    assert om.shape == (4, 7) and (om.ravel(order="F") == flat).all() and np.abs(om).max() < 1.0
    assert api._svd_width(6, 10, 2, 150, 90, "x") == (16, 2) and api._svd_width(50, 10, 0, 55, 300, "x") == (55, 0)
