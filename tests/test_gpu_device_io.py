"""Matrices and factors in device memory (nnlm_set_matrix_device / nnlm_set_factors_device / nnlm_get_factors_device, k_ingest.h) on the
MI355X, with torch tensors on the device.  The yardstick everywhere is the host upload of the fp64 widening of the same values
(x.cpu().double().numpy()): the resident matrix, the missing bits and n_non_missing must be that upload's, so fits from the same explicit
init are compared BIT FOR BIT in both arithmetic modes.  Run with `pytest -m gpu`.

Bounds: kl_const is bit-equal where row_stride = 1 (the host route's partial sums in the host route's order) and within 1e-12 relative on
the other routes (summation order only; the bound test_gpu_sparse_missing.py uses for this quantity); the traces that carry kl_const (mkl;
the target of the KL methods) inherit the 1e-12.  api.nnmf in the fp32-operand mode: the project's 1e-4 bar."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nnlm_amd  # noqa: E402
from nnlm_amd import _lib, api  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MODES = [("f64", _lib.PREC_F64), ("f32", _lib.PREC_F32)]
DTYPES = ["float64", "float32", "float16", "bfloat16"]
LAYOUTS = ["C", "F", "t", "rowslice", "colslice", "Fslice"]
SHAPES = [(37, 29), (1, 300), (300, 1), (257, 129), (513, 70)]
ERR_ARG = 1


@pytest.fixture(autouse=True)
def _default_precision(monkeypatch):
    monkeypatch.delenv("NNLM_PRECISION", raising=False)


def dev():
    return torch.device("cuda", 0)


def values(n, m, rng, missing=True):
    """Non-negative values exactly representable in every source type (multiples of 1/64 below 4), non-finite entries scattered."""
    a = rng.integers(0, 256, size=(n, m)).astype(np.float64) / 64.0
    if missing and n * m >= 4:
        flat = a.reshape(-1)
        idx = rng.choice(n * m, size=max(3, n * m // 11), replace=False)
        flat[idx[0::3]] = np.nan
        flat[idx[1::3]] = np.inf
        flat[idx[2::3]] = -np.inf
    return a


def place(a, dtype, layout):
    """The n x m host array a as a device tensor of `dtype` in `layout`."""
    dt = getattr(torch, dtype)
    n, m = a.shape
    t = torch.from_numpy(a).to(dt)
    if layout == "C":
        x = t.to(dev()).contiguous()
    elif layout == "F":
        x = torch.empty_strided((n, m), (1, n), dtype=dt, device=dev())
        x.copy_(t)
    elif layout == "t":
        x = t.t().contiguous().to(dev()).t()
    elif layout == "rowslice":  # every second row of a wider C-contiguous tensor: col_stride 1, row_stride 2 (m + 3)
        big = torch.zeros((2 * n, m + 3), dtype=dt, device=dev())
        x = big[::2, :m]
        x.copy_(t)
    elif layout == "colslice":  # every third column of a C-contiguous tensor: general strides
        big = torch.zeros((n, 3 * m + 1), dtype=dt, device=dev())
        x = big[:, 1::3]
        x.copy_(t)
    elif layout == "Fslice":  # every second column of a taller column-major tensor: row_stride 1, col_stride 2 (n + 5)
        big = torch.empty_strided((n + 5, 2 * m), (1, n + 5), dtype=dt, device=dev())
        big.zero_()
        x = big[:n, ::2]
        x.copy_(t)
    assert tuple(x.shape) == (n, m)
    return x


def column_route(x):
    """row_stride == 1: the route whose partial sums are the host upload's (decided by the strides the tensor really has: a 1 x m or
    n x 1 tensor keeps whatever strides it was made with)."""
    return x.stride(0) == 1


def widen(x):
    return x.cpu().double().numpy()


def check_info(x, layout, prec, tag, fit=False):
    """fit: also one H and one W half-step from the same factors on both handles -- their cross products read every entry of the resident
    matrix (and of its split copies in the fp32-operand mode), so equal bits say the values landed where the host upload puts them."""
    ref = widen(x)
    with _lib.Handle(0, prec) as hd, _lib.Handle(0, prec) as hh:
        hd.set_matrix_device(x)
        hh.set_matrix(ref)
        if fit:
            frng = np.random.default_rng(5)
            W0, H0 = frng.random((ref.shape[0], 3)), frng.random((3, ref.shape[1]))
            facs = []
            for h in (hd, hh):
                h.set_factors(3, W0, H0)
                h.half_step(1, (0, 0, 0), 5, 1e-9, 1)
                h.half_step(0, (0, 0, 0), 5, 1e-9, 1)
                facs.append(h.get_factors())
            assert np.array_equal(facs[0][0], facs[1][0]) and np.array_equal(facs[0][1], facs[1][1]), tag
        di, hi = hd.matrix_info(), hh.matrix_info()
        assert di["n_non_missing"] == hi["n_non_missing"] == np.isfinite(ref).sum(), tag
        assert di["any_missing"] == hi["any_missing"], tag
        rel = abs(di["kl_const"] - hi["kl_const"]) / max(abs(hi["kl_const"]), 1e-300)
        print(f"{tag}: kl_const device {di['kl_const']!r} host {hi['kl_const']!r} rel {rel:.3e}")
        if column_route(x):
            assert di["kl_const"] == hi["kl_const"], (tag, di, hi)
        else:
            assert rel <= 1e-12, (tag, di, hi, rel)
        assert hd.get_info("matrix_holdout") == -1 and hd.get_info("matrix_nnz") == -1
        fin = np.isfinite(ref)
        assert hd.get_info("matrix_min_col_observed") == fin.sum(axis=0).min(), tag
        assert hd.get_info("matrix_min_row_observed") == fin.sum(axis=1).min(), tag


@pytest.mark.parametrize("mode,prec", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_ingest_state_matches_the_host_upload(mode, prec, dtype):
    rng = np.random.default_rng(11)
    for (n, m) in SHAPES:
        a = values(n, m, rng)
        for layout in LAYOUTS:
            check_info(place(a, dtype, layout), layout, prec, f"{mode} {dtype} {layout} {n}x{m}")
    a = values(300, 40, rng, missing=False)  # nothing missing: the counts are n and m
    check_info(place(a, dtype, "C"), "C", prec, f"{mode} {dtype} C finite")


@pytest.mark.parametrize("mode,prec", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_ingest_state_over_several_tiles(mode, prec, dtype):
    a = values(3000, 2000, np.random.default_rng(12))
    for layout in ("C", "F", "rowslice"):
        check_info(place(a, dtype, layout), layout, prec, f"{mode} {dtype} {layout} 3000x2000", fit=True)


@pytest.mark.parametrize("mode,prec", MODES)
@pytest.mark.parametrize("dtype", ["float64", "float16"])
def test_ingest_loops_that_carry_state(mode, prec, dtype):
    """The two loops no small shape enters: a workgroup of the row route walking more than one tile (more than 64 column tiles: m > 4096),
    and the column / gather routes spanning several chunks (8 n m > 64 MB), whose partial sums must add up in the host route's order."""
    rng = np.random.default_rng(13)
    a = values(40, 4200 + 37, rng)
    for layout in ("C", "rowslice"):
        check_info(place(a, dtype, layout), layout, prec, f"{mode} {dtype} {layout} 40x4237", fit=True)
    a = values(70000, 130, rng)
    for layout in ("F", "Fslice", "colslice"):
        check_info(place(a, dtype, layout), layout, prec, f"{mode} {dtype} {layout} 70000x130", fit=True)


@pytest.mark.parametrize("layout", ["C", "F", "colslice"])
def test_f32_mode_range_refusals_are_the_host_routes(layout):
    rng = np.random.default_rng(14)
    a = rng.random((70, 50))
    a[3, 4] = np.nan
    big = a.copy()
    big[11, 7] = 1e39  # finite, beyond the fp32 range
    tiny = a * 1e-35   # largest entry below 2^-100
    for bad in (big, tiny):
        x = place(bad, "float64", layout)
        with _lib.Handle(0, _lib.PREC_F32) as hd, _lib.Handle(0, _lib.PREC_F32) as hh:
            with pytest.raises(nnlm_amd.NnlmError) as eh:
                hh.set_matrix(bad)
            with pytest.raises(nnlm_amd.NnlmError) as ed:
                hd.set_matrix_device(x)
            assert ed.value.code == eh.value.code == _lib.ERR_UNSUPPORTED and str(ed.value) == str(eh.value)
        with _lib.Handle(0, _lib.PREC_F64) as hd:  # the strict mode takes such a matrix
            hd.set_matrix_device(x)
            assert hd.matrix_info()["n_non_missing"] == 70 * 50 - 1


def run_fit(h, k, W0, H0, method, device_factors=False):
    """One W half-step, one H half-step, then a 5-iteration run: everything the comparison reads."""
    inner = 10 if method <= 2 else 2
    if device_factors:
        h.set_factors_device(k, torch.from_numpy(W0).to(dev()), torch.from_numpy(H0).to(dev()))
    else:
        h.set_factors(k, W0, H0)
    h.half_step(0, (0, 0, 0), inner, 1e-9, method)
    h.half_step(1, (0, 0, 0), inner, 1e-9, method)
    W1, H1 = h.get_factors()
    s1 = h.take_sweeps()
    tr = h.run((0, 0, 0), (0, 0, 0), 5, -1.0, 0, False, inner, 1e-9, method, 1)
    W2, H2 = h.get_factors()
    return W1, H1, s1, tr, W2, H2


@pytest.mark.parametrize("mode,prec", MODES)
@pytest.mark.parametrize("method", [1, 2, 3, 4])
@pytest.mark.parametrize("missing", [False, True], ids=["dense", "missing"])
def test_fits_are_bit_identical_to_the_host_upload(mode, prec, method, missing):
    rng = np.random.default_rng(100 + method)
    n, m, k = 300, 170, 5
    a = values(n, m, rng, missing=missing) + (0.0 if missing else 1.0 / 64)
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    with _lib.Handle(0, prec) as hh:
        hh.set_matrix(a)
        ref = run_fit(hh, k, W0, H0, method)
    for dtype, layout in (("float64", "C"), ("float32", "F"), ("float16", "rowslice"), ("bfloat16", "colslice"), ("float32", "C")):
        x = place(a, dtype, layout)
        assert np.array_equal(widen(x), a, equal_nan=True)  # (the values are exact in every type)
        with _lib.Handle(0, prec) as hd:
            hd.set_matrix_device(x)
            got = run_fit(hd, k, W0, H0, method, device_factors=(layout == "C"))
        tag = f"{mode} method {method} {dtype} {layout}"
        for i in (0, 1, 4, 5):
            assert np.array_equal(got[i], ref[i]), (tag, i, np.abs(got[i] - ref[i]).max())
        assert got[2] == ref[2], tag
        tg, tr = got[3], ref[3]
        assert tg["n_iteration"] == tr["n_iteration"] and np.array_equal(tg["average_epoch"], tr["average_epoch"]), tag
        assert np.array_equal(tg["mse_error"], tr["mse_error"]), tag
        exact = column_route(x)
        for key in ("mkl_error", "target_error"):
            d = np.abs(tg[key] - tr[key]) / np.maximum(np.abs(tr[key]), 1e-300)
            print(f"{tag} {key}: max rel diff {d.max():.3e}")
            if exact or (key == "target_error" and method <= 2):
                assert np.array_equal(tg[key], tr[key]), (tag, key)
            else:
                assert d.max() <= 1e-12, (tag, key, d.max())


@pytest.mark.parametrize("mode,prec", MODES)
def test_factor_import_and_export(mode, prec):
    rng = np.random.default_rng(7)
    n, m, k = 301, 77, 6
    a = values(n, m, rng, missing=False)
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    with _lib.Handle(0, prec) as h:
        h.set_matrix(a)
        h.set_factors(k, W0, H0)
        Wr, Hr = h.get_factors()
        for order in ("C", "F"):
            h.set_factors_device(k, place(W0, "float64", order), place(H0, "float64", order))
            W, H = h.get_factors()
            assert np.array_equal(W, Wr) and np.array_equal(H, Hr), order
        W32, H32 = place(W0, "float32", "C"), place(H0, "float32", "F")
        h.set_factors_device(k, W32, H32)
        W, H = h.get_factors()
        h.set_factors(k, widen(W32), widen(H32))
        Wr32, Hr32 = h.get_factors()
        assert np.array_equal(W, Wr32) and np.array_equal(H, Hr32)
        h.set_factors_device(k, None, place(H0, "float64", "C"))  # a NULL descriptor = zeros
        W, H = h.get_factors()
        assert not W.any() and np.array_equal(H, Hr)
        # export: after a half-step, so the masters hold what the library wrote
        h.set_factors(k, W0, H0)
        h.half_step(0, (0, 0, 0), 10, 1e-9, 1)
        h.half_step(1, (0, 0, 0), 10, 1e-9, 1)
        Wr, Hr = h.get_factors()
        for order in ("C", "F"):
            Wo, Ho = place(np.zeros((n, k)), "float64", order), place(np.zeros((k, m)), "float64", order)
            h.get_factors_device(Wo, Ho)
            assert np.array_equal(Wo.cpu().numpy(), Wr) and np.array_equal(Ho.cpu().numpy(), Hr), order
        Wo, Ho = place(np.zeros((n, k)), "float32", "C"), place(np.zeros((k, m)), "float32", "F")
        h.get_factors_device(Wo, Ho)
        assert np.array_equal(Wo.cpu().numpy(), Wr.astype(np.float32)) and np.array_equal(Ho.cpu().numpy(), Hr.astype(np.float32))
        h.get_factors_device(None, Ho)  # either may be left out
        # a strided destination: the gaps keep their sentinel
        big = torch.full((2 * n, 3 * k), -7.0, dtype=torch.float64, device=dev())
        h.get_factors_device(big[::2, 1::3], None)
        got = big.cpu().numpy()
        assert np.array_equal(got[::2, 1::3], Wr)
        keep = np.ones(got.shape, dtype=bool)
        keep[::2, 1::3] = False
        assert (got[keep] == -7.0).all()


def test_input_is_ordered_behind_the_callers_stream():
    rng = np.random.default_rng(3)
    n, m, k = 2000, 1500, 4
    base = torch.from_numpy(rng.random((n, m))).to(dev())
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    want = (base * 2.0 + 1.0).sqrt()
    torch.cuda.synchronize()
    with _lib.Handle(0, _lib.PREC_F64) as h:
        h.set_matrix_device(want)
        ref = run_fit(h, k, W0, H0, 1)
        info = h.matrix_info()
    s = torch.cuda.Stream(device=dev())
    s.wait_stream(torch.cuda.current_stream(dev()))
    with torch.cuda.stream(s):
        junk = torch.ones((4096, 4096), device=dev())
        for _ in range(20):  # keep the stream busy ahead of the producer of A
            junk = junk @ junk * 1e-4
        x = (base * 2.0 + 1.0).sqrt()
    with _lib.Handle(0, _lib.PREC_F64) as h:
        h.set_matrix_device(x, stream=s)  # no host synchronisation in between
        got = run_fit(h, k, W0, H0, 1)
        assert h.matrix_info() == info
        out = torch.empty((n, k), dtype=torch.float64, device=dev())
        with torch.cuda.stream(s):
            h.get_factors_device(out, None)  # stream=None: the current stream, s
            twice = out * 2.0  # consumer on the caller's stream, ordered behind the export by the event
    s.synchronize()
    for i in (0, 1, 4, 5):
        assert np.array_equal(got[i], ref[i]), i
    assert np.array_equal(twice.cpu().numpy(), 2.0 * ref[4])
    torch.cuda.current_stream(dev()).wait_stream(s)


def assert_same_result(rd, rh, exact, bar=0.0):
    W, H = rd["W"], rd["H"]
    assert isinstance(W, torch.Tensor) and W.dtype == torch.float64 and W.device.type == "cuda" and isinstance(H, torch.Tensor)
    W, H = W.cpu().numpy(), H.cpu().numpy()
    assert rd["n_iteration"] == rh["n_iteration"]
    assert isinstance(rd["mse"], np.ndarray) and np.array_equal(rd["average_epochs"], rh["average_epochs"])
    if exact:
        assert np.array_equal(W, rh["W"]) and np.array_equal(H, rh["H"])
        assert np.array_equal(rd["mse"], rh["mse"]) and np.array_equal(rd["target_loss"], rh["target_loss"])
    else:
        for a, b in ((W, rh["W"]), (H, rh["H"]), (rd["mse"], rh["mse"]), (rd["target_loss"], rh["target_loss"])):
            e = float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1.0))
            print(f"relative difference {e:.3e}")
            assert e <= bar
    assert np.allclose(rd["mkl"], rh["mkl"], rtol=1e-12 if exact else max(bar, 1e-12), atol=0)


@pytest.mark.parametrize("mode", ["f64", "f32"])
def test_api_nnmf_on_a_device_tensor_is_the_host_routes_fit(mode, monkeypatch):
    if mode == "f32":
        monkeypatch.setenv("NNLM_PRECISION", "f32")
    exact, bar = mode == "f64", 1e-4
    rng = np.random.default_rng(21)
    n, m, k = 120, 90, 4
    a = rng.random((n, m))
    a[rng.random((n, m)) < 0.05] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for layout, dtype, src in (("C", "float64", a), ("F", "float64", a), ("C", "float32", a.astype(np.float32).astype(np.float64))):
            x = place(src, dtype, layout)
            kw = dict(max_iter=30, rel_tol=1e-5)
            rd = api.nnmf(x, k, rng=np.random.default_rng(5), **kw)
            rh = api.nnmf(src, k, rng=np.random.default_rng(5), **kw)
            assert_same_result(rd, rh, exact, bar)
            assert rd["options"].keys() == rh["options"].keys() and rd["run_time"] > 0
        x = place(a, "float64", "C")
        # explicit init on the device, a host mask, W_norm
        Wi = rng.random((n, k))
        Wm = rng.random((n, k)) < 0.1
        kw = dict(init={"W": torch.from_numpy(Wi).to(dev())}, mask={"W": Wm}, W_norm=1, max_iter=20, loss="mkl", method="lee")
        rd = api.nnmf(x, k, rng=np.random.default_rng(6), **kw)
        rh = api.nnmf(a, k, rng=np.random.default_rng(6), **dict(kw, init={"W": Wi}))
        assert rd["n_iteration"] == rh["n_iteration"]
        for key in ("W", "H"):
            e = float(np.linalg.norm(rd[key].cpu().numpy() - rh[key]) / np.linalg.norm(rh[key]))
            print(f"W_norm {key}: relative difference {e:.3e}")
            assert e <= (1e-13 if exact else bar)
        assert np.allclose(rd["W"].sum(0).cpu().numpy(), 1.0, rtol=1e-12)
        # known profile given on the device
        W0 = rng.random((n, 1))
        rd = api.nnmf(x, 2, init={"W0": torch.from_numpy(W0).to(dev())}, max_iter=10, rng=np.random.default_rng(8))
        rh = api.nnmf(a, 2, init={"W0": W0}, max_iter=10, rng=np.random.default_rng(8))
        assert_same_result(rd, rh, exact, bar)


def test_api_check_k_stops_with_the_host_routes_message():
    rng = np.random.default_rng(22)
    a = rng.random((40, 30))
    a[3, 2:] = np.nan  # row 3 keeps two observed entries
    a[10:, 7] = np.nan  # column 7 keeps ten
    with pytest.raises(api.NnlmStop) as eh:
        api.nnmf(a, 3)
    with pytest.raises(api.NnlmStop) as ed:
        api.nnmf(place(a, "float64", "C"), 3)
    assert str(ed.value) == str(eh.value) and "k larger than 2" in str(ed.value)
    api.nnmf(place(a, "float64", "C"), 3, check_k=False, max_iter=2, show_warning=False)


@pytest.mark.parametrize("mode", ["f64", "f32"])
def test_api_nnmf_batch_on_a_device_tensor(mode, monkeypatch):
    if mode == "f32":
        monkeypatch.setenv("NNLM_PRECISION", "f32")
    rng = np.random.default_rng(23)
    a = rng.random((150, 110))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        rd, bd = api.nnmf_batch(place(a, "float32", "C"), [2, 3], nrun=2, rng=np.random.default_rng(9), max_iter=15)
        rh, bh = api.nnmf_batch(a.astype(np.float32).astype(np.float64), [2, 3], nrun=2, rng=np.random.default_rng(9), max_iter=15)
    assert bd == bh and len(rd) == len(rh) == 4
    for d, h in zip(rd, rh):
        assert_same_result(d, h, mode == "f64", 1e-4)
    bad = a.copy()
    bad[0, 0] = np.inf
    with pytest.raises(nnlm_amd.NnlmError, match="missing"):
        api.nnmf_batch(place(bad, "float64", "C"), 2)


def test_refusals_return_err_arg_without_touching_the_pointer():
    lib = _lib.load()
    host = torch.zeros((8, 6), dtype=torch.float64)
    good = torch.ones((8, 6), dtype=torch.float64, device=dev())
    with _lib.Handle(0, _lib.PREC_F64) as h:
        def refused(d, n=8, m=6):
            rc = lib.nnlm_set_matrix_device(h._h, ctypes.byref(d), n, m, None)
            return rc, lib.nnlm_last_error(h._h).decode()
        rc, msg = refused(_lib.DevMatrix(host.data_ptr(), _lib.DT_F64, 6, 1))  # a host tensor's pointer
        assert rc == ERR_ARG and "A" in msg and "host" in msg, msg
        rc, msg = refused(_lib.DevMatrix(good.data_ptr(), _lib.DT_F64, 0, 1))  # expand(): stride 0
        assert rc == ERR_ARG and "positive" in msg, msg
        rc, msg = refused(_lib.DevMatrix(good.data_ptr(), _lib.DT_F64, 1, 2))  # as_strided overlap
        assert rc == ERR_ARG and "overlaps" in msg, msg
        rc, msg = refused(_lib.DevMatrix(good.data_ptr(), 7, 6, 1))
        assert rc == ERR_ARG and "dtype" in msg, msg
        with pytest.raises(ValueError, match="zero"):
            h.set_matrix_device(good[:1].expand(8, 6))
        with pytest.raises(nnlm_amd.NnlmError) as e:
            h.set_matrix_device(torch.as_strided(good, (8, 6), (1, 2)))
        assert e.value.code == ERR_ARG
        h.set_matrix_device(good)
        h.set_factors(2)
        with pytest.raises(nnlm_amd.NnlmError) as e:
            h.get_factors_device(torch.zeros((8, 2), dtype=torch.float16, device=dev()), None)
        assert e.value.code == ERR_ARG and "output" in str(e.value)
        if torch.cuda.device_count() < 2:
            return
        other = torch.ones((8, 6), dtype=torch.float64, device=torch.device("cuda", 1))
        rc, msg = refused(_lib.DevMatrix(other.data_ptr(), _lib.DT_F64, 6, 1))
        assert rc == ERR_ARG and "device" in msg, msg
        with pytest.raises(ValueError, match="device 1"):
            h.set_matrix_device(other)


def test_a_device_upload_leaves_a_plain_dense_handle():
    rng = np.random.default_rng(31)
    n, m, k = 60, 50, 3
    a = rng.random((n, m))
    x = place(a, "float64", "C")
    W0, H0 = rng.random((n, k)), rng.random((k, m))
    with _lib.Handle(0, _lib.PREC_F64) as h:
        h.set_matrix(a)
        ref = run_fit(h, k, W0, H0, 1)
        ptr = np.arange(0, 2 * m + 1, 2, dtype=np.int64)  # two held-out entries per column
        h.set_matrix_holdout(a, ptr, np.tile(np.array([1, 5], dtype=np.int32), m))
        assert h.get_info("matrix_holdout") == 2 * m
        h.set_matrix_device(x)
        assert h.get_info("matrix_holdout") == -1 and h.get_info("matrix_nnz") == -1 and not h.matrix_info()["any_missing"]
        got = run_fit(h, k, W0, H0, 1)
        for i in (0, 1, 4, 5):
            assert np.array_equal(got[i], ref[i])
        indptr = np.arange(0, m + 1, dtype=np.int64)
        h.set_matrix_csc(indptr, np.zeros(m, dtype=np.int32), np.ones(m), (n, m))
        assert h.get_info("matrix_nnz") == m and h.get_info("matrix_min_col_observed") == -1
        h.set_matrix_device(x)
        assert h.get_info("matrix_nnz") == -1 and h.get_info("matrix_holdout") == -1
        assert h.get_info("matrix_min_col_observed") == n and h.get_info("matrix_min_row_observed") == m
        h.set_factors_batch([2, 2])  # the batched entries take it as they take a host upload
        got = run_fit(h, k, W0, H0, 1)
        for i in (0, 1, 4, 5):
            assert np.array_equal(got[i], ref[i])
