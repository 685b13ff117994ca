"""-m gpu: real transforms along a strided axis and batched 2-D real transforms -- dfft_rfft1d_strided against numpy.fft.rfft(axis=1) /
n * irfft(axis=1) for every form of n (fused tuned lengths, odd and even; run-time-scheduled, four-step and Bluestein lengths on the
multi-pass form) and odd and even s, bit-identity with dfft_rfft1d at s = 1, guard regions, misaligned pointers, batch chunks, two
streams, the cross-talk bound of the column pairs, api.rfft1d / irfft1d with dim, and dfft_rfft2d_batch against rfft2 / irfft2.

The per-length sweep -- every tuned length of this family, both precisions, every kernel variant -- lives in tests/test_gpu_tuned_sweep.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = {"f64": 1e-11, "f32": 5e-4}
GUARD = 64
SENT = -12345.0

TUNED_EVEN = [16, 512, 768, 2048]
TUNED_ODD = [125, 243, 2187]
GENERIC = [15, 375]
FOUR_STEP = [15625, 16384]
BLUESTEIN = [1, 11, 97, 1009, 4099]
ALL_N = TUNED_EVEN + TUNED_ODD + GENERIC + FOUR_STEP + BLUESTEIN
S_VALUES = [1, 2, 3, 7, 64, 257, 1000]


def _rel(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def _rdt(prec):
    import torch
    return torch.float64 if prec == "f64" else torch.float32


def _cdt(prec):
    import torch
    return torch.complex128 if prec == "f64" else torch.complex64


def _code(prec):
    from distributedfft_amd import _lib as L
    return L.F64 if prec == "f64" else L.F32


def _strided(inp, out, n, s, batch, prec, direction, stream=None):
    from distributedfft_amd import _lib as L
    lib = L.load()
    return lib.dfft_rfft1d_strided(C.c_void_p(inp), C.c_void_p(out), n, s, batch, _code(prec), direction,
                                   C.c_void_p(stream) if stream else None)


def _check(rc):
    from distributedfft_amd import _lib as L
    assert rc == 0, (rc, L.load().dfft_last_error().decode())


def _guarded(count, dtype, gpu):
    import torch
    buf = torch.full((count + 2 * GUARD,), SENT, dtype=dtype, device=gpu)
    return buf, buf[GUARD:GUARD + count]


def _guards_intact(buf):
    h = buf.cpu()
    return bool((h[:GUARD] == SENT).all() and (h[-GUARD:] == SENT).all())


def _batch_for(n, s):
    return max(1, min(3, 2_000_000 // (n * s)))


def _forward(gpu, x, n, s, prec):
    """x: numpy [batch][n][s] -> (bins [batch][nh][s], input unchanged, guards intact)"""
    import torch
    batch = x.shape[0]
    nh = n // 2 + 1
    xi = torch.from_numpy(x).to(gpu)
    before = xi.clone()
    buf, out = _guarded(batch * nh * s, _cdt(prec), gpu)
    _check(_strided(xi.data_ptr(), out.data_ptr(), n, s, batch, prec, 1))
    torch.cuda.synchronize()
    assert torch.equal(xi, before)
    assert _guards_intact(buf)
    return out.cpu().numpy().reshape(batch, nh, s)


def _backward(gpu, X, n, s, prec):
    import torch
    batch = X.shape[0]
    Xi = torch.from_numpy(X).to(gpu)
    before = Xi.clone()
    buf, out = _guarded(batch * n * s, _rdt(prec), gpu)
    _check(_strided(Xi.data_ptr(), out.data_ptr(), n, s, batch, prec, -1))
    torch.cuda.synchronize()
    assert torch.equal(torch.view_as_real(Xi), torch.view_as_real(before))
    assert _guards_intact(buf)
    return out.cpu().numpy().reshape(batch, n, s)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n", ALL_N)
def test_strided_forward_vs_numpy(gpu, n, prec):
    rng = np.random.default_rng(n)
    for s in S_VALUES:
        batch = _batch_for(n, s)
        x = rng.standard_normal((batch, n, s)).astype(np.float64 if prec == "f64" else np.float32)
        got = _forward(gpu, x, n, s, prec)
        err = _rel(got, np.fft.rfft(x.astype(np.float64), axis=1))
        assert err < TOL[prec], (n, s, batch, prec, err)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n", ALL_N)
def test_strided_backward_non_hermitian_vs_numpy(gpu, n, prec):
    """Bins with non-zero imaginary DC and Nyquist parts: n * numpy.fft.irfft(X, n, axis=1)."""
    rng = np.random.default_rng(n + 1)
    nh = n // 2 + 1
    for s in S_VALUES:
        batch = _batch_for(n, s)
        X = (rng.standard_normal((batch, nh, s)) + 1j * rng.standard_normal((batch, nh, s)))
        X = X.astype(np.complex128 if prec == "f64" else np.complex64)
        assert np.abs(X[:, 0, :].imag).min() > 0
        got = _backward(gpu, X, n, s, prec)
        ref = n * np.fft.irfft(X.astype(np.complex128), n, axis=1)
        err = _rel(got, ref)
        assert err < TOL[prec], (n, s, batch, prec, err)


def _tuned_lengths():
    import re
    from pathlib import Path
    plans = (Path(__file__).resolve().parent.parent / "distributedfft_amd" / "csrc" / "dfft_plans.h").read_text()
    return sorted({int(v) for v in re.findall(r"^\s*X\((\d+),", plans, re.M)} | {768})


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_fused_sweep_every_tuned_length(gpu, prec):
    """Every tuned length in both directions: the fused kernels (the 256-thread tiles, the padded one-column tiles, the single-stage lengths)
    or, for the lengths routed to it, the multi-pass form; per-real access (s = 3, odd: a zero partner column) and complex access (s = 2,
    and s = 512, where the XCD-aware tile order of the fp32 sub-line tiles is on)."""
    lengths = _tuned_lengths()
    assert len(lengths) == 49
    rng = np.random.default_rng(17)
    for n in lengths:
        nh = n // 2 + 1
        for s in (2, 3, 512):
            x = rng.standard_normal((1, n, s)).astype(np.float64 if prec == "f64" else np.float32)
            got = _forward(gpu, x, n, s, prec)
            assert _rel(got, np.fft.rfft(x.astype(np.float64), axis=1)) < TOL[prec], (n, s, prec)
            X = (rng.standard_normal((1, nh, s)) + 1j * rng.standard_normal((1, nh, s))).astype(np.complex128 if prec == "f64" else np.complex64)
            back = _backward(gpu, X, n, s, prec)
            assert _rel(back, n * np.fft.irfft(X.astype(np.complex128), n, axis=1)) < TOL[prec], (n, s, prec)


@pytest.mark.parametrize("n", [16, 30, 125, 15, 97, 16384])
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_s1_bit_identical_to_rfft1d(gpu, n, prec):
    import torch
    from distributedfft_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng(7)
    batch, nh = 5, n // 2 + 1
    x = torch.from_numpy(rng.standard_normal((batch, n))).to(_rdt(prec)).to(gpu)
    a = torch.empty((batch, nh), dtype=_cdt(prec), device=gpu)
    b = torch.empty_like(a)
    _check(_strided(x.data_ptr(), a.data_ptr(), n, 1, batch, prec, 1))
    _check(lib.dfft_rfft1d(C.c_void_p(x.data_ptr()), C.c_void_p(b.data_ptr()), n, batch, _code(prec), 1, None))
    torch.cuda.synchronize()
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))
    ra = torch.empty((batch, n), dtype=_rdt(prec), device=gpu)
    rb = torch.empty_like(ra)
    _check(_strided(a.data_ptr(), ra.data_ptr(), n, 1, batch, prec, -1))
    _check(lib.dfft_rfft1d(C.c_void_p(a.data_ptr()), C.c_void_p(rb.data_ptr()), n, batch, _code(prec), -1, None))
    torch.cuda.synchronize()
    assert torch.equal(ra, rb)


@pytest.mark.parametrize("n", [512, 125, 15, 97])
@pytest.mark.parametrize("s", [64, 7])
def test_pointers_offset_by_one_element(gpu, n, s):
    """Real and complex sides one element past an allocation's start: the real side is then not aligned to a complex element, so an even
    s takes the per-real loads / stores (fused form) or the pack / unpack kernels (multi-pass form)."""
    import torch
    rng = np.random.default_rng(n * s)
    batch, nh = 3, n // 2 + 1
    x = rng.standard_normal((batch, n, s))
    rb = torch.zeros(batch * n * s + 1, dtype=torch.float64, device=gpu)
    rb[1:] = torch.from_numpy(x.reshape(-1)).to(gpu)
    cb = torch.zeros(batch * nh * s + 1, dtype=torch.complex128, device=gpu)
    _check(_strided(rb.data_ptr() + 8, cb.data_ptr() + 16, n, s, batch, "f64", 1))
    torch.cuda.synchronize()
    got = cb[1:].cpu().numpy().reshape(batch, nh, s)
    assert _rel(got, np.fft.rfft(x, axis=1)) < TOL["f64"]
    back = torch.zeros_like(rb)
    _check(_strided(cb.data_ptr() + 16, back.data_ptr() + 8, n, s, batch, "f64", -1))
    torch.cuda.synchronize()
    assert back[0].item() == 0.0
    assert _rel(back[1:].cpu().numpy().reshape(batch, n, s) / n, x) < TOL["f64"]


def test_batch_zero_and_multi_chunk_batch(gpu):
    import torch
    assert _strided(0x10000000, 0x20000000, 512, 64, 0, "f64", 1) == 0
    assert _strided(0x10000000, 0x20000000, 375, 64, 0, "f64", -1) == 0
    # 375 points (multi-pass form), s = 1000: 3 MB of packed pairs per item, 96 items take two 256 MiB chunks
    n, s, batch = 375, 1000, 96
    rng = np.random.default_rng(3)
    x = rng.standard_normal((batch, n, s))
    got = _forward(gpu, x, n, s, "f64")
    assert _rel(got, np.fft.rfft(x, axis=1)) < TOL["f64"]
    back = _backward(gpu, got, n, s, "f64")
    assert _rel(back / n, x) < TOL["f64"]
    del got, back
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n", [512, 243, 375, 97])
def test_two_streams_and_determinism(gpu, n):
    import torch
    rng = np.random.default_rng(11)
    s, batch, nh = 257, 4, n // 2 + 1
    xs = [torch.from_numpy(rng.standard_normal((batch, n, s))).to(gpu) for _ in range(2)]
    ref = []
    for x in xs:
        o = torch.empty((batch, nh, s), dtype=torch.complex128, device=gpu)
        _check(_strided(x.data_ptr(), o.data_ptr(), n, s, batch, "f64", 1))
        ref.append(o)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(gpu) for _ in range(2)]
    outs = [torch.empty((batch, nh, s), dtype=torch.complex128, device=gpu) for _ in range(2)]
    for _ in range(3):
        for x, o, st in zip(xs, outs, streams):
            _check(_strided(x.data_ptr(), o.data_ptr(), n, s, batch, "f64", 1, stream=st.cuda_stream))
    torch.cuda.synchronize()
    for o, r, x in zip(outs, ref, xs):
        assert torch.equal(torch.view_as_real(o), torch.view_as_real(r))
        assert _rel(o.cpu().numpy(), np.fft.rfft(x.cpu().numpy(), axis=1)) < TOL["f64"]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n", [512, 125, 15, 97])
def test_pair_cross_talk_bound(gpu, n, prec):
    """Even columns 1000x larger than odd ones: each column's error is bounded by its pair's combined magnitude, so the small columns keep
    an error of at most about 1000 x the tolerance relative to their own size -- and not more."""
    rng = np.random.default_rng(5)
    s, batch = 64, 2
    x = rng.standard_normal((batch, n, s))
    x[:, :, 0::2] *= 1000.0
    x = x.astype(np.float64 if prec == "f64" else np.float32)
    got = _forward(gpu, x, n, s, prec)
    ref = np.fft.rfft(x.astype(np.float64), axis=1)
    big = np.abs(ref).max()
    assert np.abs(got - ref).max() < TOL[prec] * big
    small_ref = ref[:, :, 1::2]
    small_err = np.abs(got[:, :, 1::2] - small_ref).max() / np.abs(small_ref).max()
    assert small_err < 2000 * TOL[prec], small_err


@pytest.mark.parametrize("shape,dim", [((64, 48), 0), ((6, 125, 10), 1), ((3, 16, 97, 4), 2), ((2, 375, 3, 5), 1), ((4, 5, 12), 2)])
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_api_dim(gpu, shape, dim, prec):
    import torch
    from distributedfft_amd import api
    rng = np.random.default_rng(len(shape) * 10 + dim)
    x = rng.standard_normal(shape).astype(np.float64 if prec == "f64" else np.float32)
    xt = torch.from_numpy(x).to(gpu)
    X = api.rfft1d(xt, dim=dim)
    ref = np.fft.rfft(x.astype(np.float64), axis=dim)
    assert tuple(X.shape) == ref.shape
    assert _rel(X.cpu().numpy(), ref) < TOL[prec]
    n = shape[dim]
    back = api.irfft1d(X, n, dim=dim)
    assert tuple(back.shape) == shape
    assert _rel(back.cpu().numpy() / n, x) < TOL[prec]
    # negative dim, and `out` checked like the other wrappers
    X2 = api.rfft1d(xt, out=torch.empty_like(X), dim=dim - len(shape))
    assert torch.equal(torch.view_as_real(X2), torch.view_as_real(X))
    with pytest.raises(AssertionError):
        api.rfft1d(xt, out=torch.empty(ref.shape, dtype=torch.complex64 if prec == "f64" else torch.complex128, device=gpu), dim=dim)
    for bad in (len(shape), -len(shape) - 1):  # out of range, as in torch and numpy
        with pytest.raises(IndexError):
            api.rfft1d(xt, dim=bad)
        with pytest.raises(IndexError):
            api.irfft1d(X, n, dim=bad)


SHAPES_2D = [(64, 64), (256, 512), (512, 512), (768, 512), (125, 243), (97, 1009), (1, 16), (16, 1)]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n1,n2", SHAPES_2D)
def test_rfft2d_batch_vs_numpy(gpu, n1, n2, prec):
    import torch
    from distributedfft_amd import api
    rng = np.random.default_rng(n1 * 7 + n2)
    batch = 3
    x = rng.standard_normal((batch, n1, n2)).astype(np.float64 if prec == "f64" else np.float32)
    xt = torch.from_numpy(x).to(gpu)
    before = xt.clone()
    X = api.rfft2d_batch(xt)
    assert torch.equal(xt, before)
    ref = np.fft.rfft2(x.astype(np.float64))
    assert tuple(X.shape) == ref.shape
    assert _rel(X.cpu().numpy(), ref) < TOL[prec], (n1, n2, prec)
    # backward on arbitrary bins (imaginary parts of the kz = 0 and kz = n2/2 columns not zero)
    Y = (rng.standard_normal(ref.shape) + 1j * rng.standard_normal(ref.shape)).astype(np.complex128 if prec == "f64" else np.complex64)
    Yt = torch.from_numpy(Y).to(gpu)
    Ybefore = Yt.clone()
    buf, out = _guarded(batch * n1 * n2, _rdt(prec), gpu)
    back = api.irfft2d_batch(Yt, n2, out=out.view(batch, n1, n2))
    assert torch.equal(torch.view_as_real(Yt), torch.view_as_real(Ybefore))
    assert _guards_intact(buf)
    ref_b = n1 * n2 * np.fft.irfft2(Y.astype(np.complex128), s=(n1, n2))
    assert _rel(back.cpu().numpy(), ref_b) < TOL[prec], (n1, n2, prec)


def test_rfft2d_batch_several_plane_groups(gpu):
    """fp64 512 x 512: 2.1 MB of bins per plane, 160 planes span two 256 MiB plane groups."""
    import torch
    from distributedfft_amd import api
    rng = np.random.default_rng(9)
    x = rng.standard_normal((160, 512, 512))
    X = api.rfft2d_batch(torch.from_numpy(x).to(gpu))
    Xh = X.cpu().numpy()
    assert _rel(Xh, np.fft.rfft2(x)) < TOL["f64"]
    back = api.irfft2d_batch(X, 512)
    assert _rel(back.cpu().numpy() / (512 * 512), x) < TOL["f64"]
    del X, back
    torch.cuda.empty_cache()
