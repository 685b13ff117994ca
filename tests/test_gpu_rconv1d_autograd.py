"""Autograd of api.rconv1d and api.fftconv1d on the GPU: torch.autograd.gradcheck in fp64, the gradients against longdouble references
built from the formulas that tests/test_rxspec1d_host.py checks against torch's CPU autograd,
    grad_x = rconv1d(g, conj H, m),   grad_H = w / m * rxspec1d(x, g, m)  (its real part for a real H),   grad_k = irfft(S, m)[:taps],
and the rules around them: out= with a tensor that requires grad, no_grad, and no cross-spectrum launch when only x needs a gradient.

grad_x is held under the bounds of tests/test_gpu_rconv1d.py, grad_H and grad_k under the bound of tests/test_gpu_rxspec1d.py (nu per
channel line over the bins, and per row of taps; n_eff = m).  Measured on an MI355X (fp64 / fp32):
    grad_x   0.785 / 0.779   fftconv1d M = 36 n = 68 / rconv1d M = 36 n = 35 complex H      (bound 16.0 / 26.0)
    grad_H   0.607 / 0.583   M = 36 n = 35, real / complex H                                (bound 56.0 / 43.0)
    grad_k   1.465 / 1.369   M = 36 n = 68, five taps; 0.893 / 0.805 at M = 1024 n = 2044   (bound 56.0 / 43.0)"""
import numpy as np
import pytest

import accuracy_ref as A
import rconv1d_cases as RC
import rxspec1d_cases as XC

pytestmark = pytest.mark.gpu

GRAD_HALVES = [48, 243, 1024, 36]       # the sweep's mid-size halves and the untuned one
TAPS = 5


def _rdt(prec):
    import torch
    return torch.float64 if prec == "f64" else torch.float32


def _check(value, bound, prec, what):
    print(f"rconv1d autograd {prec} {what}: nu {value:.3f}")
    assert value <= bound, (prec, what, value, bound)


def _weights(m):
    w = np.full(m // 2 + 1, A.LD(2) / A.LD(m), dtype=A.LD)
    w[0] = w[-1] = A.LD(1) / A.LD(m)
    return w


# ---- gradcheck --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", RC.KINDS)
@pytest.mark.parametrize("M", [8, 25])
def test_gradcheck_rconv1d(gpu, M, kind):
    import torch
    from distributedfft_amd import api
    m, n, channels, batch = 2 * M, M - 1, 3, 3
    x = torch.from_numpy(A.rand_real((batch, channels, n), 31000 + M)).to(gpu).requires_grad_(True)
    H = torch.from_numpy(np.ascontiguousarray(RC.make_filter(channels, m, kind, 31500 + M))).to(gpu).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: api.rconv1d(a, b, m), (x, H), eps=1e-6, atol=1e-7, rtol=1e-6, nondet_tol=0.0)
    assert torch.autograd.gradcheck(lambda a: api.rconv1d(a, H.detach(), m), (x,), eps=1e-6, atol=1e-7, rtol=1e-6, nondet_tol=0.0)
    assert torch.autograd.gradcheck(lambda b: api.rconv1d(x.detach(), b, m), (H,), eps=1e-6, atol=1e-7, rtol=1e-6, nondet_tol=0.0)


@pytest.mark.parametrize("M", [8, 25])
def test_gradcheck_fftconv1d(gpu, M):
    import torch
    from distributedfft_amd import api
    m, channels, batch = 2 * M, 3, 3
    n = m - TAPS + 1
    assert api.rconv1d_length(n + TAPS - 1) == m
    x = torch.from_numpy(A.rand_real((batch, channels, n), 32000 + M)).to(gpu).requires_grad_(True)
    k = torch.from_numpy(A.rand_real((channels, TAPS), 32500 + M)).to(gpu).requires_grad_(True)
    assert torch.autograd.gradcheck(api.fftconv1d, (x, k), eps=1e-6, atol=1e-7, rtol=1e-6, nondet_tol=0.0)


# ---- against the longdouble references --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("M", GRAD_HALVES)
def test_gradients_against_the_longdouble_reference(gpu, M, prec):
    import torch
    from distributedfft_amd import api
    from test_gpu_rconv1d import BOUND as RCONV_BOUND
    from test_gpu_rxspec1d import BOUND as RXSPEC_BOUND
    m, channels = 2 * M, 3
    batch = XC.batches(M, channels)[1]
    rows = batch * channels
    # rconv1d: x and the output gradient g are the two fields of the cross-spectrum case
    n = m // 2 - 1
    x, g, S, _ = XC.case(M, n, channels, batch)
    for kind in RC.KINDS:
        H = RC.make_filter(channels, m, kind, 33000 + M)
        xt = torch.from_numpy(x).to(_rdt(prec)).to(gpu).reshape(batch, channels, n).requires_grad_(True)
        Ht = torch.from_numpy(np.ascontiguousarray(H)).to(gpu)
        Ht = Ht.to(_rdt(prec) if kind == "real" else (torch.complex128 if prec == "f64" else torch.complex64)).requires_grad_(True)
        y = api.rconv1d(xt, Ht, m)
        assert y.grad_fn is not None and y.shape == xt.shape
        y.backward(torch.from_numpy(g).to(_rdt(prec)).to(gpu).reshape(batch, channels, n))
        what = f"M={M} n={n} channels={channels} batch={batch} {kind}"
        gx_ref = RC.reference(g, np.conj(H), m)
        _check(RC.nu_rows(xt.grad.cpu().numpy().reshape(rows, n), gx_ref, m, prec), RCONV_BOUND[prec], prec, what + " grad_x")
        gH_ref = S * _weights(m)
        gH_ref = gH_ref.real if kind == "real" else gH_ref
        assert Ht.grad.dtype == Ht.dtype and Ht.grad.shape == Ht.shape
        _check(XC.nu_lines(Ht.grad.cpu().numpy(), gH_ref, m, prec), RXSPEC_BOUND[prec], prec, what + " grad_H")
    # fftconv1d with n + taps - 1 = m
    n = m - TAPS + 1
    x, g, S, _ = XC.case(M, n, channels, batch)
    k = A.rand_real((channels, TAPS), 34000 + M)
    xt = torch.from_numpy(x).to(_rdt(prec)).to(gpu).reshape(batch, channels, n).requires_grad_(True)
    kt = torch.from_numpy(k).to(_rdt(prec)).to(gpu).requires_grad_(True)
    assert api.rconv1d_length(n + TAPS - 1) == m
    api.fftconv1d(xt, kt).backward(torch.from_numpy(g).to(_rdt(prec)).to(gpu).reshape(batch, channels, n))
    kp = np.zeros((channels, m), dtype=A.LD)
    kp[:, :TAPS] = k
    what = f"fftconv1d M={M} n={n} taps={TAPS} channels={channels} batch={batch}"
    gx_ref = RC.reference(g, np.conj(A.ld_rfft(kp, 1)), m)
    _check(RC.nu_rows(xt.grad.cpu().numpy().reshape(rows, n), gx_ref, m, prec), RCONV_BOUND[prec], prec, what + " grad_x")
    gk_ref = (A.ld_irfft(S, m, 1) / A.LD(m))[:, :TAPS]
    assert kt.grad.shape == kt.shape
    _check(A.nu(kt.grad.cpu().numpy(), gk_ref, m, prec, (1,)), RXSPEC_BOUND[prec], prec, what + " grad_k")


# ---- the rules --------------------------------------------------------------------------------------------------------------------------
def test_out_with_requires_grad_raises_and_no_grad_takes_the_plain_path(gpu):
    import torch
    from distributedfft_amd import api
    x = torch.from_numpy(A.rand_real((2, 3, 100), 35000)).to(gpu)
    H = torch.from_numpy(RC.make_filter(3, 128, "real", 35001)).to(gpu)
    k = torch.from_numpy(A.rand_real((3, 7), 35002)).to(gpu)
    plain = api.rconv1d(x, H, 128)
    assert plain.grad_fn is None and not plain.requires_grad
    for xr, Hr in ((True, False), (False, True)):
        xa, Ha = x.clone().requires_grad_(xr), H.clone().requires_grad_(Hr)
        with pytest.raises(ValueError):
            api.rconv1d(xa, Ha, 128, out=torch.empty_like(x))
        with pytest.raises(ValueError):
            api.fftconv1d(xa, k.clone().requires_grad_(Hr), out=torch.empty_like(x))
        y = api.rconv1d(xa, Ha, 128)
        assert y.grad_fn is not None and torch.equal(y.detach(), plain)
        with torch.no_grad():
            y = api.rconv1d(xa, Ha, 128)
            z = api.fftconv1d(xa, k.clone().requires_grad_(Hr))
            o = torch.empty_like(x)
            assert api.rconv1d(xa, Ha, 128, out=o) is o and torch.equal(o, plain)      # out= is fine where nothing is recorded
        assert y.grad_fn is None and not y.requires_grad and torch.equal(y, plain)
        assert z.grad_fn is None and torch.equal(z, api.fftconv1d(x, k))
    assert api.fftconv1d(x.clone().requires_grad_(True), k).grad_fn is not None


def test_no_cross_spectrum_when_only_x_needs_a_gradient(gpu, monkeypatch):
    """Backward honours needs_input_grad: api.rxspec1d is not called (so nothing of dfft_rxspec1d_scratch_bytes is leased) unless the
    filter or the taps require grad."""
    import torch
    from distributedfft_amd import api
    calls = []
    real = api.rxspec1d
    monkeypatch.setattr(api, "rxspec1d", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    x = torch.from_numpy(A.rand_real((20, 3, 100), 36000)).to(gpu)
    g = torch.from_numpy(A.rand_real((20, 3, 100), 36001)).to(gpu)
    H = torch.from_numpy(np.ascontiguousarray(RC.make_filter(3, 128, "complex", 36002))).to(gpu)
    k = torch.from_numpy(A.rand_real((3, 29), 36003)).to(gpu)
    assert L_scratch(100, 128, 3, 20) > 0, "the case would lease partial sums"
    xa = x.clone().requires_grad_(True)
    api.rconv1d(xa, H, 128).backward(g)
    xb = x.clone().requires_grad_(True)
    api.fftconv1d(xb, k).backward(g)
    assert calls == [] and xa.grad is not None and xb.grad is not None
    Ha = H.clone().requires_grad_(True)
    api.rconv1d(x, Ha, 128).backward(g)
    assert calls == [1] and Ha.grad is not None
    ka = k.clone().requires_grad_(True)
    api.fftconv1d(xb, ka).backward(g)
    assert calls == [1, 1] and ka.grad is not None


def L_scratch(n, m, channels, batch):
    from distributedfft_amd import _lib
    return _lib.load().dfft_rxspec1d_scratch_bytes(n, m, channels, batch, 0)
