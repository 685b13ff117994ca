"""Autograd of api.rconv1d_long and api.fftconv1d_long on the GPU: torch.autograd.gradcheck in fp64 with respect to x, the gradients
against longdouble references built from the formulas that tests/test_rxspec1d_long_host.py checks against torch's CPU autograd,
    grad_x = rconv1d_long(g, conj Hp, m),   grad_Hp = w / m * rxspec1d_long(x, g, m, filter_order=True)  (its real part for a real Hp),
    grad_k = irfft(S, m)[:taps] / m,
a whole fftconv1d_long step against torch's autograd of the rfft / irfft composition on the same device, and the rules around them:
out= with a tensor that requires grad, no_grad, and no cross-spectrum launch when only x needs a gradient.

grad_x is held under rconv1d_long_cases.BOUND, grad_Hp and grad_k under rxspec1d_long_cases.BOUND["sweep"] (nu per row, per channel line
over the bins, and per row of taps; n_eff = m).  Measured on an MI355X (fp64 / fp32), worst of m = 10240 and 20736:
    grad_x   0.539 / 0.619   fftconv1d_long m = 20736 n = 20437                       (bound 1.2 / 1.1)
    grad_Hp  0.461 / 0.513   m = 20736 n = 10369, complex Hp                          (bound 2.4 / 1.8)
    grad_k   0.640 / 0.751   m = 20736 n = 20437, 300 taps                            (bound 2.4 / 1.8)"""
import numpy as np
import pytest

import accuracy_ref as A
import mem_contract as MC
import rconv1d_long_cases as LC
import rxspec1d_long_cases as LX

pytestmark = pytest.mark.gpu

GRAD_LENGTHS = [10240, 20736]
TAPS = 300


def _rdt(prec):
    import torch
    return torch.float64 if prec == "f64" else torch.float32


def _check(value, bound, prec, what):
    print(f"rconv1d_long autograd {prec} {what}: nu {value:.3f}")
    assert value <= bound, (prec, what, value, bound)


def _filter(H, prec, gpu):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(H))
    if prec == "f32":
        t = t.to(torch.complex64 if t.is_complex() else torch.float32)
    return t.to(gpu)


# ---- gradcheck --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LC.KINDS)
def test_gradcheck_rconv1d_long_in_x(gpu, kind):
    """20 inputs: m = 10240, n = 5, two batch entries of two channels (gradcheck over the 5121 filter bins would take minutes)"""
    import torch
    from distributedfft_amd import api
    m, n, channels, batch = 10240, 5, 2, 2
    x = torch.from_numpy(A.rand_real((batch, channels, n), 51000)).to(gpu).requires_grad_(True)
    Hp = api.rconv1d_long_filter(_filter(LC.make_filter(channels, m, kind, 51500), "f64", gpu))
    assert torch.autograd.gradcheck(lambda a: api.rconv1d_long(a, Hp, m), (x,), eps=1e-6, atol=1e-7, rtol=1e-6, nondet_tol=0.0)


# ---- against the longdouble references --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("m", GRAD_LENGTHS)
def test_gradients_against_the_longdouble_reference(gpu, m, prec):
    import torch
    from distributedfft_amd import api
    channels, batch = 3, 2
    rows, M = batch * channels, m // 2
    n1, n2 = LX.SPLITS[m]
    w = LX.bin_weights(m)
    # rconv1d_long: x and the output gradient g are the two fields of the cross-spectrum case
    n = m // 2 + 1
    x, g, S, _ = LX.case(m, n, channels, batch)
    for kind in LC.KINDS:
        H = LC.make_filter(channels, m, kind, 52000 + m)
        xt = torch.from_numpy(x).to(_rdt(prec)).to(gpu).reshape(batch, channels, n).requires_grad_(True)
        Hp = api.rconv1d_long_filter(_filter(H, prec, gpu)).requires_grad_(True)
        y = api.rconv1d_long(xt, Hp, m)
        assert y.grad_fn is not None and y.shape == xt.shape
        y.backward(torch.from_numpy(g).to(_rdt(prec)).to(gpu).reshape(batch, channels, n))
        gx = LX.ld_conv(g, np.conj(H), m, n)
        _check(LC.nu_rows(xt.grad.cpu().numpy().reshape(rows, n), gx, m, prec), LC.BOUND[prec], prec, f"grad_x m={m} n={n} {kind}")
        gH = S * w if kind == "complex" else S.real * w
        assert Hp.grad.dtype == Hp.dtype and Hp.grad.shape == Hp.shape
        got = LX.unpermute(Hp.grad.cpu().numpy(), n1, n2)
        _check(LX.nu_lines(got, gH, m, prec), LX.BOUND[prec]["sweep"], prec, f"grad_Hp m={m} n={n} {kind}")
    # fftconv1d_long: m = rconv1d_long_length(n + taps - 1)
    n = m - TAPS + 1
    assert api.rconv1d_long_length(n + TAPS - 1) == m
    x, g, S, _ = LX.case(m, n, channels, batch)
    k = A.rand_real((channels, TAPS), 53000 + m)
    kp = np.zeros((channels, m), dtype=A.LD)
    kp[:, :TAPS] = k
    H = A.ld_rfft(kp, 1)
    xt = torch.from_numpy(x).to(_rdt(prec)).to(gpu).reshape(batch, channels, n).requires_grad_(True)
    kt = torch.from_numpy(k).to(_rdt(prec)).to(gpu).requires_grad_(True)
    y = api.fftconv1d_long(xt, kt)
    assert y.grad_fn is not None
    y.backward(torch.from_numpy(g).to(_rdt(prec)).to(gpu).reshape(batch, channels, n))
    gx = LX.ld_conv(g, np.conj(H), m, n)
    _check(LC.nu_rows(xt.grad.cpu().numpy().reshape(rows, n), gx, m, prec), LC.BOUND[prec], prec, f"grad_x fftconv1d_long m={m} n={n}")
    gk = (A.ld_irfft(S, m, 1) / A.LD(m))[:, :TAPS]
    assert kt.grad.shape == kt.shape and kt.grad.dtype == kt.dtype
    _check(A.nu(kt.grad.cpu().numpy(), gk, m, prec, (1,)), LX.BOUND[prec]["sweep"], prec, f"grad_k m={m} n={n} taps={TAPS}")


# ---- a whole step against torch's own autograd ------------------------------------------------------------------------------------------
# relative max-norm of torch's rfft / irfft composition (forward, grad_x, grad_k) against the longdouble formulas on this case, measured
# on an MI355X; the library is held within twice that of the composition.  The library itself measured 2.970e-16 / 3.510e-16 / 3.038e-16
# (fp64) and 2.721e-07 / 2.793e-07 / 2.481e-07 (fp32) against the formulas, and 8.082e-16 / 1.044e-15 / 9.027e-16 and 2.677e-07 /
# 2.491e-07 / 2.650e-07 against the composition.
COMPOSITION_REL = {"f64": {"y": 7.130e-16, "grad_x": 9.999e-16, "grad_k": 6.754e-16}, "f32": {"y": 2.342e-07, "grad_x": 2.533e-07, "grad_k": 2.420e-07}}


@pytest.mark.parametrize("prec", A.PRECS)
def test_fftconv1d_long_step_agrees_with_the_torch_composition(gpu, prec):
    """n = 6000, taps = 4500, three batch entries of two channels: forward + backward of fftconv1d_long against torch's autograd of
    irfft(rfft(x, m) * rfft(k, m), m)[..., :n] on the same device.  The tolerance is twice the relative max-norm error that the
    composition itself shows against the longdouble formulas (COMPOSITION_REL)."""
    import torch
    from distributedfft_amd import api
    n, taps, batch, channels = 6000, 4500, 3, 2
    m = api.rconv1d_long_length(n + taps - 1)
    assert m >= n + taps - 1 > 8192
    rows = batch * channels
    x = A.rand_real((rows, n), 54000)
    g = A.rand_real((rows, n), 54001)
    k = A.rand_real((channels, taps), 54002)
    kp = np.zeros((channels, m), dtype=A.LD)
    kp[:, :taps] = k
    H = A.ld_rfft(kp, 1)
    ref = {"y": LX.ld_conv(x, H, m, n), "grad_x": LX.ld_conv(g, np.conj(H), m, n),
           "grad_k": (A.ld_irfft(LX.reference(x, g, m, channels), m, 1) / A.LD(m))[:, :taps]}

    def rel(got, want):
        return float(np.max(np.abs(got.detach().cpu().numpy().astype(A.LD).reshape(want.shape) - want)) / np.max(np.abs(want)))

    def tensors():
        return (torch.from_numpy(x).to(_rdt(prec)).to(gpu).reshape(batch, channels, n).requires_grad_(True),
                torch.from_numpy(k).to(_rdt(prec)).to(gpu).requires_grad_(True),
                torch.from_numpy(g).to(_rdt(prec)).to(gpu).reshape(batch, channels, n))

    xa, ka, gt = tensors()
    ya = torch.fft.irfft(torch.fft.rfft(xa, m) * torch.fft.rfft(ka, m), m)[..., :n]
    ya.backward(gt)
    xb, kb, _ = tensors()
    yb = api.fftconv1d_long(xb, kb)
    yb.backward(gt)
    for name, ta, tb in (("y", ya, yb), ("grad_x", xa.grad, xb.grad), ("grad_k", ka.grad, kb.grad)):
        ea, eb = rel(ta, ref[name]), rel(tb, ref[name])
        agree = float((ta.detach() - tb.detach()).abs().max() / ta.detach().abs().max())
        print(f"fftconv1d_long step {prec} {name}: composition {ea:.3e} library {eb:.3e} library against composition {agree:.3e}")
        assert agree <= 2 * COMPOSITION_REL[prec][name], (prec, name, agree, COMPOSITION_REL[prec][name])


# ---- the rules around the gradients -----------------------------------------------------------------------------------------------------
def test_out_with_requires_grad_raises_and_no_grad_takes_the_plain_path(gpu, monkeypatch):
    import torch
    from distributedfft_amd import api
    m, n, channels, batch, taps = 10240, 6000, 2, 2, 4000
    x = torch.from_numpy(A.rand_real((batch, channels, n), 55000)).to(gpu)
    k = torch.from_numpy(A.rand_real((channels, taps), 55001)).to(gpu)
    Hp = api.rconv1d_long_filter(_filter(LC.make_filter(channels, m, "complex", 55002), "f64", gpu))
    plain, plain_k = api.rconv1d_long(x, Hp, m), api.fftconv1d_long(x, k)
    assert plain.grad_fn is None and plain_k.grad_fn is None and not plain.requires_grad
    xr, Hr, kr = x.clone().requires_grad_(True), Hp.clone().requires_grad_(True), k.clone().requires_grad_(True)
    out = torch.empty_like(x)
    for call in (lambda: api.rconv1d_long(xr, Hp, m, out=out), lambda: api.rconv1d_long(x, Hr, m, out=out),
                 lambda: api.fftconv1d_long(xr, k, out=out), lambda: api.fftconv1d_long(x, kr, out=out)):
        with pytest.raises(ValueError, match="out="):
            call()
    # out= without grad still works, and no_grad returns the plain path's bits and no graph
    assert api.rconv1d_long(x, Hp, m, out=out) is out and MC.bits_equal(out, plain)
    with torch.no_grad():
        y, yk = api.rconv1d_long(xr, Hr, m), api.fftconv1d_long(xr, kr)
        assert api.rconv1d_long(xr, Hr, m, out=out) is out
    assert y.grad_fn is None and yk.grad_fn is None and MC.bits_equal(y, plain) and MC.bits_equal(yk, plain_k) and MC.bits_equal(out, plain)
    # with grad the forward is the same call: the same bits
    y, yk = api.rconv1d_long(xr, Hr, m), api.fftconv1d_long(xr, kr)
    assert y.grad_fn is not None and yk.grad_fn is not None and MC.bits_equal(y.detach(), plain) and MC.bits_equal(yk.detach(), plain_k)
    # only x requires grad: the cross-spectrum is not launched
    calls = []
    real = api.rxspec1d_long
    monkeypatch.setattr(api, "rxspec1d_long", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    g = torch.ones_like(x)
    api.rconv1d_long(xr, Hp, m).backward(g)
    api.fftconv1d_long(xr, k).backward(g)
    assert calls == [] and xr.grad is not None
    api.rconv1d_long(x, Hr, m).backward(g)
    api.fftconv1d_long(x, kr).backward(g)
    assert len(calls) == 2 and Hr.grad is not None and kr.grad is not None
    # double backward is not built
    xa = x.clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(api.rconv1d_long(xa, Hp, m).sum(), xa, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()
