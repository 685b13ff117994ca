"""Batched 1-D real cross-spectrum (dfft_rxspec1d, api.rxspec1d) on the GPU, against longdouble references (accuracy_ref.ld_rfft on the
zero-padded rows, conjugate-multiplied and summed over the batch; tests/rxspec1d_cases.py): both precisions over the half-lengths of
rxspec1d_cases.HALVES, n = m, m/2, m/2 - 1 and 1, one and three channels, one slice of one row and several slices with a ragged last
slice and a ragged last workgroup, one batch beyond the item-count target; every fused case once more on the composed route
(DFFT_RXSPEC_FUSED=0); the auto-spectrum; bit-identical repeats; which lines share arithmetic; the buffer contract on guarded buffers.

Error measure: accuracy_ref.nu per channel line over the m/2 + 1 bins with n_eff = m."""
import ctypes as C
import os

import numpy as np
import pytest

import accuracy_ref as A
import mem_contract as MC
import rconv1d_cases as RC
import rxspec1d_cases as XC

pytestmark = pytest.mark.gpu

# BOUND: 2 x the worst nu measured on an MI355X, rounded up to two digits; tests/test_rxspec1d_host.py holds it under 8 x the nu of the
# same-precision CPU pipeline on the same cases.  Every test here prints its nu.  Measured (fp64 / fp32, and the case):
#   worst                       27.754 / 21.211  M = 8 n = 15 three channels batch = 40000 on the composed route (the fused route 4.134 /
#                                                3.934 there; fused against composed 28.296 / 23.040; auto-spectrum 11.681 / 17.431 composed,
#                                                2.971 / 2.478 fused)
#   worst without that batch    1.048 / 2.527    M = 5 n = 8 two channels batch = 17 fused / M = 48 n = 1 three channels batch = 17 composed
#                                                (fused 2.510); fused against composed 0.949 / 1.227
# The long batch sets the bound: a bin is a sum of 40000 signed products that cancels to about 1 / sqrt(batch) of the sum of their
# moduli, and the composed route adds the rows of a channel one after the other (the fused route adds 29 or 30 rows per slice and then
# 1365 slices, so its partial sums stay smaller).  n = 1 comes next: every bin of a channel is the one number sum_b x[b] g[b].  The
# same-precision CPU pipeline measures 27.437 / 21.096 on these cases, also on the long batch (tests/test_rxspec1d_host.py).
BOUND = {"f64": 56.0, "f32": 43.0}

CODE = {"f64": 0, "f32": 1}


def _rdt(prec):
    import torch
    return torch.float64 if prec == "f64" else torch.float32


def _cdt(prec):
    import torch
    return torch.complex128 if prec == "f64" else torch.complex64


def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


def _raw(x, g, out, n, m, channels, batch, prec):
    lib = _lib()
    return lib.dfft_rxspec1d(C.c_void_p(x), C.c_void_p(g), C.c_void_p(out), n, m, channels, batch, CODE[prec], None), lib.dfft_last_error().decode()


class _composed:
    """DFFT_RXSPEC_FUSED=0 for the calls inside (the library reads it per call)"""

    def __enter__(self):
        self.old = os.environ.get("DFFT_RXSPEC_FUSED")
        os.environ["DFFT_RXSPEC_FUSED"] = "0"

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("DFFT_RXSPEC_FUSED", None)
        else:
            os.environ["DFFT_RXSPEC_FUSED"] = self.old


def _check(value, prec, what, factor=1.0):
    print(f"rxspec1d {prec} {what}: nu {value:.3f}")
    assert value <= factor * BOUND[prec], (prec, what, value, factor * BOUND[prec])


def _fields(x, g, prec, gpu, batch, channels, n):
    import torch
    return (torch.from_numpy(x).to(_rdt(prec)).to(gpu).reshape(batch, channels, n), torch.from_numpy(g).to(_rdt(prec)).to(gpu).reshape(batch, channels, n))


def _sweep_case(gpu, M, n, channels, batch, prec):
    """One case: against the reference, bit-identical on a second call, inputs untouched, exact-zero imaginary parts at DC and Nyquist;
    a fused case once more on the composed route -- within the bound, and within twice the bound of the fused result; the auto-spectrum."""
    import torch
    from distributedfft_amd import api
    lib, m = _lib(), 2 * M
    fused = XC.fused(M, prec)
    x, g, ref, auto = XC.case(M, n, channels, batch)
    what = f"M={M} n={n} channels={channels} batch={batch}"
    xt, gt = _fields(x, g, prec, gpu, batch, channels, n)
    assert lib.dfft_rxspec1d_fused_applies(n, m, CODE[prec], int(n % 2 == 0)) == int(fused), what
    assert lib.dfft_rxspec1d_slices(m, channels, batch, CODE[prec]) == XC.slices_rule(M, channels, batch), what
    xk, gk = xt.clone(), gt.clone()
    got = api.rxspec1d(xt, gt, m)
    assert got.shape == (channels, M + 1) and got.dtype == _cdt(prec)
    assert torch.equal(xt, xk) and torch.equal(gt, gk), "an input was written"
    assert MC.bits_equal(api.rxspec1d(xt, gt, m), got), ("a second call differs", what)
    s = got.cpu().numpy()
    assert np.all(s[:, 0].imag == 0) and np.all(s[:, M].imag == 0), what
    _check(XC.nu_lines(s, ref, m, prec), prec, what + (" fused" if fused else " composed"))
    a = api.rxspec1d(xt, xt, m).cpu().numpy()
    assert np.all(a.imag == 0) and np.all(a.real >= 0), what + " auto-spectrum"
    _check(XC.nu_lines(a, auto, m, prec), prec, what + " auto-spectrum")
    if fused:
        with _composed():
            assert lib.dfft_rxspec1d_fused_applies(n, m, CODE[prec], int(n % 2 == 0)) == 0
            comp = api.rxspec1d(xt, gt, m)
            assert MC.bits_equal(api.rxspec1d(xt, gt, m), comp), ("composed: a second call differs", what)
            ca = api.rxspec1d(xt, xt, m).cpu().numpy()
        c = comp.cpu().numpy()
        assert np.all(c[:, 0].imag == 0) and np.all(c[:, M].imag == 0) and np.all(ca.imag == 0) and np.all(ca.real >= 0), what
        _check(XC.nu_lines(c, ref, m, prec), prec, what + " composed")
        _check(XC.nu_lines(ca, auto, m, prec), prec, what + " composed auto-spectrum")
        _check(XC.nu_lines(s, c.astype(A.CLD), m, prec), prec, what + " fused against composed", factor=2.0)


# ---- the sweep --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("M", XC.HALVES)
def test_against_the_longdouble_reference(gpu, M, prec):
    for channels in XC.CHANNELS:
        for batch in XC.batches(M, channels):
            for n in XC.n_values(2 * M):
                _sweep_case(gpu, M, n, channels, batch, prec)


@pytest.mark.parametrize("prec", A.PRECS)
def test_more_rows_than_the_item_target(gpu, prec):
    """M = 8 with a batch beyond 8 x the item-count target: the slice count is capped by the target and a slice holds about 29 rows"""
    M, n, channels, batch = XC.BEYOND_TARGET
    assert XC.slices_rule(M, channels, batch) == 4096 // channels
    _sweep_case(gpu, M, n, channels, batch, prec)


@pytest.mark.parametrize("M", sorted(set(RC.plan_points()) - set(XC.HALVES)))
def test_every_other_tuned_length(gpu, M):
    """The tuned half-lengths the sweep above leaves out: every built instantiation runs once -- both precisions, two-real (n even) and
    per-real (n odd) accesses, two channels, several slices -- and the lengths rxspec_fused_ok excludes take the composed route."""
    from distributedfft_amd import api
    m, channels = 2 * M, 2
    batch = XC.batches(M, channels)[1]
    for n in (m - 2, m - 1):
        x, g, ref, _ = XC.case(M, n, channels, batch)
        for prec in A.PRECS:
            xt, gt = _fields(x, g, prec, gpu, batch, channels, n)
            assert _lib().dfft_rxspec1d_fused_applies(n, m, CODE[prec], int(n % 2 == 0)) == int(XC.fused(M, prec))
            got = api.rxspec1d(xt, gt, m)
            assert MC.bits_equal(api.rxspec1d(xt, gt, m), got)
            _check(XC.nu_lines(got.cpu().numpy(), ref, m, prec), prec, f"M={M} n={n} channels={channels} batch={batch}" +
                   (" fused" if XC.fused(M, prec) else " composed"))


# ---- determinism ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
def test_bit_identical_across_calls_and_trim(gpu, prec):
    """Two calls on the same inputs are bit-identical, and so is a call after dfft_trim (which frees the partial-sum scratch), on the
    fused route with several slices and on the composed route."""
    from distributedfft_amd import api
    lib = _lib()
    for M in (64, 1024, 36):
        channels, n = 3, 2 * M - 2
        batch = XC.batches(M, channels)[1] + 40
        x, g, _, _ = XC.case(M, n, channels, batch)
        xt, gt = _fields(x, g, prec, gpu, batch, channels, n)
        assert lib.dfft_rxspec1d_slices(2 * M, channels, batch, CODE[prec]) >= 2
        first = api.rxspec1d(xt, gt, 2 * M)
        assert MC.bits_equal(api.rxspec1d(xt, gt, 2 * M), first), M
        assert lib.dfft_trim() == 0
        assert MC.bits_equal(api.rxspec1d(xt, gt, 2 * M), first), (M, "after dfft_trim")
        out = first.clone().zero_()
        assert api.rxspec1d(xt, gt, 2 * M, out=out) is out and MC.bits_equal(out, first)


# ---- which lines share arithmetic -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["fused", "composed"])
@pytest.mark.parametrize("prec", A.PRECS)
def test_a_row_reaches_its_channel_and_no_other(gpu, prec, route):
    """A NaN in one row (b, c) of x, or of g, makes every bin of S[c] NaN and leaves the other channels bit-identical to the clean run;
    the same row scaled by 2^24 changes S[c] and nothing else."""
    import contextlib

    import torch
    from distributedfft_amd import api
    for M in (64, 25):
        m, channels, n = 2 * M, 3, 2 * M - 1
        batch = XC.batches(M, channels)[1]
        x, g, _, _ = XC.case(M, n, channels, batch)
        xt, gt = _fields(x, g, prec, gpu, batch, channels, n)
        with (_composed() if route == "composed" else contextlib.nullcontext()):
            assert _lib().dfft_rxspec1d_fused_applies(n, m, CODE[prec], 0) == int(route == "fused")
            clean = api.rxspec1d(xt, gt, m)
            for b, c in ((0, 1), (batch - 1, 2), (batch // 2, 0)):
                for field in (0, 1):
                    for spoil in ("nan", "scale"):
                        xs, gs = xt.clone(), gt.clone()
                        t = (xs, gs)[field]
                        if spoil == "nan":
                            t[b, c, n // 3] = float("nan")
                        else:
                            t[b, c] *= 2.0 ** 24
                        got = api.rxspec1d(xs, gs, m)
                        others = [k for k in range(channels) if k != c]
                        assert MC.bits_equal(got[others], clean[others]), (M, b, c, field, spoil)
                        if spoil == "nan":
                            assert bool(torch.isnan(got[c].real).all()), (M, b, c, field)
                        else:
                            assert not MC.bits_equal(got[c], clean[c]) and bool(torch.isfinite(got[c].real).all())


# ---- the buffer contract ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["fused", "composed"])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("prec", A.PRECS)
def test_buffer_contract(gpu, prec, offset, route):
    """x, g and out in guarded buffers, on a 16-byte boundary (two-real accesses) and one element past it (per-real accesses): nothing
    outside out is written, x and g are untouched, and the result is right -- on the fused kernel with one slice and with several, on the
    composed route of the same length and on that of an untuned half-length.  An out that overlaps an input is refused."""
    import contextlib

    import torch
    from distributedfft_amd import _lib as L
    lib = _lib()
    for M in (64, 36):
        m, channels, n = 2 * M, 3, 2 * M - 2
        for batch in XC.batches(M, channels):
            x, g, ref, _ = XC.case(M, n, channels, batch)
            rows = batch * channels
            xb, xv = MC.guarded(rows * n, _rdt(prec), gpu, offset, n)
            gb, gv = MC.guarded(rows * n, _rdt(prec), gpu, offset, n)
            ob, ov = MC.guarded(channels * (M + 1), _cdt(prec), gpu, offset, M + 1)
            xv.copy_(torch.from_numpy(x).to(_rdt(prec)).reshape(-1))
            gv.copy_(torch.from_numpy(g).to(_rdt(prec)).reshape(-1))
            xkeep, gkeep = xb.clone(), gb.clone()
            vec = int(xv.data_ptr() % (2 * xv.element_size()) == 0 and gv.data_ptr() % (2 * gv.element_size()) == 0)
            assert vec == int(offset == 0)
            what = f"M={M} n={n} batch={batch} offset={offset} {route}"
            with (_composed() if route == "composed" else contextlib.nullcontext()):
                assert lib.dfft_rxspec1d_fused_applies(n, m, CODE[prec], vec) == int(route == "fused" and M == 64)
                rc, msg = _raw(xv.data_ptr(), gv.data_ptr(), ov.data_ptr(), n, m, channels, batch, prec)
                assert rc == 0, msg
                torch.cuda.synchronize()
                MC.guards_intact(ob, ov, what + " out")
                assert MC.bits_equal(xb, xkeep) and MC.bits_equal(gb, gkeep), what + ": an input (or its guards) was written"
                _check(XC.nu_lines(ov.cpu().numpy().reshape(channels, M + 1), ref, m, prec), prec, what)
                # out inside x, inside g, and reaching into either from in front: refused, nothing written
                cs = ov.element_size()
                for bad in (xv.data_ptr(), gv.data_ptr() + (rows * n - 1) * xv.element_size(), xv.data_ptr() - channels * (M + 1) * cs + cs):
                    rc, msg = _raw(xv.data_ptr(), gv.data_ptr(), bad, n, m, channels, batch, prec)
                    assert rc == L.EINVAL and "overlaps" in msg, (what, rc, msg)
                torch.cuda.synchronize()
                assert MC.bits_equal(xb, xkeep) and MC.bits_equal(gb, gkeep)
