"""Long batched 1-D real cross-spectrum (dfft_rxspec1d_long, api.rxspec1d_long) on the GPU, against longdouble references
(tests/rxspec1d_long_cases.py): the splits 64x80, 64x128, 81x128, 96x96 and 125x125 with n = m, m/2, m/2 + 1, 2 N2 + 6, 5 and 1, one row,
two batch entries of three channels and the smallest batch that is cut into slices with a ragged last one, both precisions, both store
orders, the auto-spectrum, a field off alignment, and every case once more on the composed route (DFFT_RXSPEC_LONG_FUSED=0); the Mid
instantiation of every factor length above 64; several chunks; bit-identical repeats; which lines share arithmetic.

Error measure: accuracy_ref.nu per channel line over the m/2 + 1 bins with n_eff = m, held under rxspec1d_long_cases.BOUND of the case's
class (twice the larger of the composed route's and the same-precision CPU pipeline's worst value, rounded up to two digits), fused
against composed under twice that.  Every test prints its nu.  Measured on an MI355X (fp64 / fp32), worst line per class:
    sweep    fused 0.511 / 0.561    composed 1.155 / 0.879     CPU pipeline 0.587 / 0.558     fused against composed 0.709 / 0.981
    n1       fused 0.284 / 74.977   composed 73.561 / 148.542  CPU pipeline 73.561 / 148.542  fused against composed 73.561 / 73.578
    chunks   fused 0.620            composed 1.801             CPU pipeline 1.780             fused against composed 1.894     (fp64)
(rxspec1d_long_cases.MEASURED names the cases).  The rows of one sample set the largest figures: all bins of a channel are the one
number sum_b x[b] g[b], 17 signed products that cancel to a small part of the sum of their moduli, and the rounding noise of the
long transforms of the composed route and the CPU pipeline is measured against that small sum (the fused route's transforms of a
row of one sample are sums of one term: in fp64 its products of float32 inputs are exact)."""
import os

import numpy as np
import pytest

import accuracy_ref as A
import mem_contract as MC
import rconv1d_long_cases as LC
import rxspec1d_long_cases as LX

pytestmark = pytest.mark.gpu

CODE = {"f64": 0, "f32": 1}
WORST = {}   # (route, prec, class) -> (nu, case) of this process


def _rdt(prec):
    import torch
    return torch.float64 if prec == "f64" else torch.float32


def _cdt(prec):
    import torch
    return torch.complex128 if prec == "f64" else torch.complex64


def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


class _composed:
    """DFFT_RXSPEC_LONG_FUSED=0 for the calls inside (the library reads it per call)"""

    def __enter__(self):
        self.old = os.environ.get("DFFT_RXSPEC_LONG_FUSED")
        os.environ["DFFT_RXSPEC_LONG_FUSED"] = "0"

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("DFFT_RXSPEC_LONG_FUSED", None)
        else:
            os.environ["DFFT_RXSPEC_LONG_FUSED"] = self.old


def _check(value, prec, klass, route, what, factor=1.0):
    print(f"rxspec1d_long {prec} {klass} {route} {what}: nu {value:.3f}")
    if value > WORST.get((route, prec, klass), (-1.0, ""))[0]:
        WORST[(route, prec, klass)] = (value, what)
        print(f"rxspec1d_long worst so far {route} {prec} {klass}: {value:.3f} ({what})")
    assert value <= factor * LX.BOUND[prec][klass], (prec, klass, route, what, value, factor * LX.BOUND[prec][klass])


def _fields(x, g, prec, gpu, batch, channels, n, offset=0):
    """The two fields on the device; offset = 1: one real past a 16-byte boundary (per-real accesses even for an even n)"""
    import torch
    out = []
    for a in (x, g):
        buf = torch.empty(a.size + 2, dtype=_rdt(prec), device=gpu)
        t = buf[offset:offset + a.size].view(batch, channels, n)
        t.copy_(torch.from_numpy(a).to(_rdt(prec)).reshape(batch, channels, n))
        out.append(t)
    return out


def _sweep_case(gpu, m, n, channels, batch, prec, offset=0):
    """One case: both orders against the reference, bit-identical on a second call, inputs untouched, exact-zero imaginary parts at DC
    and Nyquist, the auto-spectrum; once more on the composed route -- within the bound, and fused within twice the bound of composed."""
    import torch
    from distributedfft_amd import api
    lib, M = _lib(), m // 2
    n1, n2 = LC.split(m)
    fused, k = LX.fused(m, prec), LX.klass(n, batch)
    x, g, ref, auto = LX.case(m, n, channels, batch)
    what = f"m={m} n={n} channels={channels} batch={batch}" + (" off alignment" if offset else "")
    xt, gt = _fields(x, g, prec, gpu, batch, channels, n, offset)
    assert xt.is_contiguous() and (xt.data_ptr() % (2 * xt.element_size()) == 0) == (offset == 0)
    assert lib.dfft_rxspec1d_long_fused_applies(m, CODE[prec]) == int(fused), what
    assert lib.dfft_rxspec1d_long_slices(m, channels, batch, CODE[prec]) == LX.call_slices(m, channels, batch, prec), what
    xk, gk = xt.clone(), gt.clone()
    got = api.rxspec1d_long(xt, gt, m)
    assert got.shape == (channels, M + 1) and got.dtype == _cdt(prec)
    assert torch.equal(xt, xk) and torch.equal(gt, gk), "an input was written"
    assert MC.bits_equal(api.rxspec1d_long(xt, gt, m), got), ("a second call differs", what)
    s = got.cpu().numpy()
    assert np.all(s[:, 0].imag == 0) and np.all(s[:, M].imag == 0), what
    route = "fused" if fused else "composed"
    _check(LX.nu_lines(s, ref, m, prec), prec, k, route, what)
    # the filter's order is the same numbers, permuted
    sp = api.rxspec1d_long(xt, gt, m, filter_order=True).cpu().numpy()
    assert np.array_equal(sp, LC.permute_filter(s, n1, n2)), ("filter_order", what)
    a = api.rxspec1d_long(xt, xt, m).cpu().numpy()
    assert np.all(a.imag == 0) and np.all(a.real >= 0), what + " auto-spectrum"
    _check(LX.nu_lines(a, auto, m, prec), prec, k, route, what + " auto-spectrum")
    ap = api.rxspec1d_long(xt, xt, m, filter_order=True).cpu().numpy()
    assert np.array_equal(ap, LC.permute_filter(a, n1, n2)), ("filter_order auto-spectrum", what)
    if fused:
        with _composed():
            assert lib.dfft_rxspec1d_long_fused_applies(m, CODE[prec]) == 0
            comp = api.rxspec1d_long(xt, gt, m)
            assert MC.bits_equal(api.rxspec1d_long(xt, gt, m), comp), ("composed: a second call differs", what)
            cp = api.rxspec1d_long(xt, gt, m, filter_order=True).cpu().numpy()
            ca = api.rxspec1d_long(xt, xt, m).cpu().numpy()
        c = comp.cpu().numpy()
        assert np.all(c[:, 0].imag == 0) and np.all(c[:, M].imag == 0) and np.all(ca.imag == 0) and np.all(ca.real >= 0), what
        assert np.array_equal(cp, LC.permute_filter(c, n1, n2)), ("composed filter_order", what)
        _check(LX.nu_lines(c, ref, m, prec), prec, k, "composed", what)
        _check(LX.nu_lines(ca, auto, m, prec), prec, k, "composed", what + " auto-spectrum")
        _check(LX.nu_lines(s, c.astype(A.CLD), m, prec), prec, k, "fused-vs-composed", what, factor=2.0)


# ---- the sweep --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("m", LX.LENGTHS)
def test_against_the_longdouble_reference(gpu, m, prec):
    for batch, channels in LX.rows_of(m):
        for n in LX.n_values(m):
            _sweep_case(gpu, m, n, channels, batch, prec)
    _sweep_case(gpu, m, m // 2, 3, 2, prec, offset=1)


@pytest.mark.parametrize("N", [N for N in LX.FACTORS if N > 64])
def test_every_factor_length_above_64_runs_its_mid_kernel(gpu, N):
    """The smallest m whose split has N as the longer factor: the accumulating Mid instantiation of N runs once in both precisions (the
    (N, precision) lxspec_fused_ok excludes take the composed route) -- two batch entries of one channel, an even n (two-real accesses in
    pass A) and an odd one (per-real)."""
    m = LX.mid_length(N)
    assert LC.split(m)[1] == N
    for prec in A.PRECS:
        assert _lib().dfft_rxspec1d_long_fused_applies(m, CODE[prec]) == int((N, prec) not in LX.ROUTED)
        for n in LX.mid_n_values(m):
            _sweep_case(gpu, m, n, 1, 2, prec)


# ---- several chunks ---------------------------------------------------------------------------------------------------------------------
def test_several_chunks(gpu):
    """m = 10240 in fp64 with n = 7: 1638 rows fill the 256 MiB of pass-A results, so 3300 rows of three channels are two whole chunks and
    a ragged third whose edges fall between batch entries, and 3280 rows of four channels two chunks and a ragged third whose edges cut
    a batch entry's channels apart.  Against the reference; bit-identical on a second call; and -- three channels -- bit-identical to the
    sum, in chunk order, of three calls on the chunks' own batch entries (each of them one chunk with the same slices)."""
    import torch
    from distributedfft_amd import api
    prec = "f64"
    for m, n, channels, batch in LX.CHUNK_CASES:
        rows = batch * channels
        ch = LX.chunks(m, prec, rows)
        assert [k for _, k in ch] == [1638, 1638, rows - 2 * 1638] and 0 < rows - 2 * 1638 < 1638
        assert (1638 % channels == 0) == (channels == 3)
        x, g, ref = LX.chunk_case(m, n, channels, batch)
        xt, gt = _fields(x, g, prec, gpu, batch, channels, n)
        what = f"m={m} n={n} channels={channels} batch={batch}"
        assert _lib().dfft_rxspec1d_long_fused_applies(m, CODE[prec]) == 1
        got = api.rxspec1d_long(xt, gt, m)
        assert MC.bits_equal(api.rxspec1d_long(xt, gt, m), got), ("a second call differs", what)
        _check(LX.nu_lines(got.cpu().numpy(), ref, m, prec), prec, "chunks", "fused", what)
        gp = api.rxspec1d_long(xt, gt, m, filter_order=True)
        assert np.array_equal(gp.cpu().numpy(), LC.permute_filter(got.cpu().numpy(), *LX.SPLITS[m])), what
        if channels == 3:
            total = None
            for r0, k in ch:
                b0, nb = r0 // channels, k // channels
                assert LX.chunks(m, prec, k) == [(0, k)]
                part = api.rxspec1d_long(xt[b0:b0 + nb].contiguous(), gt[b0:b0 + nb].contiguous(), m)
                total = part if total is None else total + part
            assert MC.bits_equal(total, got), ("the chunks' own sums, added in order, differ", what)
        with _composed():
            comp = api.rxspec1d_long(xt, gt, m)
            assert MC.bits_equal(api.rxspec1d_long(xt, gt, m), comp)
        c = comp.cpu().numpy()
        _check(LX.nu_lines(c, ref, m, prec), prec, "chunks", "composed", what)
        _check(LX.nu_lines(got.cpu().numpy(), c.astype(A.CLD), m, prec), prec, "chunks", "fused-vs-composed", what, factor=2.0)
        assert torch.isfinite(got.real).all()


# ---- determinism ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
def test_bit_identical_across_calls_trim_and_other_work(gpu, prec):
    """Two calls on the same inputs are bit-identical, and so is a call after dfft_trim (which frees the scratch) and one after an
    unrelated call on the same stream (which takes the scratch and leaves other numbers in it) -- with several slices and a reduction."""
    import torch
    from distributedfft_amd import api
    lib = _lib()
    for m, channels in ((16384, 3), (31250, 1)):
        n, batch = m // 2 + 1, LX.ragged_batch(m, channels) + 24
        x, g, _, _ = LX.case(m, n, channels, batch)
        xt, gt = _fields(x, g, prec, gpu, batch, channels, n)
        assert lib.dfft_rxspec1d_long_slices(m, channels, batch, CODE[prec]) >= 2
        for order in (False, True):
            first = api.rxspec1d_long(xt, gt, m, filter_order=order)
            assert MC.bits_equal(api.rxspec1d_long(xt, gt, m, filter_order=order), first), (m, order)
            assert lib.dfft_trim() == 0
            assert MC.bits_equal(api.rxspec1d_long(xt, gt, m, filter_order=order), first), (m, order, "after dfft_trim")
            other = torch.randn(5, 3, 20000, dtype=_rdt(prec), device=gpu)
            api.rconv1d_long(other, api.rconv1d_long_filter(torch.ones(3, 20481, dtype=_rdt(prec), device=gpu)), 40960)
            api.rfft1d(torch.randn(7, 4096, dtype=_rdt(prec), device=gpu))
            assert MC.bits_equal(api.rxspec1d_long(xt, gt, m, filter_order=order), first), (m, order, "after other calls")
            out = first.clone().zero_()
            assert api.rxspec1d_long(xt, gt, m, out=out, filter_order=order) is out and MC.bits_equal(out, first)


# ---- which lines share arithmetic -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
def test_a_row_reaches_its_channel_and_no_other(gpu, prec):
    """A NaN in one row (b, c) of x, or of g, makes every bin of S[c] NaN and leaves the other channels bit-identical to the clean run
    (the fused route: an item holds rows of one channel only)."""
    import torch
    from distributedfft_amd import api
    for m in (20736, 10240):
        channels, n = 3, m // 2 + 1
        batch = LX.ragged_batch(m, channels)
        x, g, _, _ = LX.case(m, n, channels, batch)
        xt, gt = _fields(x, g, prec, gpu, batch, channels, n)
        assert _lib().dfft_rxspec1d_long_fused_applies(m, CODE[prec]) == 1
        assert _lib().dfft_rxspec1d_long_slices(m, channels, batch, CODE[prec]) >= 2
        clean = api.rxspec1d_long(xt, gt, m)
        for b, c in ((0, 1), (batch - 1, 2), (batch // 2, 0)):
            for field in (0, 1):
                xs, gs = xt.clone(), gt.clone()
                (xs, gs)[field][b, c, n // 3] = float("nan")
                got = api.rxspec1d_long(xs, gs, m)
                others = [k for k in range(channels) if k != c]
                assert MC.bits_equal(got[others], clean[others]), (m, b, c, field)
                assert bool(torch.isnan(got[c].real).all()), (m, b, c, field)
