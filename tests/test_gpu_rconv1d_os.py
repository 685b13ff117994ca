"""Overlap-save 1-D real FFT convolution (dfft_rconv1d_os, api.rconv1d_os / api.fftfilt1d) on the GPU, against longdouble references
that apply the block definition (tests/rconv1d_os_cases.py): both precisions and both filter kinds over the (m/2, discard) table of
rconv1d_os_cases.ENTRIES with n = 1, S - 1, S, S + 1, 2 S + S / 2, 3 S and n_out = n - 1, n, n + discard, item counts that make a workgroup
loop, every fused case once more on the composed route (DFFT_RCONV_FUSED=0), fftfilt1d against numpy.convolve and against fftconv1d,
the buffer contract on guarded buffers whose input guards hold NaN, and a call sequence with dfft_trim in it.

Error measure: accuracy_ref.nu per output row with n_eff = m.

The per-length sweep -- every tuned length of this family, both precisions, every kernel variant -- lives in tests/test_gpu_tuned_sweep.py."""
import ctypes as C
import os

import numpy as np
import pytest

import accuracy_ref as A
import mem_contract as MC
import rconv1d_os_cases as OC

pytestmark = pytest.mark.gpu

# BOUND: 2 x the worst nu measured on an MI355X, rounded up to two digits; tests/test_rconv1d_os_host.py holds it under 8 x the nu of the
# same-precision CPU FFT pipeline (scipy.fft per block) on the same cases.  Every test here prints its nu.  Measured (fp64 / fp32):
#   worst                2.723 / 47.308  M = 64 d = 126 n = 2 n_out = 1, complex H, composed / M = 2 d = 1 n = 2 n_out = 1, complex H, fused
#   worst with n_out > 1  2.439 / 2.525   M = 25 d = 49 (S = 1) n = 6 n_out = 5, complex H, composed / M = 2 d = 1 n = n_out = 2, complex H
#   fused against composed 1.539 / 55.507 (the same two single-sample cases); fftfilt1d 0.843 / 0.902 (against fftconv1d; m = 600 against
#   m = 1344 with 300 taps on n = 20000)
# The n_out = 1 cases set the bound: the row is ONE sample of a circular convolution of two samples with a filter of random phases, in
# which the terms nearly cancel for one of the six rows (fp32: the same-precision CPU pipeline measures the same 47.308 on it, and 2.819
# in fp64 -- tests/test_rconv1d_os_host.py), while the rounding error of the transforms scales with the whole spectrum.  Every row of
# more than one sample stays below 2.6.
BOUND = {"f64": 5.5, "f32": 95.0}

CODE = {"f64": 0, "f32": 1}
KIND = {"complex": 0, "real": 1}


def _rdt(prec):
    import torch
    return torch.float64 if prec == "f64" else torch.float32


def _cdt(prec):
    import torch
    return torch.complex128 if prec == "f64" else torch.complex64


def _filter(H, prec, kind, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(H)).to(_rdt(prec) if kind == "real" else _cdt(prec)).to(gpu)


def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


def _raw(inp, out, h, n, n_out, m, d, channels, batch, prec, kind, stream=None):
    from distributedfft_amd import _lib as L
    L.check(_lib().dfft_rconv1d_os(C.c_void_p(inp), C.c_void_p(out), C.c_void_p(h), n, n_out, m, d, channels, batch, CODE[prec], KIND[kind],
                                   C.c_void_p(stream) if stream else None), "dfft_rconv1d_os")


class _composed:
    """DFFT_RCONV_FUSED=0 for the calls inside (the library reads it per call)"""

    def __enter__(self):
        self.old = os.environ.get("DFFT_RCONV_FUSED")
        os.environ["DFFT_RCONV_FUSED"] = "0"

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("DFFT_RCONV_FUSED", None)
        else:
            os.environ["DFFT_RCONV_FUSED"] = self.old


def _check(value, prec, what, factor=1.0):
    print(f"rconv1d_os {prec} {what}: nu {value:.3f}")
    assert value <= factor * BOUND[prec], (prec, what, value, factor * BOUND[prec])


# ---- the table --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", OC.KINDS)
@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("M,d", OC.ENTRIES)
def test_against_the_longdouble_reference(gpu, M, d, prec, kind):
    """Every (n, n_out) of the entry against the reference, `in` untouched, and every fused case once more on the composed route --
    within the bound, and within twice the bound of the fused result."""
    import torch
    from distributedfft_amd import api
    lib, m = _lib(), 2 * M
    fused = OC.fused(M, prec)
    assert lib.dfft_rconv1d_os_fused_applies(m, CODE[prec]) == int(fused)
    for _, _, n, n_out, channels, batch in OC.entry_cases(M, d):
        x, H, ref = OC.case(M, d, n, n_out, channels, batch, kind)
        what = f"M={M} d={d} n={n} n_out={n_out} channels={channels} batch={batch} {kind}"
        xt = torch.from_numpy(x).to(_rdt(prec)).to(gpu).reshape(batch, channels, n)
        Ht = _filter(H, prec, kind, gpu)
        keep = xt.clone()
        got = api.rconv1d_os(xt, Ht, None if n % 2 else m, d, n_out)      # m from H's shape, and given
        assert got.shape == (batch, channels, n_out) and got.dtype == xt.dtype
        assert torch.equal(xt, keep), "in was written"
        g = got.cpu().numpy().reshape(batch * channels, n_out)
        _check(OC.nu_rows(g, ref, m, prec), prec, what + (" fused" if fused else " composed"))
        if fused:
            with _composed():
                assert lib.dfft_rconv1d_os_fused_applies(m, CODE[prec]) == 0
                comp = api.rconv1d_os(xt, Ht, m, d, n_out)
            c = comp.cpu().numpy().reshape(batch * channels, n_out)
            _check(OC.nu_rows(c, ref, m, prec), prec, what + " composed")
            _check(OC.nu_rows(g, c.astype(A.LD), m, prec), prec, what + " fused against composed", factor=2.0)


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("M,d", sorted(OC.LOOP))
def test_more_items_than_the_grid_holds(gpu, M, d, prec):
    """The FIXED case of (M, d) repeated LOOP[(M, d)] times along the batch: more items than resident workgroups x G, so a workgroup
    takes several item groups (and the last one is ragged).  Equal rows give equal results; the reference is the small case's."""
    import torch
    from distributedfft_amd import api
    m, kind = 2 * M, "complex"
    n, channels, base = OC.FIXED[(M, d)]
    x, H, ref = OC.case(M, d, n, n, channels, base, kind)
    reps = OC.LOOP[(M, d)]
    xt = torch.from_numpy(x).to(_rdt(prec)).to(gpu).reshape(base, channels, n).repeat(reps, 1, 1).contiguous()
    assert _lib().dfft_rconv1d_os_fused_applies(m, CODE[prec]) == 1
    got = api.rconv1d_os(xt, _filter(H, prec, kind, gpu), m, d)
    g = got.cpu().numpy().reshape(reps, base * channels, n)
    assert np.array_equal(g, np.broadcast_to(g[0], g.shape)), "equal rows gave different results"
    _check(OC.nu_rows(g[0], ref, m, prec), prec, f"M={M} d={d} n={n} channels={channels} batch={reps * base} {kind} looping")


# ---- fftfilt1d --------------------------------------------------------------------------------------------------------------------------
def _taps_case(n, taps, channels, batch, seed):
    x = A.rand_real((batch * channels, n), seed)
    k = A.rand_real((channels, taps), seed + 1)
    return x, k, OC.convolve_reference(x, k, n + taps - 1)


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("n,taps", [(1000, 7), (4096, 33), (20000, 300), (777, 1)])
def test_fftfilt1d_is_numpy_convolve(gpu, n, taps, prec):
    """Both modes with the chooser's block and with two blocks given by hand (which must agree within twice the bound); where fftconv1d
    accepts the problem the two agree within the bound; n = 20000 with 300 taps is beyond fftconv1d."""
    import torch
    from distributedfft_amd import api
    channels, batch = 2, 2
    x, k, full = _taps_case(n, taps, channels, batch, 15000 + n + taps)
    xt = torch.from_numpy(x).to(_rdt(prec)).to(gpu).reshape(batch, channels, n)
    kt = torch.from_numpy(k).to(_rdt(prec)).to(gpu)
    d = taps - 1 + ((taps - 1) & 1)
    for mode, n_out in (("head", n), ("full", n + taps - 1)):
        ref = full[:, :n_out]
        m, dd = api.rconv1d_os_block(taps, n_out, xt.dtype)
        assert dd == d and api.real_form(m) == 1
        got = api.fftfilt1d(xt, kt, mode)
        assert got.shape == (batch, channels, n_out) and got.dtype == xt.dtype
        g = got.cpu().numpy().reshape(-1, n_out)
        _check(OC.nu_rows(g, ref, m, prec), prec, f"fftfilt1d {mode} n={n} taps={taps} m={m} d={d}")
        others = []
        for m2 in (api.rconv1d_length(max(2 * d, d + 2, 16)), api.rconv1d_length(max(4 * d + 100, 256))):
            o = api.fftfilt1d(xt, kt, mode, m=m2).cpu().numpy().reshape(-1, n_out)
            _check(OC.nu_rows(o, ref, m2, prec), prec, f"fftfilt1d {mode} n={n} taps={taps} m={m2} d={d}")
            others.append((m2, o))
        (ma, a), (mb, b) = others
        assert ma != mb
        _check(OC.nu_rows(a, b.astype(A.LD), max(ma, mb), prec), prec, f"fftfilt1d {mode} n={n} taps={taps} m={ma} against m={mb}", factor=2.0)
        out = torch.empty_like(got)
        assert api.fftfilt1d(xt, kt, mode, out=out) is out and MC.bits_equal(out, got)
    if n + taps - 1 <= 8192:
        mc = api.rconv1d_length(n + taps - 1)
        conv = api.fftconv1d(xt, kt).cpu().numpy().reshape(-1, n)
        head = api.fftfilt1d(xt, kt).cpu().numpy().reshape(-1, n)
        _check(OC.nu_rows(head, conv.astype(A.LD), mc, prec), prec, f"fftfilt1d against fftconv1d n={n} taps={taps}")
    else:
        with pytest.raises(ValueError):
            api.fftconv1d(xt, kt)
    with pytest.raises(ValueError):
        api.fftfilt1d(xt, kt, "same")
    with pytest.raises(ValueError):
        api.fftfilt1d(xt, torch.zeros((channels, 8192), dtype=xt.dtype, device=gpu))


def test_unit_filter_is_the_identity(gpu):
    import torch
    from distributedfft_amd import api
    x = torch.from_numpy(A.rand_real((5, 3, 1000), 14100)).to(gpu)
    for H in (torch.ones((3, 65), dtype=torch.float64, device=gpu), torch.ones((3, 65), dtype=torch.complex128, device=gpu)):
        for d in (0, 32, 33):
            y = api.rconv1d_os(x, H, discard=d)
            assert float((y - x).abs().max()) <= 16 * A.EPS["f64"] * float(x.abs().max())


# ---- the buffer contract ----------------------------------------------------------------------------------------------------------------
def _nan_guards(buf, view):
    """NaN in front of and behind the view: a read outside the rows reaches the result"""
    start = MC.view_start(buf, view)
    buf[:start] = float("nan")
    buf[start + view.numel():] = float("nan")


@pytest.mark.parametrize("route", ["fused", "composed"])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("prec", A.PRECS)
def test_buffer_contract(gpu, prec, offset, route):
    """in, out and h in guarded buffers, on a 16-byte boundary (n, n_out, d even: two-real accesses) and one element past it (per-real
    accesses), the input's guards filled with NaN: nothing outside out is written, in and h are untouched, no NaN reaches the result
    and the result is right -- on the block kernel, on the composed route of the same length (DFFT_RCONV_FUSED=0) and on the composed
    route of an untuned half-length."""
    import torch
    lib = _lib()
    # (M, d, n, n_out, kind): even sizes (VEC at offset 0), odd d, odd n, n_out above n, the untuned length
    for M, d, n, n_out, kind in ((64, 32, 250, 250, "complex"), (64, 32, 250, 282, "real"), (64, 33, 250, 250, "complex"), (64, 32, 249, 249, "real"),
                                 (8, 6, 48, 54, "complex"), (36, 10, 150, 160, "complex")):
        m, channels, batch = 2 * M, 3, 5
        x, H, ref = OC.case(M, d, n, n_out, channels, batch, kind)
        rows = batch * channels
        xb, xv = MC.guarded(rows * n, _rdt(prec), gpu, offset, n)
        ob, ov = MC.guarded(rows * n_out, _rdt(prec), gpu, offset, n_out)
        hdt = _rdt(prec) if kind == "real" else _cdt(prec)
        hb, hv = MC.guarded(channels * (M + 1), hdt, gpu, offset, M + 1)
        xv.copy_(torch.from_numpy(x).to(_rdt(prec)).reshape(-1))
        hv.copy_(torch.from_numpy(np.ascontiguousarray(H)).to(hdt).reshape(-1))
        _nan_guards(xb, xv)
        xkeep, hkeep = xb.clone(), hb.clone()
        even = n % 2 == 0 and n_out % 2 == 0 and d % 2 == 0
        vec = int(even and xv.data_ptr() % (2 * xv.element_size()) == 0 and ov.data_ptr() % (2 * ov.element_size()) == 0)
        assert vec == int(even and offset == 0)
        what = f"M={M} d={d} n={n} n_out={n_out} {kind} offset={offset} {route}"
        if route == "composed":
            with _composed():
                assert lib.dfft_rconv1d_os_fused_applies(m, CODE[prec]) == 0
                _raw(xv.data_ptr(), ov.data_ptr(), hv.data_ptr(), n, n_out, m, d, channels, batch, prec, kind)
        else:
            assert lib.dfft_rconv1d_os_fused_applies(m, CODE[prec]) == int(M != 36)
            _raw(xv.data_ptr(), ov.data_ptr(), hv.data_ptr(), n, n_out, m, d, channels, batch, prec, kind)
        torch.cuda.synchronize()
        MC.guards_intact(ob, ov, what + " out")
        assert MC.bits_equal(xb, xkeep), what + ": in (or its guards) was written"
        assert MC.bits_equal(hb, hkeep), what + ": h (or its guards) was written"
        assert not bool(torch.isnan(ov).any()), what + ": a read outside the rows reached the result"
        _check(OC.nu_rows(ov.cpu().numpy().reshape(rows, n_out), ref, m, prec), prec, what)


# ---- a call sequence --------------------------------------------------------------------------------------------------------------------
def test_call_sequence_with_trim(gpu):
    """Five calls on one stream with m, d, precision and route changing between them, dfft_trim, one more call on the composed route
    (whose scratch the trim freed): every result is right."""
    import torch
    lib = _lib()
    st = torch.cuda.Stream(gpu)
    # (M, d, n, n_out, kind, prec, composed by the switch)
    seq = [(64, 32, 240, 240, "complex", "f64", False), (36, 10, 155, 165, "complex", "f64", False), (512, 256, 1920, 1919, "real", "f32", False),
           (64, 33, 95, 95, "complex", "f64", True), (25, 10, 100, 110, "real", "f32", False)]
    last = (36, 10, 62, 62, "real", "f32", False)

    def enqueue(M, d, n, n_out, kind, prec, off):
        channels, batch = 3, 2
        x, H, ref = OC.case(M, d, n, n_out, channels, batch, kind)
        xt = torch.from_numpy(x).to(_rdt(prec)).to(gpu)
        Ht = _filter(H, prec, kind, gpu)
        o = torch.empty((batch * channels, n_out), dtype=xt.dtype, device=gpu)
        st.wait_stream(torch.cuda.current_stream(gpu))
        want_fused = int(OC.fused(M, prec) and not off)
        if off:
            with _composed():
                assert lib.dfft_rconv1d_os_fused_applies(2 * M, CODE[prec]) == want_fused
                _raw(xt.data_ptr(), o.data_ptr(), Ht.data_ptr(), n, n_out, 2 * M, d, channels, batch, prec, kind, st.cuda_stream)
        else:
            assert lib.dfft_rconv1d_os_fused_applies(2 * M, CODE[prec]) == want_fused
            _raw(xt.data_ptr(), o.data_ptr(), Ht.data_ptr(), n, n_out, 2 * M, d, channels, batch, prec, kind, st.cuda_stream)
        return (xt, Ht, o, ref, 2 * M, prec, f"sequence M={M} d={d} n={n} n_out={n_out} {kind}" + (" switched off" if off else ""))

    runs = [enqueue(*c) for c in seq]
    st.synchronize()
    for _, _, o, ref, m, prec, what in runs:
        _check(OC.nu_rows(o.cpu().numpy(), ref, m, prec), prec, what)
    assert lib.dfft_trim() == 0
    _, _, o, ref, m, prec, what = enqueue(*last)
    st.synchronize()
    _check(OC.nu_rows(o.cpu().numpy(), ref, m, prec), prec, what + " after dfft_trim")
