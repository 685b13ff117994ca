"""Batched 1-D real FFT convolution (dfft_rconv1d, api.rconv1d / api.fftconv1d) on the GPU, against longdouble references
(accuracy_ref.ld_rfft / ld_irfft on the zero-padded rows; tests/rconv1d_cases.py): both precisions and both filter kinds over the
half-lengths of rconv1d_cases.HALVES, n = m, m/2, m/2 - 1 and 1, one and three channels with a ragged last row group, row counts that
make a workgroup loop, every fused case once more on the composed route (DFFT_RCONV_FUSED=0), in place bit-identical to out of place,
fftconv1d against numpy.convolve, the buffer contract on guarded buffers, and a call sequence with dfft_trim in it.

Error measure: accuracy_ref.nu per row with n_eff = m.

The per-length sweep -- every tuned length of this family, both precisions, every kernel variant -- lives in tests/test_gpu_tuned_sweep.py."""
import ctypes as C
import os

import numpy as np
import pytest

import accuracy_ref as A
import mem_contract as MC
import rconv1d_cases as RC

pytestmark = pytest.mark.gpu

# BOUND: 2 x the worst nu measured on an MI355X, rounded up to two digits; tests/test_rconv1d_host.py holds it under 8 x the nu of the
# same-precision CPU FFT pipeline on the same cases.  Every test here prints its nu.  Measured (fp64 / fp32, and the case):
#   worst             7.965 / 12.826  M = 25 n = 1 one channel / M = 512 n = 1 three channels, complex H, fused and composed alike
#   worst with n > 1  0.956 / 1.087   M = 8 n = 7, complex H (composed / fused); fftconv1d 0.737 / 0.727 (n = 100, 7 / 100 taps)
# The n = 1 cases set the bound: the row is the single sample y[0] = x[0] mean(Re H), which for a filter with random phases is about
# 1 / sqrt(m) of the filter's size, while the rounding error of the transforms scales with the whole spectrum.  The same-precision CPU
# pipeline measures 8.169 / 17.241 on those cases (tests/test_rconv1d_host.py).
BOUND = {"f64": 16.0, "f32": 26.0}

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


def _raw(inp, out, h, n, m, channels, batch, prec, kind, stream=None):
    from distributedfft_amd import _lib as L
    L.check(_lib().dfft_rconv1d(C.c_void_p(inp), C.c_void_p(out), C.c_void_p(h), n, m, channels, batch, CODE[prec], KIND[kind],
                                C.c_void_p(stream) if stream else None), "dfft_rconv1d")


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
    print(f"rconv1d {prec} {what}: nu {value:.3f}")
    assert value <= factor * BOUND[prec], (prec, what, value, factor * BOUND[prec])


# ---- the sweep --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", RC.KINDS)
@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("M", RC.HALVES)
def test_against_the_longdouble_reference(gpu, M, prec, kind):
    """n = m, m/2, m/2 - 1, 1 on one and three channels: out of place against the reference, in place bit-identical, and every fused case
    once more on the composed route -- within the bound, and within twice the bound of the fused result."""
    import torch
    from distributedfft_amd import api
    lib, m = _lib(), 2 * M
    fused = M in RC.TUNED_HALVES
    for channels in RC.CHANNELS:
        batch = RC.batch_for(M, channels)
        Hm = None
        for n in RC.n_values(m):
            x, H, ref = RC.case(M, n, channels, batch, kind)
            what = f"M={M} n={n} channels={channels} batch={batch} {kind}"
            xt = torch.from_numpy(x).to(_rdt(prec)).to(gpu).reshape(batch, channels, n)
            Ht = _filter(H, prec, kind, gpu)
            assert lib.dfft_rconv1d_fused_applies(n, m, CODE[prec], KIND[kind], int(n % 2 == 0)) == int(fused), what
            keep = xt.clone()
            got = api.rconv1d(xt, Ht, None if Hm is None else m)   # m from H's shape, and given
            Hm = m
            assert torch.equal(xt, keep), "in was written"
            g = got.cpu().numpy().reshape(batch * channels, n)
            _check(RC.nu_rows(g, ref, m, prec), prec, what + (" fused" if fused else " composed"))
            y = xt.clone()
            assert api.rconv1d(y, Ht, m, out=y) is y
            assert MC.bits_equal(y, got), ("in place differs from out of place", what)
            if fused:
                with _composed():
                    assert lib.dfft_rconv1d_fused_applies(n, m, CODE[prec], KIND[kind], int(n % 2 == 0)) == 0
                    comp = api.rconv1d(xt, Ht, m)
                    z = xt.clone()
                    api.rconv1d(z, Ht, m, out=z)
                assert MC.bits_equal(z, comp), ("composed: in place differs from out of place", what)
                c = comp.cpu().numpy().reshape(batch * channels, n)
                _check(RC.nu_rows(c, ref, m, prec), prec, what + " composed")
                _check(RC.nu_rows(g, c.astype(A.LD), m, prec), prec, what + " fused against composed", factor=2.0)


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("M,n", [(8, 7), (4096, 8192)])
def test_more_rows_than_the_grid_holds(gpu, M, n, prec):
    """3 channels x LOOP_HALVES[M] batches: more rows than resident workgroups x G, so a workgroup takes several row groups (and the last
    one is ragged).  The rows repeat the rows of one small case, whose reference is computed once."""
    import torch
    from distributedfft_amd import api
    m, channels, kind = 2 * M, 3, "complex"
    base = RC.batch_for(M, channels)
    x, H, ref = RC.case(M, n, channels, base, kind)
    reps = -(-RC.LOOP_HALVES[M] // base)
    batch = reps * base
    xt = torch.from_numpy(x).to(_rdt(prec)).to(gpu).reshape(base, channels, n).repeat(reps, 1, 1).contiguous()
    assert _lib().dfft_rconv1d_fused_applies(n, m, CODE[prec], KIND[kind], int(n % 2 == 0)) == 1
    got = api.rconv1d(xt, _filter(H, prec, kind, gpu))
    g = got.cpu().numpy().reshape(reps, base * channels, n)
    assert np.array_equal(g, np.broadcast_to(g[0], g.shape)), "equal rows gave different results"
    _check(RC.nu_rows(g[0], ref, m, prec), prec, f"M={M} n={n} channels={channels} batch={batch} {kind} looping")
    y = xt.clone()
    api.rconv1d(y, _filter(H, prec, kind, gpu), out=y)
    assert MC.bits_equal(y, got)


# ---- fftconv1d --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("n", [100, 4096])
def test_fftconv1d_is_numpy_convolve(gpu, n, prec):
    import torch
    from distributedfft_amd import api
    channels, batch = 2, 2
    x = A.rand_real((batch, channels, n), 12000 + n)
    for taps in (1, 7, n):
        k = A.rand_real((channels, taps), 13000 + n + taps)
        ref = np.stack([np.stack([np.convolve(x[b, c].astype(A.LD), k[c].astype(A.LD))[:n] for c in range(channels)]) for b in range(batch)])
        assert ref.dtype == A.LD
        xt = torch.from_numpy(x).to(_rdt(prec)).to(gpu)
        kt = torch.from_numpy(k).to(_rdt(prec)).to(gpu)
        m = api.rconv1d_length(n + taps - 1)
        assert m >= n + taps - 1 and api.real_form(m) == 1
        got = api.fftconv1d(xt, kt)
        assert got.shape == xt.shape and got.dtype == xt.dtype
        _check(RC.nu_rows(got.cpu().numpy().reshape(-1, n), ref.reshape(-1, n), m, prec), prec, f"fftconv1d n={n} taps={taps} m={m}")
        y = xt.clone()
        assert api.fftconv1d(y, kt, out=y) is y and MC.bits_equal(y, got)
    with pytest.raises(ValueError):
        api.fftconv1d(torch.zeros((1, 1, 8000), dtype=_rdt(prec), device=gpu), torch.zeros((1, 194), dtype=_rdt(prec), device=gpu))


def test_unit_filter_is_the_identity(gpu):
    import torch
    from distributedfft_amd import api
    x = torch.from_numpy(A.rand_real((5, 3, 128), 14000)).to(gpu)
    for H in (torch.ones((3, 65), dtype=torch.float64, device=gpu), torch.ones((3, 65), dtype=torch.complex128, device=gpu)):
        y = api.rconv1d(x, H)
        assert float((y - x).abs().max()) <= 16 * A.EPS["f64"] * float(x.abs().max())


# ---- the buffer contract ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["fused", "composed"])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [128, 99])
@pytest.mark.parametrize("prec", A.PRECS)
def test_buffer_contract(gpu, prec, n, offset, route):
    """in, out and h in guarded buffers, on a 16-byte boundary (n even: two-real accesses) and one element past it (per-real accesses):
    nothing outside out is written, in and h are untouched, and the result is right -- on the fused kernel, on the composed route of
    the same length (DFFT_RCONV_FUSED=0) and on the composed route of an untuned half-length."""
    import torch
    lib = _lib()
    for M, kind in ((64, "complex"), (64, "real"), (36, "complex")):
        m, channels, batch = 2 * M, 3, 5
        nn = min(n, m) - (1 if (n % 2 and min(n, m) % 2 == 0) else 0)    # keeps n's parity below m
        x, H, ref = RC.case(M, nn, channels, batch, kind)
        rows = batch * channels
        xb, xv = MC.guarded(rows * nn, _rdt(prec), gpu, offset, nn)
        ob, ov = MC.guarded(rows * nn, _rdt(prec), gpu, offset, nn)
        hdt = _rdt(prec) if kind == "real" else _cdt(prec)
        hb, hv = MC.guarded(channels * (M + 1), hdt, gpu, offset, M + 1)
        xv.copy_(torch.from_numpy(x).to(_rdt(prec)).reshape(-1))
        hv.copy_(torch.from_numpy(np.ascontiguousarray(H)).to(hdt).reshape(-1))
        xkeep, hkeep = xb.clone(), hb.clone()
        vec = int(nn % 2 == 0 and xv.data_ptr() % (2 * xv.element_size()) == 0 and ov.data_ptr() % (2 * ov.element_size()) == 0)
        assert vec == int(nn % 2 == 0 and offset == 0)
        what = f"M={M} n={nn} {kind} offset={offset} {route}"
        if route == "composed":
            with _composed():
                assert lib.dfft_rconv1d_fused_applies(nn, m, CODE[prec], KIND[kind], vec) == 0
                _raw(xv.data_ptr(), ov.data_ptr(), hv.data_ptr(), nn, m, channels, batch, prec, kind)
        else:
            assert lib.dfft_rconv1d_fused_applies(nn, m, CODE[prec], KIND[kind], vec) == int(M == 64)
            _raw(xv.data_ptr(), ov.data_ptr(), hv.data_ptr(), nn, m, channels, batch, prec, kind)
        torch.cuda.synchronize()
        MC.guards_intact(ob, ov, what + " out")
        assert MC.bits_equal(xb, xkeep), what + ": in (or its guards) was written"
        assert MC.bits_equal(hb, hkeep), what + ": h (or its guards) was written"
        _check(RC.nu_rows(ov.cpu().numpy().reshape(rows, nn), ref, m, prec), prec, what)
        # exactly in place, on the guarded input buffer
        if route == "composed":
            with _composed():
                _raw(xv.data_ptr(), xv.data_ptr(), hv.data_ptr(), nn, m, channels, batch, prec, kind)
        else:
            _raw(xv.data_ptr(), xv.data_ptr(), hv.data_ptr(), nn, m, channels, batch, prec, kind)
        torch.cuda.synchronize()
        MC.guards_intact(xb, xv, what + " in place")
        assert MC.bits_equal(xv, ov), what + ": in place differs from out of place"
        assert MC.bits_equal(hb, hkeep)


# ---- a call sequence --------------------------------------------------------------------------------------------------------------------
def test_call_sequence_with_trim(gpu):
    """Four calls on one stream with n, m, channels, precision and route changing between them, dfft_trim, one more call on the composed
    route (whose scratch the trim freed): every result is right."""
    import torch
    lib = _lib()
    st = torch.cuda.Stream(gpu)
    # (M, n, channels, kind, prec, composed by the switch)
    seq = [(64, 100, 3, "complex", "f64", False), (36, 72, 1, "complex", "f64", False), (512, 511, 3, "real", "f32", False),
           (64, 64, 3, "complex", "f64", True)]
    last = (36, 35, 3, "real", "f32", False)

    def enqueue(M, n, channels, kind, prec, off):
        batch = RC.batch_for(M, channels)
        x, H, ref = RC.case(M, n, channels, batch, kind)
        xt = torch.from_numpy(x).to(_rdt(prec)).to(gpu)
        Ht = _filter(H, prec, kind, gpu)
        o = torch.empty_like(xt)
        st.wait_stream(torch.cuda.current_stream(gpu))
        want_fused = int(M in RC.TUNED_HALVES and not off)
        if off:
            with _composed():
                assert lib.dfft_rconv1d_fused_applies(n, 2 * M, CODE[prec], KIND[kind], 0) == want_fused
                _raw(xt.data_ptr(), o.data_ptr(), Ht.data_ptr(), n, 2 * M, channels, batch, prec, kind, st.cuda_stream)
        else:
            assert lib.dfft_rconv1d_fused_applies(n, 2 * M, CODE[prec], KIND[kind], 0) == want_fused
            _raw(xt.data_ptr(), o.data_ptr(), Ht.data_ptr(), n, 2 * M, channels, batch, prec, kind, st.cuda_stream)
        return (xt, Ht, o, ref, 2 * M, prec, f"sequence M={M} n={n} channels={channels} {kind}" + (" switched off" if off else ""))

    runs = [enqueue(*c) for c in seq]
    st.synchronize()
    for _, _, o, ref, m, prec, what in runs:
        _check(RC.nu_rows(o.cpu().numpy(), ref, m, prec), prec, what)
    assert lib.dfft_trim() == 0
    _, _, o, ref, m, prec, what = enqueue(*last)
    st.synchronize()
    _check(RC.nu_rows(o.cpu().numpy(), ref, m, prec), prec, what + " after dfft_trim")
