"""Long 1-D real FFT convolution (dfft_rconv1d_long, api.rconv1d_long / api.fftconv1d_long) on the GPU against numpy float64,
irfft(rfft(x, m) * H, m)[:n] (tests/rconv1d_long_cases.py): the four splits of rconv1d_long_cases.SPLITS, n = m, m/2, m/2 + 1, 2 N2 + 6,
5 and 1, three row shapes, both precisions and both filter kinds -- out of place, in place, on buffers offset by one real, and on the
composed route (DFFT_RCONV_LONG_FUSED=0) -- the filter permutation, the identity filter, fftconv1d_long against numpy.convolve, a call
of several chunks, a call sequence with dfft_trim in it, and the rounding error in eps units.

Pass mark of the sweep: max |got - ref| / max |ref| below 1e-11 (fp64) / 5e-4 (fp32).
Accuracy in eps units (accuracy_ref.nu per row, n_eff = m, longdouble references): measured values and bounds in rconv1d_long_cases."""
import ctypes as C
import os

import numpy as np
import pytest

import accuracy_ref as A
import mem_contract as MC
import rconv1d_long_cases as LC

pytestmark = pytest.mark.gpu

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


def _raw(inp, out, hp, n, m, channels, batch, prec, kind, stream=None):
    from distributedfft_amd import _lib as L
    L.check(_lib().dfft_rconv1d_long(C.c_void_p(inp), C.c_void_p(out), C.c_void_p(hp), n, m, channels, batch, CODE[prec], KIND[kind],
                                     C.c_void_p(stream) if stream else None), "dfft_rconv1d_long")


class _composed:
    """DFFT_RCONV_LONG_FUSED=0 for the calls inside (the library reads it per call)"""

    def __enter__(self):
        self.old = os.environ.get("DFFT_RCONV_LONG_FUSED")
        os.environ["DFFT_RCONV_LONG_FUSED"] = "0"

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("DFFT_RCONV_LONG_FUSED", None)
        else:
            os.environ["DFFT_RCONV_LONG_FUSED"] = self.old


def _rel(got, ref):
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / np.abs(ref).max())


def _check(got, ref, prec, what):
    e = _rel(got, ref)
    print(f"rconv1d_long {prec} {what}: rel {e:.3e}")
    assert e < LC.BOUND_REL[prec], (prec, what, e, LC.BOUND_REL[prec])


# ---- the sweep --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LC.KINDS)
@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("m", LC.LENGTHS)
def test_against_numpy(gpu, m, prec, kind):
    """Every n and row shape: out of place (in untouched), in place, input and output one real past a 16-byte boundary in guarded
    buffers, and the composed route -- all within the pass mark of the reference, the routes within it of each other."""
    import torch
    from distributedfft_amd import api
    lib = _lib()
    assert lib.dfft_rconv1d_long_fused_applies(m, CODE[prec]) == 1
    for batch, channels in LC.ROWS:
        rows = batch * channels
        for n in LC.n_values(m):
            x, H, ref = LC.case(m, n, channels, batch, kind)
            what = f"m={m} n={n} batch={batch} channels={channels} {kind}"
            xt = torch.from_numpy(x).to(_rdt(prec)).to(gpu).reshape(batch, channels, n)
            Hp = api.rconv1d_long_filter(_filter(H, prec, kind, gpu))
            keep = xt.clone()
            got = api.rconv1d_long(xt, Hp)
            assert torch.equal(xt, keep), "in was written"
            g = got.cpu().numpy().reshape(rows, n)
            _check(g, ref, prec, what + " fused")
            y = xt.clone()
            assert api.rconv1d_long(y, Hp, m, out=y) is y
            assert MC.bits_equal(y, got), ("in place differs from out of place", what)
            # one real past a 16-byte boundary: per-real accesses
            xb, xv = MC.guarded(rows * n, _rdt(prec), gpu, 1, n)
            ob, ov = MC.guarded(rows * n, _rdt(prec), gpu, 1, n)
            xv.copy_(xt.reshape(-1))
            xkeep = xb.clone()
            _raw(xv.data_ptr(), ov.data_ptr(), Hp.data_ptr(), n, m, channels, batch, prec, kind)
            torch.cuda.synchronize()
            MC.guards_intact(ob, ov, what + " offset out")
            assert MC.bits_equal(xb, xkeep), what + ": in (or its guards) was written"
            _check(ov.cpu().numpy().reshape(rows, n), ref, prec, what + " offset by one real")
            with _composed():
                assert lib.dfft_rconv1d_long_fused_applies(m, CODE[prec]) == 0
                comp = api.rconv1d_long(xt, Hp, m)
                z = xt.clone()
                api.rconv1d_long(z, Hp, m, out=z)
            c = comp.cpu().numpy().reshape(rows, n)
            _check(c, ref, prec, what + " composed")
            _check(z.cpu().numpy().reshape(rows, n), ref, prec, what + " composed in place")
            e = float(np.abs(g.astype(np.float64) - c).max() / np.abs(ref).max())
            assert e < LC.BOUND_REL[prec], ("fused against composed", what, e)


# ---- every factor length ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", LC.FACTORS)
def test_every_factor_length_runs_its_kernels(gpu, N):
    """m = 2 N^2 splits into (N, N): the pass A / pass C and the Mid kernels of N (64, which is never the longer factor: (64, 80)) -- one
    row with an even n (two-real accesses) and an odd one (per-real), fp64 with a complex filter and fp32 with a real one."""
    import torch
    from distributedfft_amd import api
    m = 2 * N * max(N, 80)
    assert LC.split(m) == (N, max(N, 80))
    for n in (m // 2 + 2, m // 2 + 1):
        x = A.rand_real((1, n), 35000 + N + n)
        for prec, kind in (("f64", "complex"), ("f32", "real")):
            H = LC.make_filter(1, m, kind, 36000 + N)
            ref = LC.reference64(x, H, m)
            assert _lib().dfft_rconv1d_long_fused_applies(m, CODE[prec]) == 1
            xt = torch.from_numpy(x).to(_rdt(prec)).to(gpu).reshape(1, 1, n)
            got = api.rconv1d_long(xt, api.rconv1d_long_filter(_filter(H, prec, kind, gpu)))
            _check(got.cpu().numpy().reshape(1, n), ref, prec, f"N1=N2={N} m={m} n={n} {kind}")


# ---- the filter -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", LC.LENGTHS)
def test_filter_permutation_is_exact(gpu, m):
    import torch
    from distributedfft_amd import api
    n1, n2 = LC.SPLITS[m]
    a, b = C.c_int(0), C.c_int(0)
    assert _lib().dfft_rconv1d_long_split(m, C.byref(a), C.byref(b)) == 1 and (a.value, b.value) == (n1, n2)
    for prec in A.PRECS:
        for kind in LC.KINDS:
            H = LC.make_filter(3, m, kind, 31000 + m)
            Ht = _filter(H, prec, kind, gpu)
            keep = Ht.clone()
            Hp = api.rconv1d_long_filter(Ht, m)
            assert Hp.shape == Ht.shape and Hp.dtype == Ht.dtype and torch.equal(Ht, keep)
            assert np.array_equal(Hp.cpu().numpy(), LC.permute_filter(Ht.cpu().numpy(), n1, n2)), (m, prec, kind)


@pytest.mark.parametrize("prec", A.PRECS)
def test_unit_filter_is_the_identity(gpu, prec):
    import torch
    from distributedfft_amd import api
    for m in LC.LENGTHS:
        for n in (m, m // 2 + 1):
            x = torch.from_numpy(A.rand_real((2, 3, n), 32000 + m)).to(_rdt(prec)).to(gpu)
            for dt in (_rdt(prec), _cdt(prec)):
                H = torch.ones((3, m // 2 + 1), dtype=dt, device=gpu)
                y = api.rconv1d_long(x, api.rconv1d_long_filter(H))
                assert float((y - x).abs().max()) < LC.BOUND_REL[prec] * float(x.abs().max()), (m, n, dt)


# ---- fftconv1d_long ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("n,taps", [(6000, 6000), (9000, 4000)])
def test_fftconv1d_long_is_numpy_convolve(gpu, n, taps, prec):
    import torch
    from distributedfft_amd import api
    channels, batch = 2, 2
    x = A.rand_real((batch, channels, n), 33000 + n)
    k = A.rand_real((channels, taps), 34000 + taps)
    ref = np.stack([np.stack([np.convolve(x[b, c], k[c])[:n] for c in range(channels)]) for b in range(batch)])
    xt = torch.from_numpy(x).to(_rdt(prec)).to(gpu)
    kt = torch.from_numpy(k).to(_rdt(prec)).to(gpu)
    m = api.rconv1d_long_length(n + taps - 1)
    assert m >= n + taps - 1 and LC.split(m) is not None
    got = api.fftconv1d_long(xt, kt)
    assert got.shape == xt.shape and got.dtype == xt.dtype
    _check(got.cpu().numpy().reshape(-1, n), ref.reshape(-1, n), prec, f"fftconv1d_long n={n} taps={taps} m={m}")
    y = xt.clone()
    assert api.fftconv1d_long(y, kt, out=y) is y and MC.bits_equal(y, got)
    with pytest.raises(ValueError, match="fftconv1d"):
        api.fftconv1d_long(torch.zeros((1, 1, 4000), dtype=_rdt(prec), device=gpu), torch.zeros((1, 100), dtype=_rdt(prec), device=gpu))
    with pytest.raises(ValueError):
        api.fftconv1d_long(torch.zeros((1, 1, 8), dtype=_rdt(prec), device=gpu), torch.zeros((1, 1 << 23), dtype=_rdt(prec), device=gpu))


# ---- several chunks ---------------------------------------------------------------------------------------------------------------------
def test_several_chunks_give_the_rows_of_one(gpu):
    """m = 16384 in fp64: 128 KiB of scratch per row, 2048 rows per chunk.  2055 rows (a ragged second chunk of 7, filter rows that
    do not start at 0 there) repeat the rows of a single-chunk call, whose results they must equal row by row."""
    import torch
    from distributedfft_amd import api
    m, n, channels, base = 16384, 8193, 3, 2
    lib = _lib()
    batch = 685                                            # 2055 rows
    rows = batch * channels
    assert lib.dfft_rconv1d_long_scratch_bytes(n, m, channels, batch, 0) == 2048 * (m // 2) * 16 < rows * (m // 2) * 16
    assert rows * (m // 2) * 16 < 300 << 20
    x, H, ref = LC.case(m, n, channels, base, "complex")
    xt = torch.from_numpy(x).to(gpu).reshape(base, channels, n)
    Hp = api.rconv1d_long_filter(_filter(H, "f64", "complex", gpu))
    one = api.rconv1d_long(xt, Hp)
    _check(one.cpu().numpy().reshape(-1, n), ref, "f64", "several chunks: the base rows")
    reps = -(-batch // base)
    big = xt.repeat(reps, 1, 1)[:batch].contiguous()
    got = api.rconv1d_long(big, Hp)
    want = one.repeat(reps, 1, 1)[:batch]
    assert torch.equal(got, want), "rows of a later chunk differ from the single-chunk result"


# ---- a call sequence --------------------------------------------------------------------------------------------------------------------
def test_call_sequence_with_trim(gpu):
    """Two different m back to back on one stream, dfft_trim, one more call (whose scratch the trim freed): every result is right."""
    import torch
    from distributedfft_amd import api
    lib = _lib()
    st = torch.cuda.Stream(gpu)

    def enqueue(m, n, channels, batch, kind, prec):
        x, H, ref = LC.case(m, n, channels, batch, kind)
        xt = torch.from_numpy(x).to(_rdt(prec)).to(gpu)
        Hp = api.rconv1d_long_filter(_filter(H, prec, kind, gpu))
        o = torch.empty_like(xt)
        st.wait_stream(torch.cuda.current_stream(gpu))
        _raw(xt.data_ptr(), o.data_ptr(), Hp.data_ptr(), n, m, channels, batch, prec, kind, st.cuda_stream)
        return xt, Hp, o, ref, prec, f"sequence m={m} n={n} {kind}"

    runs = [enqueue(16384, 16384, 3, 2, "complex", "f64"), enqueue(31250, 15626, 2, 5, "real", "f32")]
    st.synchronize()
    for _, _, o, ref, prec, what in runs:
        _check(o.cpu().numpy(), ref, prec, what)
    assert lib.dfft_trim() == 0
    _, _, o, ref, prec, what = enqueue(20736, 5, 3, 2, "complex", "f64")
    st.synchronize()
    _check(o.cpu().numpy(), ref, prec, what + " after dfft_trim")


# ---- accuracy in eps units --------------------------------------------------------------------------------------------------------------
_NU = {}


def _measure(gpu):
    """Worst nu per (route, precision) over LC.acc_cases(), rows of more than one sample and rows of one sample apart; the CPU pipeline is
    the same-precision scipy.fft (numpy computes float32 transforms in double)."""
    if _NU:
        return _NU
    import torch
    from distributedfft_amd import api
    try:
        import scipy.fft as sf
    except ImportError:   # pragma: no cover
        sf = None
    batch, channels = LC.ACC_ROWS
    for m, n, kind in LC.acc_cases():
        x, H, ref = LC.acc_case(m, n, kind)
        for prec in A.PRECS:
            xt = torch.from_numpy(x).to(_rdt(prec)).to(gpu).reshape(batch, channels, n)
            Hp = api.rconv1d_long_filter(_filter(H, prec, kind, gpu))
            res = {"fused": api.rconv1d_long(xt, Hp).cpu().numpy().reshape(-1, n)}
            with _composed():
                res["composed"] = api.rconv1d_long(xt, Hp).cpu().numpy().reshape(-1, n)
            if sf is not None or prec == "f64":
                mod = sf if sf is not None else np.fft
                Hc = H.astype(A.RDT[prec] if kind == "real" else A.CDT[prec])[np.arange(x.shape[0]) % channels]
                res["cpu"] = mod.irfft(mod.rfft(x.astype(A.RDT[prec]), m, axis=1) * Hc, m, axis=1)[:, :n]
            for route, g in res.items():
                v = LC.nu_rows(g, ref, m, prec)
                print(f"rconv1d_long nu {route} {prec} m={m} n={n} {kind}: {v:.3f}")
                key = (route, prec, n == 1)
                if v > _NU.get(key, (-1.0, ""))[0]:
                    _NU[key] = (v, f"m={m} n={n} {kind}")
            v = LC.nu_rows(res["fused"], res["composed"].astype(A.LD), m, prec)
            key = ("fused-composed", prec, n == 1)
            if v > _NU.get(key, (-1.0, ""))[0]:
                _NU[key] = (v, f"m={m} n={n} {kind}")
    return _NU


@pytest.mark.parametrize("prec", A.PRECS)
def test_accuracy_in_eps_units(gpu, prec):
    nu = _measure(gpu)
    for key in sorted(nu):
        if key[1] == prec:
            print(f"rconv1d_long worst nu {key[0]} {prec} {'n = 1' if key[2] else 'n > 1'}: {nu[key][0]:.3f}  ({nu[key][1]})")
    for single, bound in ((False, LC.BOUND[prec]), (True, LC.BOUND_N1[prec])):
        assert bound is not None, "no bound recorded"
        for route in ("fused", "composed", "fused-composed"):
            v, what = nu[(route, prec, single)]
            assert v <= bound, (route, prec, what, v, bound)
