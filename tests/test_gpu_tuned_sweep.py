"""-m gpu: every tuned-length instantiation of the fused kernel families, launched once.

Nine kernel families are instantiated per entry of DFFT_PLAN_TABLE, per precision and per template variant, each with its own geometry;
the family modules run a handful of lengths each.  Here every (family, length) is one test id that runs both precisions and every
variant (forward / backward, two-real and per-real accesses, rows / columns, filter kind, pad mode, output kind) of tests/tuned_sweep.py
through the family's public entry point, against the longdouble reference, and judges every transformed line with accuracy_ref.nu.

The cap is a condition, not a fitted bound: accuracy_ref.CEILING of the family ("real", "r2r", "bluestein"; the STFT takes "real", twice
that for power output, as test_gpu_stft.py does) and the BOUND of test_gpu_rconv1d.py / test_gpu_rconv1d_os.py for the two convolutions.
A dropped or misplaced point, a wrong twiddle or a wrong pairing partner puts nu many orders of magnitude above any of them.  Every case
asserts the route it is there for (tuned_sweep.ROUTED: the composed form at the few instantiations the route rules send there) before it
runs, and that its input comes back bit-identical.  No environment switch is used, except in test_composed_route_next_to_a_spilling_length.
Every nu is printed; the worst per (family, precision) when the module's last test has run.  Buffer guards: the mem-contract modules.

Cases that measure above the family's accuracy_ref.BOUND (2 x the worst of the few lengths measured before) but under the ceiling pass
and are printed as "above BOUND".  Seen on an MI355X, all fp32 at n = 3 (a column of two bins), also in DESIGN.md, "Tuned-length sweep":
    real columns  rfft s = 6 0.864, rfft s = 34 0.906, irfft s = 6 0.918, irfft s = 7 1.516      (BOUND 0.84, ceiling 3.2)
    r2r           dst2 s = 6 1.122                                                                (BOUND 1.1, ceiling 4.4)
Worst nu per family (fp64 / fp32): real rows 0.473 / 0.534, row pairs 0.562 / 0.665, real columns 0.766 / 1.516, r2r 1.134 / 1.122,
Bluestein 0.946 / 0.724, rconv1d 2.946 / 3.302, overlap-save 1.548 / 0.929, STFT 1.261 / 1.682 (both power output).  No instantiation
computes a wrong result.  346 test ids, 8.4 s in all."""
import ctypes as C
import os

import numpy as np
import pytest

import accuracy_ref as A
import rconv1d_cases as RC
import rconv1d_os_cases as RCO
import stft_cases as SC
import tuned_sweep as TS
from test_gpu_rconv1d import BOUND as RCONV_BOUND
from test_gpu_rconv1d_os import BOUND as OSCONV_BOUND

pytestmark = pytest.mark.gpu
FWD, BWD = +1, -1
WORST = {}
ABOVE = []


@pytest.fixture(scope="module", autouse=True)
def _print_the_worst_nu_per_family():
    yield
    for (family, prec), (value, what) in sorted(WORST.items()):
        print(f"tuned sweep worst {family} {prec}: nu {value:.3f}  ({what})")
    for line in ABOVE:
        print("tuned sweep above BOUND: " + line)


@pytest.fixture(autouse=True)
def _no_route_switch(monkeypatch):
    for name in ("DFFT_R2R_FUSED", "DFFT_RCONV_FUSED", "DFFT_STFT_FUSED", "DFFT_BLUESTEIN_FUSED"):
        monkeypatch.delenv(name, raising=False)


def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


def _rdt(prec):
    import torch
    return torch.float64 if prec == "f64" else torch.float32


def _cdt(prec):
    import torch
    return torch.complex128 if prec == "f64" else torch.complex64


def _gpu(x, prec, gpu):
    """numpy (float32-exact values) -> a device tensor of the working precision (a copy: the shared inputs are read-only)"""
    import torch
    t = torch.from_numpy(np.array(x, order="C")).to(gpu)
    return t.to(_cdt(prec) if t.is_complex() else _rdt(prec))


def _run(call, xt):
    """call(xt) -> numpy, with the input bit-identical afterwards"""
    import torch
    keep = xt.clone()
    got = call(xt)
    assert torch.equal(torch.view_as_real(xt) if xt.is_complex() else xt, torch.view_as_real(keep) if keep.is_complex() else keep), "in was written"
    return got.cpu().numpy()


def _check(family, prec, value, cap, what, bound=None):
    print(f"tuned sweep {family} {prec} {what}: nu {value:.3f}")
    if value > WORST.get((family, prec), (-1.0, ""))[0]:
        WORST[(family, prec)] = (value, what)
    if bound is not None and bound < value <= cap:
        ABOVE.append(f"{family} {prec} {what}: nu {value:.3f} (BOUND {bound}, ceiling {cap})")
    assert value <= cap, (family, prec, what, value, cap)


# ---- real rows --------------------------------------------------------------------------------------------------------------------------
def _real_rows(gpu, family, n, form, scaled):
    from distributedfft_amd import api
    assert api.real_form(n) == form
    x, F, X, b = TS.real_rows_case(n, scaled)
    for prec in TS.PRECS:
        cap, bound = A.CEILING["real"][prec], A.BOUND["real"][prec]
        _check(family, prec, A.nu(_run(api.rfft1d, _gpu(x, prec, gpu)), F, n, prec, (1,)), cap, f"rfft n={n} rows={TS.ROWS}", bound)
        _check(family, prec, A.nu(_run(lambda t: api.irfft1d(t, n), _gpu(X, prec, gpu)), b, n, prec, (1,)), cap, f"irfft n={n} rows={TS.ROWS}", bound)


@pytest.mark.parametrize("M", TS.LENGTHS["real_rows"])
def test_real_rows(gpu, M):
    """dfft_rfft1d on n = 2 M (form 1, the half-length kernels), five rows under different scales, both directions"""
    _real_rows(gpu, "real_rows", 2 * M, 1, True)


@pytest.mark.parametrize("n", TS.LENGTHS["real_pair"])
def test_real_pair(gpu, n):
    """dfft_rfft1d on odd tuned n (form 2, two rows per transform), five rows: the last has no partner"""
    _real_rows(gpu, "real_pair", n, 2, False)


# ---- real columns -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", TS.LENGTHS["real_cols"])
def test_real_cols(gpu, n):
    from distributedfft_amd import api
    lib = _lib()
    for s in TS.real_cols_s(n):
        x, F, X, b = TS.real_cols_case(n, s)
        for prec in TS.PRECS:
            fused = TS.route("real_cols", n, prec, s) == "fused"
            assert lib.dfft_rfft_cols_fused_applies(n, s, TS.CODE[prec]) == int(fused), (n, s, prec)
            assert (lib.dfft_rfft1d_strided_scratch_bytes(n, s, 2, TS.CODE[prec]) == 0) == fused, (n, s, prec)
            cap, bound, tag = A.CEILING["real"][prec], A.BOUND["real"][prec], "fused" if fused else "composed"
            _check("real_cols", prec, A.nu(_run(lambda t: api.rfft1d(t, dim=1), _gpu(x, prec, gpu)), F, n, prec, (1,)), cap, f"rfft n={n} s={s} {tag}", bound)
            _check("real_cols", prec, A.nu(_run(lambda t: api.irfft1d(t, n, dim=1), _gpu(X, prec, gpu)), b, n, prec, (1,)), cap,
                   f"irfft n={n} s={s} {tag}", bound)


# ---- DCT / DST --------------------------------------------------------------------------------------------------------------------------
def _r2r_length(gpu, n, composed=False):
    import torch
    from distributedfft_amd import api
    lib = _lib()
    for form, s in TS.R2R_FORMS.items():
        case = TS.r2r_case(n, s)
        vec = int(form == "cols_vec")
        for prec in TS.PRECS:
            xt = _gpu(case[0], prec, gpu)
            assert xt.data_ptr() % 16 == 0
            for kind, ref in zip(A.R2R_KINDS, case[1:]):
                fused = not composed and TS.route("r2r", n, prec, TS.R2R_THREE[kind], form) == "fused"
                assert lib.dfft_r2r_fused_applies(n, s, TS.CODE[prec], TS.R2R_CODE[kind], vec) == int(fused), (n, s, prec, kind)
                assert (lib.dfft_r2r1d_strided_scratch_bytes(n, s, 2, TS.CODE[prec], TS.R2R_CODE[kind], vec) == 0) == fused, (n, s, prec, kind)
                tag = "fused" if fused else "composed"
                got = _run(lambda t: api.r2r(t, kind, dim=1), xt)
                _check("r2r", prec, A.nu(got, ref, n, prec, (1,)), A.CEILING["r2r"][prec], f"{kind} n={n} s={s} {tag}", A.BOUND["r2r"][prec])
                if kind == "dst3" and not composed:      # in place, once per (n, form): bit-identical to out of place
                    y = xt.clone()
                    assert api.r2r(y, kind, dim=1, out=y) is y
                    assert np.array_equal(y.cpu().numpy(), got), ("in place differs from out of place", n, s, prec, kind)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", TS.LENGTHS["r2r"])
def test_r2r(gpu, n):
    """All four kinds on [2][n][s]: s = 1 (rows), 6 (column pairs as one value), 7 (two reals, an odd last column)"""
    _r2r_length(gpu, n)


# ---- Bluestein --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", TS.LENGTHS["bluestein"])
def test_bluestein(gpu, M):
    """The fused Bluestein kernels on the padded length M: fft1d_any of the largest non-smooth n <= 2048 that pads to M, on [3][n] (rows
    kernel) and [2][n][3] (cols kernel), both directions"""
    from distributedfft_amd import api
    lib = _lib()
    n, both = TS.bluestein_cases(M)
    assert api.length_kind(n) == 3 and api.bluestein_length(n) == M
    for shape, axis, x, F in both:
        s = int(np.prod(shape[axis + 1:]))
        assert lib.dfft_bluestein_fused_applies(n, s) == 1, (n, s)
        for prec in TS.PRECS:
            assert lib.dfft_fft1d_any_scratch_bytes(n, s, shape[0], TS.CODE[prec]) == 0
            xt = _gpu(x, prec, gpu)
            cap, bound = A.CEILING["bluestein"][prec], A.BOUND["bluestein"][prec]
            _check("bluestein", prec, A.nu(_run(lambda t: api.fft1d_any(t, axis, FWD), xt), F, n, prec, (axis,)), cap, f"M={M} n={n} s={s} fwd", bound)
            _check("bluestein", prec, A.nu(_run(lambda t: api.fft1d_any(t, axis, BWD), xt), A.reverse_bins(F, [axis]), n, prec, (axis,)), cap,
                   f"M={M} n={n} s={s} bwd", bound)


# ---- rconv1d ----------------------------------------------------------------------------------------------------------------------------
def _filter(H, prec, kind, gpu):
    import torch
    return torch.from_numpy(np.array(H, order="C")).to(_rdt(prec) if kind == "real" else _cdt(prec)).to(gpu)


def _rconv_length(gpu, M, composed=False):
    from distributedfft_amd import api
    lib, m = _lib(), 2 * M
    for n, kind, batch in TS.rconv_cases(M):
        x, H, ref = RC.case(M, n, TS.RCONV_CHANNELS, batch, kind)
        for prec in TS.PRECS:
            fused = not composed and TS.route("rconv", M, prec) == "fused"
            assert lib.dfft_rconv1d_fused_applies(n, m, TS.CODE[prec], TS.FILTER_CODE[kind], int(n % 2 == 0)) == int(fused), (M, n, prec)
            assert (lib.dfft_rconv1d_scratch_bytes(n, m, TS.RCONV_CHANNELS, batch, TS.CODE[prec]) == 0) == fused, (M, n, prec)
            xt = _gpu(x, prec, gpu).reshape(batch, TS.RCONV_CHANNELS, n)
            Ht = _filter(H, prec, kind, gpu)
            got = _run(lambda t: api.rconv1d(t, Ht, m), xt).reshape(batch * TS.RCONV_CHANNELS, n)
            _check("rconv", prec, RC.nu_rows(got, ref, m, prec), RCONV_BOUND[prec], f"M={M} n={n} batch={batch} {kind} {'fused' if fused else 'composed'}")


@pytest.mark.parametrize("M", TS.LENGTHS["rconv"])
def test_rconv1d(gpu, M):
    """m = 2 M, three channels: n = m (two reals per access, circular) and an odd n (per-real accesses, the cut inside a pair), both filters"""
    _rconv_length(gpu, M)


# ---- overlap-save -----------------------------------------------------------------------------------------------------------------------
def _osconv_length(gpu, M, composed=False):
    from distributedfft_amd import api
    lib, m = _lib(), 2 * M
    for d, n, n_out, channels, batch, kind in TS.osconv_cases(M):
        x, H, ref = RCO.case(M, d, n, n_out, channels, batch, kind)
        for prec in TS.PRECS:
            fused = not composed and TS.route("osconv", M, prec) == "fused"
            assert lib.dfft_rconv1d_os_fused_applies(m, TS.CODE[prec]) == int(fused), (M, prec)
            assert (lib.dfft_rconv1d_os_scratch_bytes(n_out, m, d, channels, batch, TS.CODE[prec]) == 0) == fused, (M, d, n, prec)
            xt = _gpu(x, prec, gpu).reshape(batch, channels, n)
            Ht = _filter(H, prec, kind, gpu)
            got = _run(lambda t: api.rconv1d_os(t, Ht, m, d, n_out), xt).reshape(batch * channels, n_out)
            _check("osconv", prec, RCO.nu_rows(got, ref, m, prec), OSCONV_BOUND[prec],
                   f"M={M} d={d} n={n} {kind} {'vec' if TS.osconv_vec(d, n) else 'scalar'} {'fused' if fused else 'composed'}")


@pytest.mark.parametrize("M", TS.LENGTHS["osconv"])
def test_rconv1d_os(gpu, M):
    """m = 2 M, three channels, batch 2: d = M with a ragged last block, an odd d, an all-even case where the first is not; both filters"""
    _osconv_length(gpu, M)


# ---- STFT -------------------------------------------------------------------------------------------------------------------------------
def _stft_length(gpu, M, composed=False):
    import torch
    from distributedfft_amd import _lib as L
    lib, m = _lib(), 2 * M
    for shape, mode, kind in TS.stft_cases(M):
        _, hop, pad, n, wkind = shape
        x, win, frames, ref = SC.forward_case(M, hop, pad, n, wkind, mode)
        want = SC.power(ref) if kind == "power" else ref
        rows = x.shape[0]
        for prec in TS.PRECS:
            fused = not composed and TS.route("stft", M, prec) == "fused"
            assert lib.dfft_stft1d_fused_applies(m, TS.CODE[prec]) == int(fused), (M, prec)
            assert (lib.dfft_stft1d_scratch_bytes(m, frames, rows, TS.CODE[prec], SC.KIND_CODE[kind]) == 0) == fused, (M, prec)
            xt, wt = _gpu(x, prec, gpu), _gpu(win, prec, gpu)
            out = torch.empty((rows, frames, M + 1), dtype=_rdt(prec) if kind == "power" else _cdt(prec), device=gpu)

            def call(t):
                L.check(lib.dfft_stft1d(C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(wt.data_ptr()), n, m, hop, pad, frames, rows,
                                        TS.CODE[prec], SC.MODE_CODE[mode], SC.KIND_CODE[kind], 1.0, None), "dfft_stft1d")
                torch.cuda.synchronize()
                return out
            got = _run(call, xt)
            cap = A.CEILING["real"][prec] * (2.0 if kind == "power" else 1.0)
            _check("stft", prec, SC.nu_frames(got, want, m, prec), cap,
                   f"M={M} hop={hop} pad={pad} n={n} {mode} {kind} {'vec' if TS.stft_vec(shape) else 'scalar'} {'fused' if fused else 'composed'}")


@pytest.mark.parametrize("M", TS.LENGTHS["stft"])
def test_stft(gpu, M):
    """n_fft = 2 M: the base case of stft_cases, an odd hop, an all-even case where the base is not; both pad modes and output kinds"""
    _stft_length(gpu, M)


# ---- the composed route next to the lengths that are routed because their fused kernels would spill -------------------------------------
@pytest.mark.parametrize("family", sorted(TS.COMPOSED_NEIGHBOUR))
def test_composed_route_next_to_a_spilling_length(gpu, family, monkeypatch):
    """The routed (length, precision) of these families run the composed form above; here a neighbouring fused length runs it too, under
    the family's switch, against the same references and caps"""
    switch, n = TS.COMPOSED_NEIGHBOUR[family]
    monkeypatch.setenv(switch, "0")
    assert os.environ[switch] == "0"
    {"r2r": _r2r_length, "rconv": _rconv_length, "osconv": _osconv_length, "stft": _stft_length}[family](gpu, n, composed=True)
