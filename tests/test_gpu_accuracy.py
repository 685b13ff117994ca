"""-m gpu: the rounding error of every transform, in units of eps * sqrt(log2 n), against longdouble references (tests/accuracy_ref.py).

The other GPU tests hold max|got - ref| / max|ref| below 1e-11 (fp64) / 5e-4 (fp32) against float64 numpy: four to five orders of
magnitude above what a correct FFT delivers, and blind to one bad line among good ones.  Here every transformed LINE (a row or column of
a 1-D call, a plane of a 2-D call, a rank's output of a 3-D plan) must keep nu = ||got - ref||_2 / ||ref||_2 / (eps sqrt(log2 n_eff))
under BOUND[family][prec]: 2 x the worst nu measured on an MI355X, and never above 8 x the same-precision CPU FFT (CEILING); the table is
in DESIGN.md, "Numerics: measured rounding error".  tests/test_accuracy_host.py proves on three spoiled transforms that these bounds reject
what the old pass mark lets through.

Inputs: seeded standard normals that float32 holds exactly (both precisions share input and reference); on the complex 1-D routes line i
is scaled by 2^s_i, s_i cycling through -8 ... 8, so cross-talk between lines shows on the small line's own norm; unit impulses, whose
transform is known in closed form (nu_impulse = max|got - ref| / eps; the impulse at n - 1 walks a whole twiddle table); one tone.
2^24 points are left out: the longdouble reference alone takes more than a few seconds."""
import numpy as np
import pytest

import accuracy_ref as A
from test_gpu_parity import GENERIC, TUNED, _run_plans

pytestmark = pytest.mark.gpu
FWD, BWD = +1, -1
DIRS = [FWD, BWD]


@pytest.fixture(scope="module", autouse=True)
def _worst_per_family():
    """After the module's last case: the worst nu per family and precision, the figures of DESIGN.md's table."""
    yield
    for (family, prec), (value, what) in sorted(A.WORST.items()):
        print(f"accuracy worst {family} {prec}: nu {value:.3f} (bound {A.BOUND[family][prec]})  {what}")


def _gpu(x, prec, gpu):
    """numpy (complex or real, float32-exact values) -> device tensor of the working precision"""
    import torch
    t = torch.from_numpy(np.array(x, order="C")).to(gpu)   # a copy: the shared inputs are read-only
    if t.is_complex():
        return t.to(torch.complex128 if prec == "f64" else torch.complex64)
    return t.to(torch.float64 if prec == "f64" else torch.float32)


def _host(t):
    return t.cpu().numpy()


def _c1d(gpu, call, family, prec, n, shape, axis, what, base=0, impulses=None, tone=True, inplace=True):
    """One complex 1-D route: `call(tensor, direction, out)` transforms along `axis` of `shape`.  Scaled random lines forward, backward and
    both in place; impulses forward and backward; one tone."""
    x, F = A.complex_lines(n, shape, axis, 1000 + n, base)
    xt = _gpu(x, prec, gpu)
    A.check(family, prec, A.nu(_host(call(xt, FWD, None)), F, n, prec, (axis,)), f"{what} random fwd")
    A.check(family, prec, A.nu(_host(call(xt, BWD, None)), A.reverse_bins(F, [axis]), n, prec, (axis,)), f"{what} random bwd")
    if inplace:
        y = xt.clone()
        call(y, FWD, y)
        A.check(family, prec, A.nu(_host(y), F, n, prec, (axis,)), f"{what} random fwd in place")
        y = xt.clone()
        call(y, BWD, y)
        A.check(family, prec, A.nu(_host(y), A.reverse_bins(F, [axis]), n, prec, (axis,)), f"{what} random bwd in place")
    pos = tuple(A.impulse_positions(n) if impulses is None else impulses)
    d, Fd = A.impulse_lines(n, shape, axis, pos)
    dt = _gpu(d, prec, gpu)
    A.check(family + "-impulse", prec, A.nu_impulse(_host(call(dt, FWD, None)), Fd, prec), f"{what} impulses {pos} fwd")
    A.check(family + "-impulse", prec, A.nu_impulse(_host(call(dt, BWD, None)), np.conj(Fd), prec), f"{what} impulses {pos} bwd")
    if tone:
        t, Ft = A.tone_lines(n, shape, axis, prec)
        A.check(family, prec, A.nu(_host(call(_gpu(t, prec, gpu), FWD, None)), Ft, n, prec, (axis,)), f"{what} tone")


def _family(n):
    return "tuned" if n in TUNED else "generic"


# ---- complex 1-D: every tuned and run-time-scheduled length ----------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("n", TUNED + GENERIC)
def test_rows(gpu, n, prec):
    from distributedfft_amd import api
    _c1d(gpu, lambda t, d, out: api.fft1d_rows(t, d, out=out), _family(n), prec, n, (9, n), 1, f"rows n={n}")


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("width", [32, 21])   # 21: the ragged tile, and the scalar fall-back in fp32
@pytest.mark.parametrize("n", TUNED + GENERIC)
def test_cols(gpu, n, width, prec):
    from distributedfft_amd import api
    _c1d(gpu, lambda t, d, out: api.fft1d_cols(t, d, out=out), _family(n), prec, n, (3, n, width), 1, f"cols n={n} width={width}")


# ---- four-step lengths -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("n", A.FOUR_STEP)
def test_four_step(gpu, n, prec):
    """Rows, and columns of width 4: two random lines under different scales, and the impulse at n - 1 (every entry of the hi x lo table)."""
    from distributedfft_amd import api
    assert api.length_kind(n) == 2
    _c1d(gpu, lambda t, d, out: api.fft1d_rows(t, d, out=out), "four-step", prec, n, (2, n), 1, f"rows n={n}", base=2, impulses=(n - 1,),
         tone=False)
    _c1d(gpu, lambda t, d, out: api.fft1d_cols(t, d, out=out), "four-step", prec, n, (2, n, 4), 1, f"cols n={n} width=4", base=2,
         impulses=(n - 1,), tone=False, inplace=False)


# ---- Bluestein -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("n", A.BLUESTEIN)
def test_bluestein(gpu, n, prec):
    from distributedfft_amd import api
    assert api.length_kind(n) == 3
    _c1d(gpu, lambda t, d, out: api.fft1d_any(t, -1, d, out=out), "bluestein", prec, n, (3, n), 1, f"any n={n} last axis", tone=False)
    _c1d(gpu, lambda t, d, out: api.fft1d_any(t, 1, d, out=out), "bluestein", prec, n, (2, n, 3), 1, f"any n={n} middle axis", tone=False)


# ---- real and real-to-real -------------------------------------------------------------------------------------------------------------
def _real_family(n, name):
    from distributedfft_amd import api
    return name + "-bluestein" if api.length_kind(n) == 3 else name


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("s", A.REAL_S)
@pytest.mark.parametrize("n", A.REAL_N)
def test_rfft_irfft(gpu, n, s, prec):
    """Dim 1 of [2][n][s]; at s = 1 also the contiguous call on the rows of [3][n]."""
    from distributedfft_amd import api
    fam = _real_family(n, "real")
    batch = 3 if s == 1 else 2
    x, F = A.real_lines(n, batch, s, 2000 + n)
    X, b = A.half_spectra(n, batch, s, 3000 + n)
    if s == 1:
        got = _host(api.rfft1d(_gpu(x[:, :, 0], prec, gpu)))[:, :, None]
        back = _host(api.irfft1d(_gpu(X[:, :, 0], prec, gpu), n))[:, :, None]
        A.check(fam, prec, A.nu(got, F, n, prec, (1,)), f"rfft n={n} contiguous")
        A.check(fam, prec, A.nu(back, b, n, prec, (1,)), f"irfft n={n} contiguous")
        x, F, X, b = x[:2], F[:2], X[:2], b[:2]
    got = _host(api.rfft1d(_gpu(x, prec, gpu), dim=1))
    back = _host(api.irfft1d(_gpu(X, prec, gpu), n, dim=1))
    A.check(fam, prec, A.nu(got, F, n, prec, (1,)), f"rfft n={n} s={s}")
    A.check(fam, prec, A.nu(back, b, n, prec, (1,)), f"irfft n={n} s={s}")


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("n1,n2", A.REAL_2D)
def test_rfft2d_irfft2d(gpu, n1, n2, prec):
    from distributedfft_amd import api
    x, F = A.real_planes(n1, n2, 3, 4000 + n1)
    X, b = A.half_planes(n1, n2, 3, 5000 + n1)
    A.check("real", prec, A.nu(_host(api.rfft2d_batch(_gpu(x, prec, gpu))), F, n1 * n2, prec, (1, 2)), f"rfft2 {n1}x{n2}")
    A.check("real", prec, A.nu(_host(api.irfft2d_batch(_gpu(X, prec, gpu), n2)), b, n1 * n2, prec, (1, 2)), f"irfft2 {n1}x{n2}")


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("s", A.REAL_S)
@pytest.mark.parametrize("n", A.REAL_N)
def test_r2r(gpu, n, s, prec):
    from distributedfft_amd import api
    fam = _real_family(n, "r2r")
    case = A.r2r_lines(n, 3 if s == 1 else 2, s, 6000 + n)
    xt = _gpu(case[0], prec, gpu)
    for kind, ref in zip(A.R2R_KINDS, case[1:]):
        A.check(fam, prec, A.nu(_host(api.r2r(xt, kind, dim=1)), ref, n, prec, (1,)), f"{kind} n={n} s={s}")


# ---- 2-D and 3-D complex ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("n1,n2,batch", A.ONE_LAUNCH_2D + A.PLAIN_2D)
def test_fft2d(gpu, n1, n2, batch, prec):
    from distributedfft_amd import api
    fam = "2d-one-launch" if (n1, n2, batch) in A.ONE_LAUNCH_2D else "2d"
    x, F = A.complex_planes(n1, n2, batch, 7000 + n1)
    xt = _gpu(x, prec, gpu)
    A.check(fam, prec, A.nu(_host(api.fft2d_batch(xt, FWD)), F, n1 * n2, prec, (1, 2)), f"fft2 {n1}x{n2}x{batch} fwd")
    A.check(fam, prec, A.nu(_host(api.fft2d_batch(xt, BWD)), A.reverse_bins(F, (1, 2)), n1 * n2, prec, (1, 2)), f"fft2 {n1}x{n2}x{batch} bwd")


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("flags", [0, 1], ids=["fused", "unfused"])
@pytest.mark.parametrize("direction", DIRS, ids=["fwd", "bwd"])
@pytest.mark.parametrize("N,P", A.PLANS_3D)
def test_plan_3d(gpu, N, P, direction, flags, prec):
    """Forward: X slabs of x -> the ranks' [y][z][kx] slabs of fftn(x).  Backward: x read as a spectrum, handed over in that layout ->
    the X slabs of its unnormalised inverse.  One line per rank."""
    x, F = A.complex_volume(N, 8000 + N[0])
    if direction == FWD:
        inputs, refs = A.split_x(x, P), A.split_bins(F, P)
    else:
        inputs, refs = A.split_bins(x, P), A.split_x(A.reverse_bins(F, (0, 1, 2)), P)
    outs, _ = _run_plans(gpu, N, P, prec, None, direction, flags, inputs)
    pairs = [(outs[g][:refs[g].size].reshape(refs[g].shape), refs[g]) for g in range(P)]
    A.check("3d", prec, A.nu_parts(pairs, N[0] * N[1] * N[2], prec), f"plan {N} P={P} {'fwd' if direction > 0 else 'bwd'} flags={flags}")


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("N,P", A.PLANS_R2C)
def test_plan_r2c(gpu, N, P, prec):
    from distributedfft_amd import api
    from test_gpu_r2c import _run
    x, F = A.real_volume(N, 9000 + N[0])
    refs = A.split_bins(F, P)
    outs, _, _ = _run(gpu, N, P, prec, A.split_x(x, P), api.FORWARD)
    pairs = [(outs[g][0][:refs[g].size].reshape(refs[g].shape), refs[g]) for g in range(P)]
    A.check("r2c-3d", prec, A.nu_parts(pairs, N[0] * N[1] * N[2], prec), f"r2c plan {N} P={P}")


# ---- spectral filters ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("real", [False, True], ids=["complex-field", "real-field"])
@pytest.mark.parametrize("N,P", A.PLANS_CONV)
def test_conv(gpu, N, P, real, prec):
    """PlanConv / PlanConvReal with a real filter; n_eff counts both transforms.  PlanConvRealMulti runs the same kernels and is left out."""
    if real:
        from test_gpu_conv_real import _run
    else:
        from test_gpu_conv import _run
    x, H, ref = A.conv_case(N, real, 9500 + N[0])
    outs, _ = _run(gpu, N, P, prec, x, H.astype(A.RDT[prec]))
    pairs = list(zip(A.split_x(outs[0], P), A.split_x(ref, P)))
    A.check("conv", prec, A.nu_parts(pairs, (N[0] * N[1] * N[2]) ** 2, prec), f"conv{'-real' if real else ''} {N} P={P}")
