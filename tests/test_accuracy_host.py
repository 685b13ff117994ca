"""Host side of the accuracy tests (no GPU): the longdouble references of tests/accuracy_ref.py are right; the yardstick -- the
same-precision CPU FFT (scipy.fft) on exactly the inputs of tests/test_gpu_accuracy.py, measured with the same nu -- stays under the
YARDSTICK constants; no BOUND exceeds its CEILING; and the bounds bite: three spoiled transforms that the suite's old pass mark
(max|got - ref| / max|ref| < 1e-11 / 5e-4) lets through are rejected at n = 4096, 8192 and 65536.

Where scipy is missing, fp64 runs against numpy and fp32 is skipped (numpy computes complex64 transforms in double: a flat 0.2 eps that
says nothing).  That is the only skip."""
import numpy as np
import pytest

import accuracy_ref as A
from test_gpu_parity import GENERIC, TUNED
from test_r2r_host import direct

try:
    import scipy.fft as sf
except ImportError:   # pragma: no cover
    sf = None

LD, CLD = A.LD, A.CLD


def _rel_l2(a, b):
    return float(np.sqrt(np.sum(np.abs(a - b) ** 2)) / np.sqrt(np.sum(np.abs(b) ** 2)))


# ---- the reference is right ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 5, 7, 8, 12, 49, 125, 97, 211])
def test_ld_fft_is_the_defining_sum(n):
    x = A.rand_complex((3, n), n).astype(CLD)
    k = np.arange(n, dtype=np.int64)
    for sign in (+1, -1):
        W = A.ld_phase(np.outer(k, k) % n, n, sign)            # [k][j]
        assert W.dtype == CLD
        want = np.einsum("kj,bj->bk", W, x)
        got = A.ld_fft(x, -1, sign)
        assert got.dtype == CLD
        assert _rel_l2(got, want) < 1e-17, (n, sign)
    assert _rel_l2(A.reverse_bins(A.ld_fft(x), [1]), A.ld_fft(x, -1, -1)) < 1e-17
    assert _rel_l2(A.ld_fftn(x.reshape(1, 3, n), (1, 2)), A.ld_fft(A.ld_fft(x, 1), 0).reshape(1, 3, n)) < 1e-17
    # the closed form of the impulses
    d, F = A.impulse_lines(n, (3, n), 1, tuple(A.impulse_positions(n)))
    assert np.abs(A.ld_fft(d, 1) - F).max() < 1e-17 and np.abs(np.abs(F) - 1).max() < 1e-18


@pytest.mark.parametrize("kind", A.R2R_KINDS)
@pytest.mark.parametrize("n", [1, 2, 3, 8, 15, 16, 125])
def test_ld_r2r_is_the_direct_sum(n, kind):
    """against the float64 direct sums of tests/test_r2r_host.py, whose own rounding error is below n eps of the largest output"""
    x = A.rand_real((2, n, 3), n + 1)
    got = A.ld_r2r(x, kind)
    assert got.dtype == LD
    ref = direct(x, kind)
    assert np.abs(got - ref).max() <= 8 * n * 2.0 ** -52 * np.abs(ref).max(), (n, kind)


@pytest.mark.parametrize("n", [2, 3, 8, 15, 16, 125])
def test_ld_real_transforms(n):
    x = A.rand_real((2, n, 3), n + 2)
    X = A.ld_rfft(x, 1)
    assert X.shape == (2, n // 2 + 1, 3) and X.dtype == CLD
    assert np.array_equal(X, A.ld_fft(x.astype(CLD), 1)[:, :n // 2 + 1, :])
    assert np.abs(X - np.fft.rfft(x, axis=1)).max() < 1e-13 * n
    assert np.abs(A.ld_irfft(X, n, 1) - n * x).max() < 1e-16 * n
    Y = A.rand_complex((2, n // 2 + 1, 3), n + 3)        # any input: the imaginary parts of bin 0 and bin n/2 are ignored
    assert np.abs(A.ld_irfft(Y, n, 1) - n * np.fft.irfft(Y, n, axis=1)).max() < 1e-13 * n
    v = A.rand_real((4, 6, n), n + 4)
    H = np.random.default_rng(n).uniform(0.5, 2.0, (4, 6, n // 2 + 1))
    want = np.fft.irfftn(np.fft.rfftn(v) * H, s=v.shape, axes=(0, 1, 2))
    assert np.abs(A.ld_conv(v, H, real=True) - want).max() < 1e-13 * np.abs(want).max()
    c = A.rand_complex((4, 6, n), n + 5)
    Hc = np.random.default_rng(n).uniform(0.5, 2.0, (4, 6, n))
    want = np.fft.ifftn(np.fft.fftn(c) * Hc)
    assert np.abs(A.ld_conv(c, Hc) - want).max() < 1e-13 * np.abs(want).max()


def test_nu_sees_one_bad_line():
    """A line 2^-16 the size of its neighbours that is off by 1e-3 of ITSELF: invisible to the old measure, 1e-3 / eps to nu."""
    x, F = A.complex_lines(64, (17, 64), 1, 1)
    got = np.array(F)
    got[0] *= 1 + LD(1e-3)                                # line 0 carries the scale 2^-8, line 16 the scale 2^8
    assert A.old_measure(got.astype(np.complex128), F.astype(np.complex128)) < 1e-5
    assert A.nu(got, F, 64, "f32", (1,)) > 1e3


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------
def _fft(x, axis, sign, prec):
    x = x.astype(A.CDT[prec])
    if sf is None:
        return np.fft.fft(x, axis=axis) if sign > 0 else np.fft.ifft(x, axis=axis, norm="forward")
    return sf.fft(x, axis=axis) if sign > 0 else sf.ifft(x, axis=axis, norm="forward")


def _fftn(x, axes, sign, prec):
    x = x.astype(A.CDT[prec])
    m = sf if sf is not None else np.fft
    return m.fftn(x, axes=axes) if sign > 0 else m.ifftn(x, axes=axes, norm="forward")


def _record(worst, family, prec, value, what):
    if value > worst.get((family, prec), (-1.0, ""))[0]:
        worst[(family, prec)] = (value, what)


def _c1d(worst, family, prec, n, shape, axis, base=0, impulses=None, tone=True):
    x, F = A.complex_lines(n, shape, axis, 1000 + n, base)
    _record(worst, family, prec, A.nu(_fft(x, axis, +1, prec), F, n, prec, (axis,)), f"n={n} random fwd")
    _record(worst, family, prec, A.nu(_fft(x, axis, -1, prec), A.reverse_bins(F, [axis]), n, prec, (axis,)), f"n={n} random bwd")
    pos = tuple(A.impulse_positions(n) if impulses is None else impulses)
    d, Fd = A.impulse_lines(n, shape, axis, pos)
    _record(worst, family + "-impulse", prec, A.nu_impulse(_fft(d, axis, +1, prec), Fd, prec), f"n={n} impulses fwd")
    _record(worst, family + "-impulse", prec, A.nu_impulse(_fft(d, axis, -1, prec), np.conj(Fd), prec), f"n={n} impulses bwd")
    if tone:
        t, Ft = A.tone_lines(n, shape, axis, prec)
        _record(worst, family, prec, A.nu(_fft(t, axis, +1, prec), Ft, n, prec, (axis,)), f"n={n} tone")


_MEASURED = {}


def _yardsticks():
    """The CPU FFT on every case of tests/test_gpu_accuracy.py, both precisions, case-major so that a reference is computed once."""
    if _MEASURED:
        return _MEASURED
    precs = A.PRECS if sf is not None else ("f64",)
    w = _MEASURED
    for n in TUNED + GENERIC:
        for prec in precs:
            _c1d(w, "tuned" if n in TUNED else "generic", prec, n, (9, n), 1)
            for width in (32, 21):
                _c1d(w, "tuned" if n in TUNED else "generic", prec, n, (3, n, width), 1)
    for n in A.FOUR_STEP:
        for prec in precs:
            _c1d(w, "four-step", prec, n, (2, n), 1, base=2, impulses=(n - 1,), tone=False)   # (the columns repeat these two lines)
    for n in A.BLUESTEIN:
        for prec in precs:
            _c1d(w, "bluestein", prec, n, (3, n), 1, tone=False)
            _c1d(w, "bluestein", prec, n, (2, n, 3), 1, tone=False)
    for n in A.REAL_N:
        blue = "-bluestein" if n == 1009 else ""
        for s in A.REAL_S:
            batch = 3 if s == 1 else 2
            x, F = A.real_lines(n, batch, s, 2000 + n)
            X, b = A.half_spectra(n, batch, s, 3000 + n)
            case = A.r2r_lines(n, batch, s, 6000 + n)
            for prec in precs:
                if sf is not None:
                    got, back = sf.rfft(x.astype(A.RDT[prec]), axis=1), sf.irfft(X.astype(A.CDT[prec]), n, axis=1, norm="forward")
                else:
                    got, back = np.fft.rfft(x, axis=1), np.fft.irfft(X, n, axis=1, norm="forward")
                _record(w, "real" + blue, prec, A.nu(got, F, n, prec, (1,)), f"rfft n={n} s={s}")
                _record(w, "real" + blue, prec, A.nu(back, b, n, prec, (1,)), f"irfft n={n} s={s}")
                if sf is not None:   # numpy has no DCT / DST: the r2r yardstick needs scipy
                    for kind, ref in zip(A.R2R_KINDS, case[1:]):
                        f = sf.dct if kind.startswith("dct") else sf.dst
                        _record(w, "r2r" + blue, prec, A.nu(f(case[0].astype(A.RDT[prec]), int(kind[-1]), axis=1), ref, n, prec, (1,)),
                                f"{kind} n={n} s={s}")
    for n1, n2 in A.REAL_2D:
        x, F = A.real_planes(n1, n2, 3, 4000 + n1)
        X, b = A.half_planes(n1, n2, 3, 5000 + n1)
        m = sf if sf is not None else np.fft
        for prec in precs:
            _record(w, "real", prec, A.nu(m.rfft2(x.astype(A.RDT[prec])), F, n1 * n2, prec, (1, 2)), f"rfft2 {n1}x{n2}")
            _record(w, "real", prec, A.nu(m.irfft2(X.astype(A.CDT[prec]), s=(n1, n2), norm="forward"), b, n1 * n2, prec, (1, 2)),
                    f"irfft2 {n1}x{n2}")
    for n1, n2, batch in A.ONE_LAUNCH_2D + A.PLAIN_2D:
        fam = "2d-one-launch" if (n1, n2, batch) in A.ONE_LAUNCH_2D else "2d"
        x, F = A.complex_planes(n1, n2, batch, 7000 + n1)
        for prec in precs:
            _record(w, fam, prec, A.nu(_fftn(x, (1, 2), +1, prec), F, n1 * n2, prec, (1, 2)), f"fft2 {n1}x{n2} fwd")
            _record(w, fam, prec, A.nu(_fftn(x, (1, 2), -1, prec), A.reverse_bins(F, (1, 2)), n1 * n2, prec, (1, 2)), f"fft2 {n1}x{n2} bwd")
    for N, P in A.PLANS_3D:
        x, F = A.complex_volume(N, 8000 + N[0])
        B = A.reverse_bins(F, (0, 1, 2))
        for prec in precs:
            got = _fftn(x, None, +1, prec)
            _record(w, "3d", prec, A.nu_parts(zip(A.split_bins(got, P), A.split_bins(F, P)), x.size, prec), f"fftn {N} P={P} fwd")
            got = _fftn(x, None, -1, prec)
            _record(w, "3d", prec, A.nu_parts(zip(A.split_x(got, P), A.split_x(B, P)), x.size, prec), f"fftn {N} P={P} bwd")
    m = sf if sf is not None else np.fft
    for N, P in A.PLANS_R2C:
        x, F = A.real_volume(N, 9000 + N[0])
        for prec in precs:
            got = m.rfftn(x.astype(A.RDT[prec]))
            _record(w, "r2c-3d", prec, A.nu_parts(zip(A.split_bins(got, P), A.split_bins(F, P)), x.size, prec), f"rfftn {N} P={P}")
    for N, P in A.PLANS_CONV:
        for real in (False, True):
            x, H, ref = A.conv_case(N, real, 9500 + N[0])
            for prec in precs:
                if real:
                    got = m.irfftn(m.rfftn(x.astype(A.RDT[prec])) * H.astype(A.RDT[prec]), s=N)
                else:
                    got = m.ifftn(m.fftn(x.astype(A.CDT[prec])) * H.astype(A.RDT[prec]))
                assert got.dtype == (A.RDT[prec] if real else A.CDT[prec]) or sf is None
                _record(w, "conv", prec, A.nu_parts(zip(A.split_x(got, P), A.split_x(ref, P)), x.size ** 2, prec), f"conv real={real} {N}")
    return w


@pytest.mark.parametrize("prec", A.PRECS)
def test_yardstick_is_under_its_constants(prec):
    """Recomputes the CPU FFT's nu per family and holds it under YARDSTICK, the constants CEILING derives from."""
    if prec == "f32" and sf is None:
        pytest.skip("the fp32 yardstick needs scipy.fft: numpy computes complex64 transforms in double")
    w = _yardsticks()
    missing = []
    for fam in A.YARDSTICK:
        if (fam, prec) not in w:
            missing.append(fam)
            continue
        value, what = w[(fam, prec)]
        print(f"yardstick {fam} {prec}: {value:.3f}  ({what})")
        assert value <= A.YARDSTICK[fam][prec], (fam, prec, value, what)
    assert not missing or (sf is None and all(f.startswith("r2r") for f in missing)), missing


def test_no_bound_exceeds_its_ceiling():
    assert set(A.BOUND) == set(A.YARDSTICK) == set(A.CEILING)
    for fam in A.BOUND:
        for prec in A.PRECS:
            assert 0 < A.BOUND[fam][prec] <= A.CEILING[fam][prec], (fam, prec)
            if fam in A.FIXED_CEILING:
                want = 40.0 if fam.endswith("-impulse") else 9.0 if fam == "bluestein" else 3.2
                assert A.CEILING[fam][prec] == want, (fam, prec)
            else:
                assert A.CEILING[fam][prec] <= 8 * A.YARDSTICK[fam][prec] + 1e-12, (fam, prec)


# ---- the bounds bite -----------------------------------------------------------------------------------------------------------------
def _mutant(x, slip):
    """An exact longdouble FFT of the rows of x (n even) whose last radix-2 stage is spoiled: slip "all": w^(k+1) for w^k in every
    butterfly; "one": in one butterfly of row 0, as from one lane or one ragged tile; "rel": every twiddle off by 3e-13 of itself, as from
    a recurrence or a product of stored powers taken once too often; None: unspoiled."""
    n = x.shape[-1]
    h = n // 2
    E, O = A.ld_fft(x[..., 0::2]), A.ld_fft(x[..., 1::2])
    k = np.arange(h, dtype=np.int64)
    w = np.broadcast_to(A.ld_phase(k, n, +1), O.shape).copy()
    if slip == "all":
        w[...] = A.ld_phase(k + 1, n, +1)
    elif slip == "one":
        w[0, h // 3] = A.ld_phase(np.int64(h // 3 + 1), n, +1)
    elif slip == "rel":
        w *= 1 + LD(3e-13)
    else:
        assert slip is None
    return np.concatenate([E + w * O, E - w * O], axis=-1)


def _verdicts(n, slip, prec):
    """Every measure tests/test_gpu_accuracy.py applies to a length of n's family, on its inputs -> [(measure, family, value)]"""
    four = n > 4096
    fam = "four-step" if four else "tuned"
    shape = (2, n) if four else (9, n)
    out = []
    x, F = A.complex_lines(n, shape, 1, 1000 + n, 2 if four else 0)
    out.append(("random", fam, A.nu(_mutant(x, slip).astype(A.CDT[prec]), F, n, prec, (1,))))
    d, Fd = A.impulse_lines(n, shape, 1, (n - 1,) if four else tuple(A.impulse_positions(n)))
    out.append(("impulse", fam + "-impulse", A.nu_impulse(_mutant(d, slip).astype(A.CDT[prec]), Fd, prec)))
    if not four:
        t, Ft = A.tone_lines(n, shape, 1, prec)
        out.append(("tone", fam, A.nu(_mutant(t, slip).astype(A.CDT[prec]), Ft, n, prec, (1,))))
    return out


def _old_measure(n, slip, prec):
    """The existing tests' input (uniform, 9 rows up to 4096 points and 5 above), reference (float64 numpy) and measure."""
    rng = np.random.default_rng(n)
    x = rng.uniform(-1, 1, (9 if n <= 4096 else 5, n)) + 1j * rng.uniform(-1, 1, (9 if n <= 4096 else 5, n))
    x = x.astype(A.CDT[prec]).astype(np.complex128)
    return A.old_measure(_mutant(x, slip).astype(A.CDT[prec]).astype(np.complex128), np.fft.fft(x))


OLD_TOL = {"f64": 1e-11, "f32": 5e-4}
# (slip, precision in which it applies, the lengths at which it passes the old pass mark, the measures that must each reject it at every
# length).  A slip in every butterfly, or in every twiddle, shows on every input.  The slip in ONE butterfly moves two bins of one line:
# the impulses catch it at every length (both bins are off by |w - 1| of a bin of modulus 1: 800 ... 12900 eps), the random line only up
# to 8192 points (nu 79 and 19; 0.8 at 65536, where two bins of 65536 vanish in the line's norm), and the tone, whose spectrum is one
# bin, never.
MUTANTS = [("all", "f32", (8192, 65536), ("random", "impulse", "tone")),
           ("one", "f32", (4096, 8192, 65536), ("impulse",)),
           ("rel", "f64", (4096, 8192, 65536), ("random", "impulse", "tone"))]


@pytest.mark.parametrize("slip,prec,passes_old,catchers", MUTANTS)
@pytest.mark.parametrize("n", [4096, 8192, 65536])
def test_bounds_reject_the_mutants(n, slip, prec, passes_old, catchers):
    old = _old_measure(n, slip, prec)
    print(f"mutant {slip} n={n} {prec}: old measure {old:.3e}")
    if n in passes_old:
        assert old < OLD_TOL[prec], "the gap this test documents: the old pass mark lets the mutant through"
    verdicts = _verdicts(n, slip, prec)
    for measure, fam, value in verdicts:
        print(f"mutant {slip} n={n} {prec}: {measure} {fam} {value:.1f} (bound {A.BOUND[fam][prec]}, ceiling {A.CEILING[fam][prec]})")
        assert A.BOUND[fam][prec] <= A.CEILING[fam][prec]
        if measure in catchers:    # above the ceiling, so above every bound a later measurement may set
            assert value > A.CEILING[fam][prec], (n, slip, prec, measure, value)
    assert {"random", "impulse"} <= {m for m, _, _ in verdicts}    # (the tone is an input of the tuned lengths only)
    if slip == "one" and n <= 8192:
        assert verdicts[0][2] > A.CEILING[verdicts[0][1]][prec], "the random line sees one butterfly up to 8192 points"
    # the unspoiled twin passes every one of them: the mutant's model of a transform is sound
    for _, fam, value in _verdicts(n, None, prec):
        assert value <= A.YARDSTICK[fam][prec], (fam, value)
