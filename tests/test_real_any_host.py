"""Any-length real transforms, host side (no GPU): the dfft_real_form rule, a numpy model of the two-for-one pack / split and merge /
unpack formulas of csrc/dfft_real_pair.hip, and the argument checks of dfft_rfft1d / dfft_plan_create_r2c_any that run before the
device is queried."""
import ctypes as C

import numpy as np
import pytest


def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


FORMS = {1: 3, 2: 2, 3: 2, 4: 1, 15: 2, 16: 1, 22: 3, 30: 1, 97: 3, 125: 2, 2187: 2, 4096: 1, 8192: 1, 8194: 3, 15625: 3, 16384: 3,
         2 ** 23 + 1: 0}


def test_real_form_rule():
    from distributedfft_amd import api
    for n, f in FORMS.items():
        assert api.real_form(n) == f, (n, api.real_form(n), f)
    for n in (0, -4):
        assert api.real_form(n) == 0
    # form 1 is exactly where the half-length plans of dfft_plan_create_r2c apply: n even and n/2 a single-pass length
    for n in range(2, 400):
        half = n % 2 == 0 and api.length_kind(n // 2) == 1
        assert (api.real_form(n) == 1) == half, n
        if not half:
            assert api.real_form(n) == (2 if api.length_kind(n) == 1 else 3), n


# ---- numpy model of the two-for-one formulas -------------------------------------------------------------------------------------
def _pair_rfft(x):
    """rows [r][n] -> bins [r][n//2 + 1] through one complex transform per pair of rows (an odd last row paired with zeros)."""
    r, n = x.shape
    xa = np.vstack([x, np.zeros((r % 2, n))])
    Z = np.fft.fft(xa[0::2] + 1j * xa[1::2], axis=1)
    m = np.arange(n // 2 + 1)
    Zk, Zm = Z[:, m], Z[:, (n - m) % n]
    A = (Zk + np.conj(Zm)) / 2
    B = (Zk - np.conj(Zm)) / 2j
    out = np.empty((xa.shape[0], n // 2 + 1), complex)
    out[0::2], out[1::2] = A, B
    return out[:r]


def _pair_irfft(X, n):
    """bins [r][n//2 + 1] -> n * irfft per row through one inverse complex transform per pair of rows."""
    r = X.shape[0]
    Xa = np.vstack([X, np.zeros((r % 2, X.shape[1]), complex)])
    A, B = Xa[0::2].copy(), Xa[1::2].copy()
    for M in (A, B):  # numpy's rule: the imaginary parts of the DC and Nyquist bins do not count
        M[:, 0] = M[:, 0].real
        if n % 2 == 0:
            M[:, n // 2] = M[:, n // 2].real
    k = np.arange(n)
    lo = 2 * k <= n
    m = np.where(lo, k, n - k)
    Af, Bf = A[:, m], B[:, m]
    Z = np.where(lo, Af + 1j * Bf, np.conj(Af) + 1j * np.conj(Bf))
    z = np.fft.ifft(Z, axis=1) * n
    out = np.empty((Xa.shape[0], n))
    out[0::2], out[1::2] = z.real, z.imag
    return out[:r]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 9, 15, 16, 22, 97, 125, 128, 243])
@pytest.mark.parametrize("rows", [1, 2, 5, 8])
def test_pair_model_matches_numpy(n, rows):
    rng = np.random.default_rng(n * 100 + rows)
    x = rng.standard_normal((rows, n))
    ref = np.fft.rfft(x, axis=1)
    assert np.abs(_pair_rfft(x) - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    # non-Hermitian input: imaginary DC / Nyquist parts present; the result is n * irfft all the same
    X = rng.standard_normal((rows, n // 2 + 1)) + 1j * rng.standard_normal((rows, n // 2 + 1))
    ref = n * np.fft.irfft(X, n, axis=1)
    assert np.abs(_pair_irfft(X, n) - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    # and the round trip
    assert np.abs(_pair_irfft(_pair_rfft(x), n) / n - x).max() <= 1e-12


# ---- argument checks, before the device query ------------------------------------------------------------------------------------
def _rfft1d(inp, out, n, batch, dtype=0, direction=1):
    lib = _lib()
    rc = lib.dfft_rfft1d(C.c_void_p(inp) if inp else None, C.c_void_p(out) if out else None, n, batch, dtype, direction, None)
    return rc, lib.dfft_last_error().decode()


def test_rfft1d_argument_errors():
    from distributedfft_amd import _lib as L
    A, B = 0x10000000, 0x20000000
    for d in (1, -1):
        assert _rfft1d(0, B, 15, 4, direction=d)[0] == L.EINVAL
        assert _rfft1d(A, 0, 15, 4, direction=d)[0] == L.EINVAL
        assert _rfft1d(A, B, 15, -1, direction=d)[0] == L.EINVAL
        assert _rfft1d(A, B, 15, 4, dtype=7, direction=d)[0] == L.EINVAL
        assert _rfft1d(A, A, 15, 4, direction=d)[0] == L.EINVAL            # out == in
        assert _rfft1d(A, A + 64, 15, 4, direction=d)[0] == L.EINVAL       # overlapping ranges
        rc, msg = _rfft1d(A, B, 2 ** 23 + 1, 4, direction=d)
        assert rc == L.EUNSUPPORTED and str(2 ** 23 + 1) in msg
        assert _rfft1d(A, B, 0, 4, direction=d)[0] == L.EUNSUPPORTED
    assert _rfft1d(A, B, 15, 4, direction=0)[0] == L.EINVAL
    if _lib().dfft_device_count() > 0:
        return
    for n in (3, 15, 16, 97, 125, 8192, 15625, 16384):
        for d in (1, -1):
            assert _rfft1d(A, B, n, 4, direction=d)[0] == L.ENOGPU, n
    # ranges that merely touch do not overlap: 4 rows of 16 reals (fp64) = 512 bytes
    assert _rfft1d(A, A + 512, 16, 4)[0] == L.ENOGPU


def _create_any(n0, n1, n2, flags=0, in_ptr=0x1000, out_ptr=0x2000, dtype=0, direction=1, P=1, g=0):
    lib = _lib()
    h = C.c_void_p()
    rc = lib.dfft_plan_create_r2c_any(C.byref(h), n0, n1, n2, dtype, direction, C.c_void_p(in_ptr), C.c_void_p(out_ptr) if out_ptr else None,
                                      None, g, P, flags)
    return rc, lib.dfft_last_error().decode()


@pytest.mark.parametrize("direction", [1, -1])
def test_r2c_any_plan_argument_errors(direction):
    from distributedfft_amd import _lib as L
    d = dict(direction=direction)
    rc, msg = _create_any(8192, 16, 15, **d)
    assert rc == L.EUNSUPPORTED and "8192" in msg                       # long N0
    rc, msg = _create_any(16, 8192, 15, **d)
    assert rc == L.EUNSUPPORTED and "8192" in msg                       # long N1
    rc, msg = _create_any(16, 16, 2 ** 23 + 1, **d)
    assert rc == L.EUNSUPPORTED and "N2 = " in msg                      # no real form
    assert _create_any(16, 16, 15, out_ptr=0, **d)[0] == L.EINVAL       # out == NULL
    assert _create_any(16, 16, 15, out_ptr=0x1000, **d)[0] == L.EINVAL  # out == in
    for f in (L.PLAN_OVERLAP, L.PLAN_NATURAL, L.PLAN_UNFUSED, L.PLAN_ANY_LENGTH, L.PLAN_OVERLAP | L.PLAN_INPUT_FROM_IN):
        assert _create_any(16, 16, 15, flags=f, **d)[0] == L.EUNSUPPORTED, f
    assert _create_any(16, 16, 15, dtype=7, **d)[0] == L.EINVAL
    assert _create_any(16, 16, 15, P=2, g=0, **d)[0] == L.EINVAL        # P > 1 without a communicator


def test_r2c_any_plan_accepts_every_form_up_to_the_device_query():
    """Shapes of every real form pass the argument checks; without a GPU the first error is the device query's.  The old entry point
    keeps refusing the real axes that are not of form 1."""
    from distributedfft_amd import _lib as L
    from distributedfft_amd import api
    shapes = ((16, 16, 15), (8, 8, 97), (16, 16, 16384), (12, 10, 125), (6, 4, 22), (5, 7, 2187), (4, 4, 16), (8, 8, 15625))
    for N in shapes:
        assert api.r2c_counts(*N, 1, 0)[0] == N[0] * N[1] * N[2]
        if api.real_form(N[2]) != 1:
            lib = _lib()
            h = C.c_void_p()
            assert lib.dfft_plan_create_r2c(C.byref(h), *N, 0, 1, C.c_void_p(0x1000), C.c_void_p(0x2000), None, 0, 1, 0) == L.EUNSUPPORTED, N
    if _lib().dfft_device_count() > 0:
        return
    for N in shapes:
        for flags in (L.PLAN_DEFAULT, L.PLAN_INPUT_FROM_IN):
            for d in (1, -1):
                assert _create_any(*N, flags=flags, direction=d)[0] == L.ENOGPU, N
