"""Host tests (no GPU) of the any-length transforms: the length classes of dfft_length_kind, the padded lengths of
dfft_bluestein_length, the unchanged answers of dfft_length_supported, and a numpy model of the chirp / B^ construction of
csrc/dfft_bluestein.hip, step for step, against numpy.fft."""
import numpy as np
import pytest

from distributedfft_amd import _lib

# (n, kind): 1 single-pass, 2 four-step, 3 Bluestein, 0 none
KINDS = [
    (1, 3), (11, 3), (13, 3), (22, 3), (4100, 3), (8191, 3), (2 * 4099, 3), (2 ** 23 - 1, 3), (4099, 3), (1009, 3), (2039, 3),
    (2049, 3), (65537, 3), (1000003, 3), (97, 3), (101, 3), (211, 3),
    (12, 1), (4096, 1), (2, 1), (1000, 1), (2401, 1), (3600, 1),
    (8192, 2), (2 ** 22, 2), (6561, 2), (2 ** 24, 2),
    (0, 0), (-4, 0), (2 ** 23 + 1, 0), (2 ** 25, 0),
]
# what dfft_length_supported answered before any-length transforms existed
SUPPORTED_BEFORE = {1: 0, 11: 0, 13: 0, 22: 0, 4100: 0, 8191: 0, 2 * 4099: 0, 2 ** 23 - 1: 0, 12: 1, 4096: 1, 8192: 1, 2 ** 22: 1,
                    0: 0, -4: 0, 2 ** 23 + 1: 0, 2 ** 25: 0}
TUNED = [2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 16, 24, 25, 32, 40, 48, 49, 64, 80, 96, 100, 125, 128, 160, 192, 200, 256, 320, 343, 384, 400,
         512, 640, 768, 1000, 1024, 1280, 1536, 2048, 27, 81, 243, 625, 729, 2187, 3125, 2401, 4096]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("n,kind", KINDS)
def test_length_kind(lib, n, kind):
    assert lib.dfft_length_kind(n) == kind


@pytest.mark.parametrize("n", sorted(SUPPORTED_BEFORE))
def test_length_supported_unchanged(lib, n):
    assert lib.dfft_length_supported(n) == SUPPORTED_BEFORE[n]


@pytest.mark.parametrize("n,kind", KINDS)
def test_bluestein_length_is_valid_for_its_path(lib, n, kind):
    m = lib.dfft_bluestein_length(n)
    if kind != 3:
        assert m == 0
        return
    if n == 1:
        assert m == 1
        return
    assert m >= 2 * n - 1
    if n <= 2048:  # fused form: the smallest tuned single-pass length
        assert m in TUNED and m <= 4096
        assert not any(2 * n - 1 <= t < m for t in TUNED)
    else:          # multi-pass form: a four-step length (and the smallest one)
        assert 4096 < m <= 2 ** 24 and lib.dfft_length_kind(m) == 2
    assert m <= 2 ** 24


def test_bluestein_length_is_the_smallest_four_step_length(lib):
    for n in (2049, 4099, 5003):
        m = lib.dfft_bluestein_length(n)
        assert all(lib.dfft_length_kind(k) != 2 for k in range(2 * n - 1, m))


def test_python_wrappers_and_flag(lib):
    from distributedfft_amd import api
    assert api.PLAN_ANY_LENGTH == 16
    assert api.length_kind(11) == 3 and api.bluestein_length(11) == 24
    assert api.length_kind(4096) == 1 and api.bluestein_length(4096) == 0


def _chirp(n, d):
    m = np.arange(n, dtype=np.int64)
    q = (m * m) % (2 * n)                       # 64-bit integers, as the library does
    return np.exp(-d * 1j * np.pi * q / n)


def bluestein_model(x, d, M):
    """csrc/dfft_bluestein.hip step for step: chirp, B^ = FFT_M(b) / M, pad, FFT, multiply, inverse as conj . FFT . conj, chirp."""
    n = x.shape[-1]
    c = _chirp(n, d)
    b = np.zeros(M, dtype=np.complex128)
    b[:n] = np.conj(c) / M
    b[M - np.arange(1, n)] = np.conj(c[1:]) / M
    bhat = np.fft.fft(b)
    a = np.zeros(x.shape[:-1] + (M,), dtype=np.complex128)
    a[..., :n] = x * c
    A = np.fft.fft(a, axis=-1)
    y = np.fft.fft(np.conj(A * bhat), axis=-1)  # the fused kernel's conj . forward . conj inverse (1/M folded into B^)
    return c * np.conj(y[..., :n])


@pytest.mark.parametrize("n", [1, 11, 13, 97, 1009, 2039, 4099])
@pytest.mark.parametrize("d", [1, -1])
def test_numpy_model_of_the_construction(lib, n, d):
    rng = np.random.default_rng(n)
    x = rng.uniform(-1, 1, (3, n)) + 1j * rng.uniform(-1, 1, (3, n))
    M = int(lib.dfft_bluestein_length(n))
    got = bluestein_model(x, d, M)
    ref = np.fft.fft(x, axis=-1) if d > 0 else np.fft.ifft(x, axis=-1) * n
    assert np.abs(got - ref).max() / np.abs(ref).max() < 1e-13
