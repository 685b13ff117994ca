"""The long 1-D real FFT convolution (dfft_rconv1d_long) as shared by tests/test_rconv1d_long_host.py and tests/test_gpu_rconv1d_long.py:
the numpy restatement of the three passes, the filter permutation, the cases, inputs, filters and references.  No GPU, no scipy.

Accuracy in eps units (accuracy_ref.nu per row, n_eff = m, longdouble references), measured on an MI355X over ACC_CASES by
test_gpu_rconv1d_long.py::test_accuracy_in_eps_units (worst row of the sweep):
    MEASURED, below.  BOUND / BOUND_N1 = twice the larger of the composed-route and the same-precision CPU-pipeline worst values,
    rounded up to two digits; rows of one sample (n = 1) have their own bound: their output is one number, the mean of a spectrum whose
    errors all add up in it, so nu -- which divides by the row's own norm -- is larger there."""
from functools import lru_cache

import numpy as np

import accuracy_ref as A

LD, CLD = A.LD, A.CLD

# the factor lengths of the library: every 2^a, 3 * 2^a, 5 * 2^a in [64, 2048], 81 and 125
FACTORS = sorted({b << a for b in (1, 3, 5) for a in range(12) if 64 <= b << a <= 2048} | {81, 125})
# m -> (N1, N2): N1 even with power-of-two factors; N1 odd with radix 3; N2 not a power of two; M odd
SPLITS = {16384: (64, 128), 20736: (81, 128), 18432: (96, 96), 31250: (125, 125)}
LENGTHS = sorted(SPLITS)
KINDS = ("real", "complex")
ROWS = ((2, 3), (1, 1), (5, 2))          # (batch, channels): odd and even row counts, one row, row % channels
BOUND_REL = {"f64": 1e-11, "f32": 5e-4}  # max |got - ref| / max |ref| against numpy float64

# worst nu per (route, precision) over ACC_CASES, rows of more than one sample / rows of one sample
MEASURED = {
    "fused": {"f64": (0.511, 3.120), "f32": (0.552, 1.502)},     # m=16384 n=8193 complex, m=18432 n=1 complex / m=16384 n=m real, m=18432 n=1 complex
    "composed": {"f64": (0.502, 4.236), "f32": (0.546, 0.729)},  # m=16384 n=8193 complex, m=18432 n=1 complex / m=31250 n=m complex, m=18432 n=1 complex
    "cpu": {"f64": (0.569, 0.923), "f32": (0.534, 1.427)},       # m=31250 n=m real, m=18432 n=1 complex / m=31250 n=m complex, m=16384 n=1 complex
}
BOUND = {"f64": 1.2, "f32": 1.1}      # 2 x 0.569 (CPU), 2 x 0.546 (composed)
BOUND_N1 = {"f64": 8.5, "f32": 2.9}   # 2 x 4.236 (composed), 2 x 1.427 (CPU)


def split(m):
    """The library's split of m/2: the most balanced pair of factor lengths, the larger as N2; None if m is not accepted"""
    if m % 2 or m <= 8192 or m > 1 << 23:
        return None
    M, best = m // 2, None
    for a in FACTORS:
        if a * a <= M and M % a == 0 and M // a in FACTORS:
            best = (a, M // a)
    return best


def n_values(m):
    """n = m (circular), m/2, m/2 + 1 (odd: per-real accesses), 2 N2 + 6 (a partly filled second tile row), 5, 1"""
    return [m, m // 2, m // 2 + 1, 2 * SPLITS[m][1] + 6, 5, 1]


def permute_filter(H, n1, n2):
    """hp[c][k1 N2 + k2] = H[c][k1 + N1 k2], hp[c][M] = H[c][M]"""
    M = n1 * n2
    k1, k2 = np.meshgrid(np.arange(n1), np.arange(n2), indexing="ij")
    hp = np.empty_like(H)
    hp[:, :M] = H[:, (k1 + n1 * k2).reshape(-1)]
    hp[:, M] = H[:, M]
    return hp


def pipeline_model(x, hp, n1, n2):
    """One row as the three kernels compute it, thread for thread.  hp [M + 1] is the permuted filter of the row's channel."""
    M, m, n = n1 * n2, 2 * n1 * n2, x.shape[-1]
    WM = lambda p: np.exp(-2j * np.pi * (p % M) / M)  # noqa: E731
    # pass A: z[j1][j2] read from the reals (zeros beyond n), N1-point transforms down the columns, times W_M^{k1 j2}
    z = np.zeros((n1, n2), dtype=complex)
    for j1 in range(n1):
        if 2 * j1 * n2 >= n:
            break                               # tile rows wholly beyond n: zeros in registers
        for j2 in range(n2):
            j = j1 * n2 + j2
            z[j1, j2] = (x[2 * j] if 2 * j < n else 0.0) + 1j * (x[2 * j + 1] if 2 * j + 1 < n else 0.0)
    S = np.fft.fft(z, axis=0)
    scr = S * WM(np.outer(np.arange(n1), np.arange(n2)))
    # Mid: items of two scratch rows (k1, N1 - k1); rows 0 and N1/2 pair with themselves
    rowc = np.exp(-2j * np.pi * np.arange(n1) / m)           # the per-row constant
    colt = np.exp(-2j * np.pi * np.arange(n2) / (2 * n2))    # the per-thread table
    sc = 0.5 / m
    out = np.empty_like(scr)
    items = [(0, n1 // 2 if n1 % 2 == 0 else None)] + [(i, n1 - i) for i in range(1, (n1 + 1) // 2)]
    done = set()
    for ra, rb in items:
        tiles = {ra: np.fft.fft(scr[ra])}                    # 2a: row k1 holds Z[k1 + N1 k2] at position k2
        if rb is not None:
            tiles[rb] = np.fft.fft(scr[rb])
        for ka in tiles:
            kb = 0 if ka == 0 else n1 - ka                   # the partner's row (itself for 0 and N1/2)
            zp = np.empty(n2, dtype=complex)
            for k2 in range(n2):                             # one iteration = one (thread, point)
                pk = (0 if k2 == 0 else n2 - k2) if ka == 0 else n2 - 1 - k2
                k0 = ka == 0 and k2 == 0
                zk, zm = tiles[ka][k2], tiles[kb][pk]        # 2b: Z[k] and Z[M - k]
                w = rowc[ka] * colt[k2]                      # e^{-2 pi i (ka + N1 k2) / m}
                xe = zk + np.conj(zm)
                xo = -1j * (zk - np.conj(zm))
                t = xo * w
                ya = (xe + t) * (hp[ka * n2 + k2] * sc)      # 2c
                yb = np.conj(xe - t) * (hp[M if k0 else kb * n2 + pk] * sc)
                if k0:
                    ya, yb = ya.real + 0j, yb.real + 0j
                zp[k2] = np.conj((ya + np.conj(yb)) + 1j * (ya - np.conj(yb)) * np.conj(w))
            assert ka not in done
            done.add(ka)
            out[ka] = np.conj(np.fft.fft(zp))                # 2d: conj . forward . conj
    assert done == set(range(n1))
    # pass C: times W_M^{-k1 j2}, N1-point inverse down the columns, Re / Im as the reals 2j, 2j + 1 < n
    zz = np.fft.ifft(out * np.conj(WM(np.outer(np.arange(n1), np.arange(n2)))), axis=0) * n1
    y = np.zeros(m)
    y[0::2], y[1::2] = zz.real.reshape(-1), zz.imag.reshape(-1)
    return y[:n]


def make_filter(channels, m, kind, seed):
    """modulus in [0.5, 2] (float32 values): real ones uniform, complex ones those moduli with random phases (rconv1d_cases.make_filter)"""
    rng = np.random.default_rng(seed)
    mod = rng.uniform(0.5, 2.0, (channels, m // 2 + 1)).astype(np.float32).astype(np.float64)
    if kind == "real":
        return mod
    ph = rng.uniform(0.0, 2 * np.pi, mod.shape)
    return (mod * np.exp(1j * ph)).astype(np.complex64).astype(np.complex128)


def reference64(x, H, m):
    """numpy float64: irfft(rfft(x, m) * H, m)[:n] of rows [rows][n], row r with H[r % channels]"""
    rows, n = x.shape
    return np.fft.irfft(np.fft.rfft(x, m, axis=1) * H[np.arange(rows) % H.shape[0]], m, axis=1)[:, :n]


@lru_cache(maxsize=64)
def case(m, n, channels, batch, kind):
    """-> (x [batch * channels][n] float64 of float32 values, H [channels][m/2 + 1], numpy float64 reference), frozen"""
    seed = 21000 + m + 4 * n + channels + (100 if kind == "complex" else 0)
    x = A.rand_real((batch * channels, n), seed)
    H = make_filter(channels, m, kind, seed + 1)
    ref = reference64(x, H, m)
    for a in (x, H, ref):
        a.setflags(write=False)
    return x, H, ref


# the accuracy sweep: every split, both filter kinds, three rows of three channels
ACC_ROWS = (1, 3)


def acc_cases():
    for m in LENGTHS:
        for kind in KINDS:
            for n in (m, m // 2 + 1, 1):
                yield m, n, kind


@lru_cache(maxsize=32)
def acc_case(m, n, kind):
    """-> (x, H, longdouble reference) of one case of the accuracy sweep"""
    batch, channels = ACC_ROWS
    x, H, _ = case(m, n, channels, batch, kind)
    xp = np.zeros((x.shape[0], m), dtype=LD)
    xp[:, :n] = x
    Y = A.ld_rfft(xp, 1) * np.asarray(H).astype(CLD)[np.arange(x.shape[0]) % channels]
    ref = (A.ld_irfft(Y, m, 1) / LD(m))[:, :n]
    ref.setflags(write=False)
    return x, H, ref


def nu_rows(got, ref, m, prec):
    """accuracy_ref.nu per row, n_eff = m"""
    return A.nu(got, ref, m, prec, (1,))
