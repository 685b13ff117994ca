"""The long batched 1-D real cross-spectrum (dfft_rxspec1d_long) as shared by tests/test_rxspec1d_long_host.py (which measures the CPU
yardstick on the cases) and tests/test_gpu_rxspec1d_long.py / tests/test_gpu_rconv1d_long_autograd.py (which run the library on them):
the numpy restatement of the kernels, the restated chunk / slice rule, the cases, inputs and longdouble references.  No GPU, no scipy.

Inputs come from accuracy_ref.rand_real (float32 values, so both precisions share one input and one reference).  The reference is
sum_b conj(X[b, c]) G[b, c] of accuracy_ref.ld_rfft on the zero-padded rows, in longdouble (rxspec1d_cases.reference).

Accuracy in eps units (accuracy_ref.nu per channel line over the m/2 + 1 bins, n_eff = m), worst line per class of case:
    "sweep"   all_cases() with n > 1
    "n1"      all_cases() with n = 1: every bin of a channel is the one number sum_b x[b] g[b], a sum of at most 17 signed products
              that cancels, so nu -- which divides by the line's own norm -- is larger there (as in rconv1d_long_cases.BOUND_N1)
    "chunks"  CHUNK_CASES (fp64): batches of about a thousand rows per channel; a bin is a sum of signed products that cancels to
              about 1 / sqrt(batch) of the sum of their moduli (the long batch set the bound of the short form too)
MEASURED, below.  BOUND = twice the larger of the composed route's (on an MI355X) and the same-precision CPU pipeline's worst value
(tests/test_rxspec1d_long_host.py measures the latter again on every run), rounded up to two digits, per class."""
from functools import lru_cache

import numpy as np

import accuracy_ref as A
import rconv1d_long_cases as LC
import rxspec1d_cases as XC

LD, CLD = A.LD, A.CLD
FACTORS = LC.FACTORS
# m -> (N1, N2): every radix family, odd N1, N1 == N2, M odd
SPLITS = {10240: (64, 80), 16384: (64, 128), 20736: (81, 128), 18432: (96, 96), 31250: (125, 125)}
LENGTHS = list(SPLITS)
ESIZE = {"f64": 16, "f32": 8}

# ---- the rule of include/dfft.h (dfft_rxspec1d_long): fixed constants, never the device ------------------------------------------------
SCRATCH_CAP = 256 << 20                 # pass-A results of a chunk: at most max(this, one row pair's)
TARGET_ITEMS = 2048                     # (slice, channel, row pair) items worth cutting the batch for
MIN_STEPS = 8                           # rows of a channel in a slice, at least
# (N2, precision) that lxspec_fused_ok of dfft_lxspec.hip sends to the composed route: their accumulating kernels would spill
ROUTED = {(384, "f64"), (640, "f64"), (1280, "f64"), (1536, "f64")}

# worst nu per (route, precision, class).  The cases: sweep -- fused m=31250 n=m batch=17 / m=16384 n=8193 batch=17; composed m=207360
# n=103682 / 103681 (two rows: they share one transform there); CPU m=10368 n=5185 / m=31250 n=m batch=17.  n1 -- m=18432 n=1 batch=17
# throughout (the fused fp64 worst is m=20736).  chunks -- m=10240 n=7 channels=4 batch=820 throughout.
MEASURED = {
    "fused": {"f64": {"sweep": 0.511, "n1": 0.284, "chunks": 0.620}, "f32": {"sweep": 0.561, "n1": 74.977}},
    "composed": {"f64": {"sweep": 1.155, "n1": 73.561, "chunks": 1.801}, "f32": {"sweep": 0.879, "n1": 148.542}},
    "cpu": {"f64": {"sweep": 0.587, "n1": 73.561, "chunks": 1.780}, "f32": {"sweep": 0.558, "n1": 148.542}},
}
# 2 x 1.155, 2 x 73.561, 2 x 1.801 (composed) / 2 x 0.879, 2 x 148.542 (composed; the CPU pipeline's n1 figures are the same numbers)
BOUND = {"f64": {"sweep": 2.4, "n1": 150.0, "chunks": 3.7}, "f32": {"sweep": 1.8, "n1": 300.0}}
# (m, n, channels, batch), fp64: two whole chunks of 1638 rows and a ragged third of 24 / of 4; the chunk edges fall between batch
# entries (1638 = 3 * 546) / inside one (1638 = 4 * 409 + 2).  The scratch, not the input, sets the chunk: the fields stay tiny.
CHUNK_CASES = ((10240, 7, 3, 1100), (10240, 7, 4, 820))


def klass(n, batch):
    return "chunks" if batch > 100 else ("n1" if n == 1 else "sweep")


def chunk_rows(m, prec, rows, cap=SCRATCH_CAP):
    """Rows per chunk: the batch * channels rows are cut in order; a row costs m/2 complex for either field (two counted always)"""
    rb = 2 * (m // 2) * ESIZE[prec]
    return max(1, min(rows, max(cap, rb) // rb))


def slices_rule(m, channels, rows):
    """Slices of a chunk of `rows` rows: a channel has at most steps = ceil(rows / channels) rows there"""
    n1 = LC.split(m)[0]
    steps = -(-rows // channels)
    return max(1, min(TARGET_ITEMS // (channels * ((n1 + 1) // 2)), steps // MIN_STEPS))


def call_slices(m, channels, batch, prec, cap=SCRATCH_CAP):
    """dfft_rxspec1d_long_slices: the slices of the first (the largest) chunk"""
    return slices_rule(m, channels, chunk_rows(m, prec, batch * channels, cap))


def scratch_bytes(m, channels, batch, prec, cap=SCRATCH_CAP):
    """dfft_rxspec1d_long_scratch_bytes: the pass-A results of a chunk and the partial sums of its slices"""
    nr = chunk_rows(m, prec, batch * channels, cap)
    return (nr * 2 * (m // 2) + slices_rule(m, channels, nr) * channels * (m // 2 + 1)) * ESIZE[prec]


def chunks(m, prec, rows, cap=SCRATCH_CAP):
    """[(first row, rows)] of the chunks"""
    nr = chunk_rows(m, prec, rows, cap)
    return [(r0, min(nr, rows - r0)) for r0 in range(0, rows, nr)]


def step_ranges(steps, slices):
    """[(first step, steps)] of the slices: contiguous, the first steps % slices of them one step longer"""
    return XC.slice_ranges(steps, slices)


def fused(m, prec):
    return (LC.split(m)[1], prec) not in ROUTED


@lru_cache(maxsize=None)
def ragged_batch(m, channels=1):
    """The smallest batch that the rule cuts into two or more slices with a ragged last one"""
    b = 2 * MIN_STEPS
    while True:
        s = call_slices(m, channels, b, "f64")
        if s >= 2 and b % s:
            assert call_slices(m, channels, b, "f32") == s
            return b
        b += 1


def rows_of(m):
    """(batch, channels): one row; odd row count with row % channels; several slices with a ragged last one"""
    return ((1, 1), (2, 3), (ragged_batch(m), 1))


def n_values(m):
    """n = m, m/2, m/2 + 1 (odd: per-real accesses), 2 N2 + 6 (a partly filled second tile row), 5, 1"""
    return [m, m // 2, m // 2 + 1, 2 * SPLITS[m][1] + 6, 5, 1]


@lru_cache(maxsize=None)
def mid_length(N):
    """The smallest accepted m whose split has N as the longer factor: its call runs the Mid instantiation of N"""
    return min(2 * a * N for a in FACTORS if a <= N and LC.split(2 * a * N) == (a, N))


# ---- the kernels, thread for thread ------------------------------------------------------------------------------------------------------
def pass_a_model(x, n1, n2):
    """One row: z[j1][j2] read from the reals (zeros beyond n), N1-point transforms down the columns, times W_M^{k1 j2} -> [N1][N2]"""
    M, n = n1 * n2, x.shape[-1]
    z = np.zeros((n1, n2), dtype=complex)
    for j1 in range(n1):
        if 2 * j1 * n2 >= n:
            break
        for j2 in range(n2):
            j = j1 * n2 + j2
            z[j1, j2] = (x[2 * j] if 2 * j < n else 0.0) + 1j * (x[2 * j + 1] if 2 * j + 1 < n else 0.0)
    return np.fft.fft(z, axis=0) * np.exp(-2j * np.pi * (np.outer(np.arange(n1), np.arange(n2)) % M) / M)


def _bins_model(scr, ka_rows, n1, n2):
    """The N2-point stages and the exchange of one item: {ka: (2 X[ka + N1 k2] over k2, 2 X[M] or None)}"""
    m = 2 * n1 * n2
    rowc = np.exp(-2j * np.pi * np.arange(n1) / m)
    colt = np.exp(-2j * np.pi * np.arange(n2) / (2 * n2))
    tiles = {ka: np.fft.fft(scr[ka]) for ka in ka_rows}
    out = {}
    for ka in ka_rows:
        kb = 0 if ka == 0 else n1 - ka
        v, nyq = np.empty(n2, dtype=complex), None
        for k2 in range(n2):
            pk = (0 if k2 == 0 else n2 - k2) if ka == 0 else n2 - 1 - k2
            zk, zm = tiles[ka][k2], tiles[kb][pk]
            xe = zk + np.conj(zm)
            xo = -1j * (zk - np.conj(zm))
            v[k2] = xe + xo * (rowc[ka] * colt[k2])
            if ka == 0 and k2 == 0:
                nyq = xe.real - xo.real
        out[ka] = (v, nyq)
    return out


def kernel_model(x, g, n1, n2, channels, slices, order, row0=0):
    """One chunk as the kernels compute it: x, g [rows][n] (g is x: the auto-spectrum), row r of channel (row0 + r) % channels ->
    out [channels][M + 1] in `order`.  Items (slice, channel, row pair), running sums per (item, bin), times 1/4 at the store, the
    slices summed in order."""
    M, rows = n1 * n2, x.shape[0]
    autos = g is x
    steps = -(-rows // channels)
    items = [(0, n1 // 2 if n1 % 2 == 0 else None)] + [(i, n1 - i) for i in range(1, (n1 + 1) // 2)]
    partial = np.zeros((slices, channels, M + 1), dtype=complex)
    sx = [pass_a_model(r, n1, n2) for r in x]
    sg = sx if autos else [pass_a_model(r, n1, n2) for r in g]
    for s, (q0, count) in enumerate(step_ranges(steps, slices)):
        for c in range(channels):
            rc = (c - row0) % channels
            for ra, rb in items:
                ka_rows = [ra] + ([rb] if rb is not None else [])
                acc = {ka: np.zeros(n2, dtype=complex) for ka in ka_rows}
                accn = 0.0
                for q in range(q0, q0 + count):
                    r = rc + q * channels
                    if r >= rows:
                        continue
                    X = _bins_model(sx[r], ka_rows, n1, n2)
                    G = X if autos else _bins_model(sg[r], ka_rows, n1, n2)
                    for ka in ka_rows:
                        if autos:
                            acc[ka] += np.abs(X[ka][0]) ** 2
                        else:
                            acc[ka] += np.conj(X[ka][0]) * G[ka][0]
                        if ka == 0:
                            accn += X[0][1] * G[0][1]
                for ka in ka_rows:
                    partial[s, c, ka * n2:(ka + 1) * n2] = acc[ka] * 0.25
                    if ka == 0:
                        partial[s, c, 0] = partial[s, c, 0].real
                        partial[s, c, M] = accn * 0.25
    hp = partial[0].copy()
    for s in range(1, slices):
        hp += partial[s]
    return hp if order else unpermute(hp, n1, n2)


def unpermute(hp, n1, n2):
    """The inverse of rconv1d_long_cases.permute_filter: S[c][k1 + N1 k2] = hp[c][k1 N2 + k2], S[c][M] = hp[c][M]"""
    M = n1 * n2
    k1, k2 = np.meshgrid(np.arange(n1), np.arange(n2), indexing="ij")
    S = np.empty_like(hp)
    S[:, (k1 + n1 * k2).reshape(-1)] = hp[:, :M]
    S[:, M] = hp[:, M]
    return S


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
reference = XC.reference


@lru_cache(maxsize=8)
def case(m, n, channels, batch):
    """-> (x, g [batch * channels][n] float64, reference [channels][m/2 + 1] clongdouble, auto-spectrum reference of x), frozen"""
    seed = 41000 + m + 4 * n + channels + 7 * (batch % 1000)
    x = A.rand_real((batch * channels, n), seed)
    g = A.rand_real((batch * channels, n), seed + 1)
    ref, auto = reference(x, g, m, channels), reference(x, x, m, channels)
    for a in (x, g, ref, auto):
        a.setflags(write=False)
    return x, g, ref, auto


@lru_cache(maxsize=4)
def chunk_case(m, n, channels, batch):
    """-> (x, g, reference) of a case of many short rows.  rfft(x, m)[k] = sum_j x[j] W^(jk) with n terms, so
    S[c][k] = sum_(j, l) R_c[j][l] conj(W^(jk)) W^(lk) with the n x n matrices R_c = sum_b x[b, c, j] g[b, c, l], all in longdouble"""
    seed = 43000 + m + channels + batch
    x = A.rand_real((batch * channels, n), seed)
    g = A.rand_real((batch * channels, n), seed + 1)
    k = np.arange(m // 2 + 1, dtype=np.int64)
    E = np.stack([A.ld_phase((j * k) % m, m, +1) for j in range(n)])          # [n][m/2 + 1]: W^(jk)
    xl, gl = x.astype(LD).reshape(batch, channels, n), g.astype(LD).reshape(batch, channels, n)
    ref = np.empty((channels, m // 2 + 1), dtype=CLD)
    for c in range(channels):
        R = xl[:, c, :].T @ gl[:, c, :]
        ref[c] = np.einsum("jl,jk,lk->k", R.astype(CLD), np.conj(E), E)
    for a in (x, g, ref):
        a.setflags(write=False)
    return x, g, ref


def mid_n_values(m):
    """An even n (two-real accesses in pass A) and an odd one (per-real)"""
    return [m // 2 + 2, m // 2 + 1]


def all_cases():
    """Every (m, n, channels, batch) of the sweep, and two batch entries of one channel at mid_length(N) of every factor length N > 64"""
    for m in LENGTHS:
        for batch, channels in rows_of(m):
            for n in n_values(m):
                yield m, n, channels, batch
    for N in FACTORS:
        if N > 64:
            for n in mid_n_values(mid_length(N)):
                yield mid_length(N), n, 1, 2


def nu_lines(got, ref, m, prec):
    """accuracy_ref.nu per channel line over the m/2 + 1 bins, n_eff = m"""
    return A.nu(got, ref, m, prec, (1,))


# ---- the gradient formulas in longdouble -------------------------------------------------------------------------------------------------
def ld_conv(x, H, m, n_out):
    """irfft(rfft(x, m) * H, m)[:, :n_out] of rows [rows][n] in longdouble, row r with H[r % channels]"""
    rows, n = x.shape
    xp = np.zeros((rows, m), dtype=LD)
    xp[:, :n] = x
    Y = A.ld_rfft(xp, 1) * np.asarray(H).astype(CLD)[np.arange(rows) % H.shape[0]]
    return (A.ld_irfft(Y, m, 1) / LD(m))[:, :n_out]


def bin_weights(m):
    """w / m: 1 / m at bins 0 and m/2, 2 / m elsewhere"""
    w = np.full(m // 2 + 1, LD(2) / LD(m), dtype=LD)
    w[0] = w[-1] = LD(1) / LD(m)
    return w
