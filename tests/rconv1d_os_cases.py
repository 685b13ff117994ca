"""The cases of the overlap-save 1-D real FFT convolution (dfft_rconv1d_os) shared by tests/test_rconv1d_os_host.py (which measures the
CPU yardstick on them) and tests/test_gpu_rconv1d_os.py (which runs the library on them): inputs, filters, longdouble references that
apply the block definition itself.  No GPU, no scipy.  Inputs and filters as in rconv1d_cases.py (float32 values, filter moduli in
[0.5, 2], so no reference row is identically zero)."""
from functools import lru_cache

import numpy as np

import accuracy_ref as A
import rconv1d_cases as RC

LD, CLD = A.LD, A.CLD
KINDS = RC.KINDS

# (M, d) -> what it reaches.  m = 2 M, S = m - d.
#   2      the smallest length, every discard
#   8      G = 256: 3 channels x 35 batches x 5 blocks = 525 items, workgroups straddle rows and channels, ragged last group; d even and odd
#   25     odd half-length; d = 49: S = 1
#   64     no overlap, even, odd and near-full discard
#   512    a mid-size tuned length
#   4096   G = 1, three blocks
#   36     untuned: the composed route
#   1536   routed in fp64 (composed), fused in fp32
ENTRIES = [(2, 0), (2, 1), (2, 2), (2, 3), (8, 6), (8, 5), (25, 10), (25, 49), (64, 0), (64, 32), (64, 33), (64, 126), (512, 256), (4096, 4096),
           (36, 10), (1536, 512)]
FIXED = {(8, 6): (48, 3, 35), (8, 5): (52, 3, 35), (25, 49): (6, 3, 2), (4096, 4096): (10240, 3, 1)}   # (M, d) -> (n, channels, batch); else swept
TUNED_HALVES = [2, 8, 25, 64, 512, 4096, 1536]
ROUTED = {(1536, "f64")}                 # tuned, but on the composed route (osconv_fused_ok of dfft_osconv.hip)
LOOP = {(8, 6): 4000, (4096, 4096): 400}  # (M, d) -> repeats of the FIXED case: more items than resident workgroups x G on 256 CUs


def fused(M, prec):
    return M in TUNED_HALVES and (M, prec) not in ROUTED


def blocks(n_out, m, d):
    return -(-n_out // (m - d))


def n_values(m, d):
    """n = 1, S - 1, S, S + 1, 2 S + S / 2, 3 S: below, at and above one block, a ragged and a whole last block"""
    S = m - d
    return sorted({n for n in (1, S - 1, S, S + 1, 2 * S + S // 2, 3 * S) if n >= 1})


def n_out_values(n, d):
    """n_out = n - 1, n, n + d: a ragged last block, the causal head, the full length (its last blocks may read only padding)"""
    return sorted({v for v in (n - 1, n, n + d) if v >= 1})


def entry_cases(M, d):
    """Every (M, d, n, n_out, channels, batch) of a table entry"""
    if (M, d) in FIXED:
        n, channels, batch = FIXED[(M, d)]
        ns = [n]
    else:
        channels, batch, ns = 3, 2, n_values(2 * M, d)
    for n in ns:
        for n_out in n_out_values(n, d):
            yield M, d, n, n_out, channels, batch


def all_cases():
    for M, d in ENTRIES:
        for kind in KINDS:
            for c in entry_cases(M, d):
                yield c + (kind,)


def gather(x, m, d, n_out):
    """The zero-filled blocks xb [rows][nb][m]: xb[r, b, i] = x[r, b S - d + i] inside [0, n), else 0"""
    rows, n = x.shape
    S, nb = m - d, blocks(n_out, m, d)
    idx = np.arange(nb)[:, None] * S - d + np.arange(m)[None, :]
    inside = (idx >= 0) & (idx < n)
    return np.where(inside[None], x[:, np.clip(idx, 0, n - 1)], 0)


def reference(x, H, m, d, n_out):
    """The block definition in longdouble on rows [rows][n] -> [rows][n_out], row r with H[r % channels]"""
    rows = x.shape[0]
    xb = gather(np.asarray(x).astype(LD), m, d, n_out)
    Y = A.ld_rfft(xb, 2) * np.asarray(H).astype(CLD)[np.arange(rows) % H.shape[0]][:, None, :]
    cb = A.ld_irfft(Y, m, 2) / LD(m)
    return cb[:, :, d:].reshape(rows, -1)[:, :n_out]


def convolve_reference(x, k, n_out):
    """numpy.convolve(x[r], k[r % channels])[:n_out] in longdouble"""
    return np.stack([np.convolve(x[r].astype(LD), k[r % k.shape[0]].astype(LD))[:n_out] for r in range(x.shape[0])])


@lru_cache(maxsize=1024)
def case(M, d, n, n_out, channels, batch, kind):
    """-> (x [batch * channels][n] float64, H [channels][M + 1], reference longdouble [batch * channels][n_out]), frozen"""
    m = 2 * M
    seed = 21000 + 64 * M + 8 * d + 4 * n + channels + (100 if kind == "complex" else 0)
    x = A.rand_real((batch * channels, n), seed)
    H = RC.make_filter(channels, m, kind, seed + 1)
    ref = reference(x, H, m, d, n_out)
    for a in (x, H, ref):
        a.setflags(write=False)
    return x, H, ref


def taps_spectrum(k, m):
    """rfft of the taps zero-padded to m, in longdouble"""
    kp = np.zeros((k.shape[0], m), dtype=LD)
    kp[:, :k.shape[1]] = k
    return A.ld_rfft(kp, 1)


def nu_rows(got, ref, m, prec):
    """accuracy_ref.nu per output row, n_eff = m"""
    return A.nu(got, ref, m, prec, (1,))
