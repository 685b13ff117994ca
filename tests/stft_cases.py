"""The cases of the batched short-time Fourier transform (dfft_stft1d / dfft_istft1d) shared by tests/test_stft_host.py and
tests/test_gpu_stft.py: inputs, windows, and longdouble references that apply the definition itself -- frames built with index
arithmetic, accuracy_ref.ld_rfft / ld_irfft, overlap-add in longdouble.  No GPU, no scipy.  Inputs and windows hold float32 values, so
both precisions share one input and one reference; the windows are bounded away from zero (Hann + 0.1, rectangular), so no reference
frame is identically zero (accuracy_ref.nu asserts it)."""
from functools import lru_cache

import numpy as np

import accuracy_ref as A

LD, CLD = A.LD, A.CLD
MODES = ("reflect", "zero")
KINDS = ("complex", "power")
MODE_CODE = {"zero": 0, "reflect": 1}
KIND_CODE = {"complex": 0, "power": 1}
ROWS = 3

# (M, dtype) that are tuned but run the composed route (stft_fused_ok of dfft_stft.hip)
ROUTED = {(3125, "f64"), (2401, "f64")}
TUNED_HALVES = [2, 8, 25, 64, 512, 4096, 3125]
UNTUNED_HALVES = [18]


def fused(M, prec):
    return M in TUNED_HALVES and (M, prec) not in ROUTED


def _base(M):
    """hop = m / 4, pad = m / 2, a few frames long, Hann + 0.1"""
    m = 2 * M
    return (M, max(1, m // 4), M, 3 * m + 2, "hann")


# (M, hop, pad, n, window): one factor at a time around the base case M = 64 (m = 128), hop = 32, pad = 64, n = 386.
#   half lengths  2 the smallest, 8 (256 items per workgroup step), 25 odd (pad = 25 and hop = 12: no two-real loads), 64, 512, 4096 (one
#                 item per workgroup), 3125 tuned but routed to the composed form, 18 untuned
#   hops          1, odd, m / 4, m, m + 3 (gaps between the frames)
#   pads          0, 1 (odd: per-real loads), m / 2, m - 1
#   row lengths   below m, m, odd, a few frames; n = 100 with pad = 64 mirrors more than half a row
#   windows       Hann + 0.1 and rectangular
# n, hop and pad are all even in the base case (whole frames load two reals per access, the frames at the row ends do not: the switch
# inside one call) and each of them is odd in at least one case.
FORWARD = ([_base(M) for M in (2, 8, 25, 64, 512, 4096, 3125, 18)] +
           [(64, hop, 64, 386, "hann") for hop in (1, 7, 128, 131)] +
           [(64, 32, pad, 386, "hann") for pad in (0, 1, 127)] +
           [(64, 32, 64, n, "hann") for n in (100, 128, 301, 640)] +
           [(64, 32, 64, 386, "rect"), (64, 32, 0, 128, "rect"), (8, 4, 8, 9, "rect"), (18, 5, 3, 77, "rect")])

# More items than resident workgroups x G on 256 CUs: (M, hop, pad, n, window) -> repeats of its ROWS rows along the batch
LOOP = {(8, 4, 8, 2000, "hann"): 1400, (4096, 2048, 4096, 12288, "hann"): 70}

# Inverse, (M, hop, pad, frames, window): Hann + 0.1 and rectangular, hop = m / 4, m / 2, m and an odd value below m, pad = 0 and m / 2,
# tuned and untuned M; n is the longest the frames reach, (frames - 1) hop + m - pad, and in one case each a shorter and a one-sample row
INVERSE = ([(64, hop, pad, 9, win) for hop in (32, 64, 128, 37) for pad in (0, 64) for win in ("hann", "rect")] +
           [(M, max(1, M // 2), M, 6, "hann") for M in (2, 8, 25, 512, 4096, 3125, 18)] +
           [(18, 7, 0, 11, "rect"), (18, 36, 18, 4, "hann")])
INVERSE_SHORT = {(64, 32, 64, 9, "hann"): 200, (64, 37, 0, 9, "rect"): 1}   # case -> n below the longest


def frames_of(n, m, hop, pad):
    return 1 + (n + 2 * pad - m) // hop if n + 2 * pad >= m else 0


def window(m, kind):
    """Hann (periodic) + 0.1, or ones; float32 values"""
    if kind == "rect":
        return np.ones(m)
    assert kind == "hann"
    return (0.6 - 0.5 * np.cos(2 * np.pi * np.arange(m) / m)).astype(np.float32).astype(np.float64)


def gather(x, m, hop, pad, frames, mode):
    """xb [rows][frames][m]: xb[r, f, i] = P(x[r], f hop - pad + i), outside [0, n) zero or the mirrored sample"""
    n = x.shape[1]
    idx = np.arange(frames)[:, None] * hop - pad + np.arange(m)[None, :]
    inside = (idx >= 0) & (idx < n)
    if mode == "reflect":
        assert pad < n
        mir = np.where(idx < 0, -idx, 2 * (n - 1) - idx)
        assert np.all((mir >= 0) & (mir < n) | inside)
        return x[:, np.where(inside, idx, np.clip(mir, 0, n - 1))]
    return np.where(inside[None], x[:, np.clip(idx, 0, n - 1)], 0)


def reference(x, win, m, hop, pad, frames, mode, scale=1.0):
    """The definition in longdouble: [rows][n] -> [rows][frames][m/2 + 1]"""
    xb = gather(np.asarray(x).astype(LD), m, hop, pad, frames, mode) * np.asarray(win).astype(LD)
    return A.ld_rfft(xb, 2) * LD(scale)


def power(X):
    return X.real ** 2 + X.imag ** 2


def envelope(win, m, hop, frames):
    """sum_f win^2[s - f hop], s in [0, (frames - 1) hop + m), in longdouble"""
    env = np.zeros((frames - 1) * hop + m, dtype=LD)
    w2 = np.asarray(win).astype(LD) ** 2
    for f in range(frames):
        env[f * hop:f * hop + m] += w2
    return env


def inverse_reference(X, win, inv_env, n, m, hop, pad):
    """out[r][t] = inv_env[t] sum_f win[i] c_f[i] / m, i = t + pad - f hop, c_f = m irfft(X[r][f], m), in longdouble"""
    rows, frames = X.shape[:2]
    c = A.ld_irfft(X, m, 2) * np.asarray(win).astype(LD) / LD(m)
    y = np.zeros((rows, (frames - 1) * hop + m), dtype=LD)
    for f in range(frames):
        y[:, f * hop:f * hop + m] += c[:, f]
    return y[:, pad:pad + n] * np.asarray(inv_env).astype(LD)


@lru_cache(maxsize=256)
def forward_case(M, hop, pad, n, wkind, mode, rows=ROWS):
    """-> (x [rows][n] float64, win [m], frames, reference clongdouble [rows][frames][M + 1]), frozen"""
    m = 2 * M
    frames = frames_of(n, m, hop, pad)
    assert frames >= 1
    x = A.rand_real((rows, n), 31000 + 64 * M + 8 * hop + 4 * pad + n)
    win = window(m, wkind)
    ref = reference(x, win, m, hop, pad, frames, mode)
    for a in (x, win, ref):
        a.setflags(write=False)
    return x, win, frames, ref


def usable(case, mode):
    """reflect padding needs pad < n"""
    M, hop, pad, n, _ = case
    return mode == "zero" or pad < n


@lru_cache(maxsize=256)
def inverse_case(M, hop, pad, frames, wkind, rows=ROWS):
    """-> (X [rows][frames][M + 1] complex128, win [m], inv_env [n] (float32 values), n, reference longdouble [rows][n]), frozen.  Where the
    envelope has gaps (hop > m never happens here) inv_env would be infinite: the cases keep hop <= m."""
    m = 2 * M
    assert hop <= m
    n = INVERSE_SHORT.get((M, hop, pad, frames, wkind), (frames - 1) * hop + m - pad)
    X = A.rand_complex((rows, frames, M + 1), 33000 + 64 * M + 8 * hop + pad + frames)
    win = window(m, wkind)
    env = envelope(win, m, hop, frames)[pad:pad + n]
    assert env.min() > 0.009
    inv_env = (1 / env).astype(np.float32).astype(np.float64)
    ref = inverse_reference(X, win, inv_env, n, m, hop, pad)
    for a in (X, win, inv_env, ref):
        a.setflags(write=False)
    return X, win, inv_env, n, ref


def nu_frames(got, ref, m, prec):
    """accuracy_ref.nu per frame (the last axis), n_eff = m"""
    return A.nu(got, ref, m, prec, (-1,))


def nu_rows(got, ref, m, prec):
    """accuracy_ref.nu per output row, n_eff = m"""
    return A.nu(got, ref, m, prec, (-1,))
