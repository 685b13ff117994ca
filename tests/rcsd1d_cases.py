"""The cases of the framed (Welch) 1-D real cross-spectrum (dfft_rcsd1d) shared by tests/test_rcsd1d_host.py (which measures the CPU
yardstick on them) and tests/test_gpu_rcsd1d.py (which runs the library on them): inputs, windows, longdouble references, and a
restatement of the slice rule from which the frame counts are chosen.  No GPU, no scipy.

Inputs come from accuracy_ref.rand_real (float32 values, so both precisions share one input and one reference); the Hann window is
rounded through float32 for the same reason.  The reference frames the rows with numpy, multiplies by the window, applies
accuracy_ref.ld_rfft, conjugate-multiplies and sums over the frames, all in longdouble."""
from functools import lru_cache

import numpy as np

import accuracy_ref as A
import rconv1d_cases as RC

LD, CLD = A.LD, A.CLD
HALVES = RC.HALVES                      # 2, 8, 25, 48, 64, 243, 512, 1000, 1024, 4096 (tuned) and 36 (untuned)
ROWS = (1, 3)
WINDOWS = ("hann", "rect")

# the slice rule of dfft_rcsd1d_slices (include/dfft.h): fixed constants, never the device
GROUPS_PER_PART = 512                   # two resident workgroups on each of 256 CUs ...
MAX_GROUP_FACTOR = 32                   # ... times the thread groups of a workgroup, at most 32
MIN_FRAMES = 8                          # frames per slice, at least
# (M, precision) that rcsd_fused_ok of dfft_csd.hip sends to the composed route: the cross kernel would spill -- or, (1024, fp32), was
# measured no faster than the composed route -- and the lighter auto-spectrum kernel would
ROUTED = {(3125, "f64"), (3125, "f32"), (1536, "f64"), (200, "f64"), (384, "f64"), (400, "f64"), (640, "f64"), (1280, "f64"), (2401, "f64"),
          (48, "f64"), (80, "f64"), (96, "f64"), (100, "f64"), (160, "f64"), (192, "f64"), (320, "f64"), (4096, "f64"), (1024, "f32")}
ROUTED_AUTO = {(3125, "f64"), (3125, "f32"), (1280, "f64"), (1536, "f64"), (2401, "f64")}
# (M, rows, frames, hop, tail, window): one frame pair per row, more rows than a 256-CU part holds thread groups of the 8-point kernel
# (256 per workgroup), so a workgroup loops
BEYOND_TARGET = (8, 600001, 2, 3, 1, "hann")


def slices_rule(M, rows, frames):
    target = GROUPS_PER_PART * min(RC.rows_per_group(M), MAX_GROUP_FACTOR)
    return max(1, min(target // rows, frames // MIN_FRAMES))


def slice_ranges(frames, slices):
    """[(first frame, frames)] of the slices: contiguous, the first frames % slices of them one frame longer"""
    per, rem = divmod(frames, slices)
    return [(s * per + min(s, rem), per + (1 if s < rem else 0)) for s in range(slices)]


def fused(M, prec, autos=False):
    return M in RC.plan_points() and (M, prec) not in (ROUTED_AUTO if autos else ROUTED)


@lru_cache(maxsize=None)
def frame_counts(M, rows):
    """1 (one slice of one frame), and the smallest frame count with two or more slices, a ragged last slice and -- G > 1 thread groups
    per workgroup -- an item count rows * slices that leaves a ragged last workgroup: 17 where two slices do (where G divides the row
    count every item count is a whole number of workgroups, and the last condition is dropped)"""
    G = RC.rows_per_group(M)
    f = 2 * MIN_FRAMES
    while True:
        s = slices_rule(M, rows, f)
        if s >= 2 and f % s and (G == 1 or rows % G == 0 or (rows * s) % G):
            return (1, f)
        f += 1


def hops(M):
    """m/2 (two reals per access where it is even), m (no overlap), an odd hop (real by real) and, for M <= 64, 1"""
    m = 2 * M
    odd = M + 1 if M % 2 == 0 else M + 2
    out = [M, m, odd] + ([1] if M <= 64 else [])
    return sorted(set(out))


def tails(hop):
    """samples behind the last whole frame: none, and an odd count below hop (an odd n puts rows 1 and 2 on odd bases)"""
    return (0,) if hop < 2 else (0, 3 if hop > 3 else 1)


def window(name, m):
    """m window values, float32-exact: the periodic Hann window, or ones"""
    if name == "rect":
        return np.ones(m)
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(m) / m)).astype(np.float32).astype(np.float64)


def frames_of(x, m, hop):
    """[rows][n] -> the whole frames [rows][frames][m], frame f the samples [f hop, f hop + m)"""
    return np.lib.stride_tricks.sliding_window_view(x, m, axis=1)[:, ::hop]


def reference(x, g, win, m, hop):
    """out[r][k] = sum_f conj(rfft(win x_f)[k]) rfft(win g_f)[k] of rows [rows][n] in longdouble"""
    w = np.asarray(win).astype(LD)
    X = A.ld_rfft(frames_of(x, m, hop).astype(LD) * w, 2)
    G = X if g is x else A.ld_rfft(frames_of(g, m, hop).astype(LD) * w, 2)
    return (np.conj(X) * G).sum(axis=1)


@lru_cache(maxsize=8)
def case(M, rows, frames, hop, tail, wname):
    """-> (x, g [rows][n] float64, window [m], reference [rows][M + 1] clongdouble, auto-spectrum reference of x), frozen"""
    m = 2 * M
    n = (frames - 1) * hop + m + tail
    seed = 31000 + 16 * M + 4 * hop + rows + 7 * frames + tail
    x = A.rand_real((rows, n), seed)
    g = A.rand_real((rows, n), seed + 1)
    win = window(wname, m)
    ref, auto = reference(x, g, win, m, hop), reference(x, x, win, m, hop)
    assert ref.shape == (rows, M + 1) and frames_of(x, m, hop).shape[1] == frames
    for a in (x, g, win, ref, auto):
        a.setflags(write=False)
    return x, g, win, ref, auto


def cases_of(M):
    """Every (M, rows, frames, hop, tail, window) of the sweep for one half-length"""
    for rows in ROWS:
        for frames in frame_counts(M, rows):
            for hop in hops(M):
                for tail in tails(hop):
                    for wname in WINDOWS:
                        yield M, rows, frames, hop, tail, wname


def all_cases():
    for M in HALVES:
        yield from cases_of(M)
    yield BEYOND_TARGET


def nu_lines(got, ref, m, prec):
    """accuracy_ref.nu per row over the m/2 + 1 bins, n_eff = m"""
    return A.nu(got, ref, m, prec, (1,))
