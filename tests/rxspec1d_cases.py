"""The cases of the batched 1-D real cross-spectrum (dfft_rxspec1d) shared by tests/test_rxspec1d_host.py (which measures the CPU yardstick
on them) and tests/test_gpu_rxspec1d.py (which runs the library on them): inputs, longdouble references, and a restatement of the slice
rule from which the batches are chosen.  No GPU, no scipy.

Inputs come from accuracy_ref.rand_real (float32 values, so both precisions share one input and one reference).  The reference is
sum_b conj(X[b, c]) G[b, c] of accuracy_ref.ld_rfft on the zero-padded rows, in longdouble."""
from functools import lru_cache

import numpy as np

import accuracy_ref as A
import rconv1d_cases as RC

LD, CLD = A.LD, A.CLD
HALVES = RC.HALVES                      # 2, 8, 25, 48, 64, 243, 512, 1000, 1024, 4096 (tuned) and 36 (untuned)
CHANNELS = RC.CHANNELS                  # 1 and 3
n_values = RC.n_values                  # m, m/2, m/2 - 1, 1

# the slice rule of dfft_rxspec1d_slices (include/dfft.h): fixed constants, never the device
GROUPS_PER_PART = 512                   # two resident workgroups on each of 256 CUs ...
MAX_GROUP_FACTOR = 8                    # ... times the thread groups of a workgroup, at most 8
MIN_ROWS = 8                            # rows per slice, at least
# (M, precision) that rxspec_fused_ok of dfft_xspec.hip sends to the composed route: their fused kernels would spill
ROUTED = {(3125, "f64"), (3125, "f32"), (1536, "f64"), (200, "f64"), (384, "f64"), (400, "f64"), (640, "f64"), (1280, "f64"), (2401, "f64")}
BEYOND_TARGET = (8, 15, 3, 40000)       # (M, n, channels, batch): more rows than MIN_ROWS x the item-count target, about 29 rows per slice


def slices_rule(M, channels, batch):
    target = GROUPS_PER_PART * min(RC.rows_per_group(M), MAX_GROUP_FACTOR)
    return max(1, min(target // channels, batch // MIN_ROWS))


def slice_ranges(batch, slices):
    """[(first row, rows)] of the slices: contiguous, the first batch % slices of them one row longer"""
    per, rem = divmod(batch, slices)
    return [(s * per + min(s, rem), per + (1 if s < rem else 0)) for s in range(slices)]


def fused(M, prec):
    return M in RC.plan_points() and (M, prec) not in ROUTED


@lru_cache(maxsize=None)
def batches(M, channels):
    """1 (one slice of one row), and the smallest batch with two or more slices, a ragged last slice and -- G > 1 thread groups per
    workgroup -- an item count that leaves a ragged last workgroup (where G divides the channel count every item count is a whole
    number of workgroups, and the last condition is dropped)"""
    G = RC.rows_per_group(M)
    b = 2 * MIN_ROWS
    while True:
        s = slices_rule(M, channels, b)
        if s >= 2 and b % s and (G == 1 or channels % G == 0 or (channels * s) % G):
            return (1, b)
        b += 1


def reference(x, g, m, channels):
    """S[c][k] of rows [batch * channels][n] in longdouble"""
    rows, n = x.shape
    xp, gp = np.zeros((rows, m), dtype=LD), np.zeros((rows, m), dtype=LD)
    xp[:, :n], gp[:, :n] = x, g
    P = np.conj(A.ld_rfft(xp, 1)) * A.ld_rfft(gp, 1)
    return P.reshape(rows // channels, channels, m // 2 + 1).sum(axis=0)


@lru_cache(maxsize=8)
def case(M, n, channels, batch):
    """-> (x, g [batch * channels][n] float64, reference [channels][M + 1] clongdouble, auto-spectrum reference of x), frozen"""
    seed = 21000 + 16 * M + 4 * n + channels + 7 * (batch % 1000)
    x = A.rand_real((batch * channels, n), seed)
    g = A.rand_real((batch * channels, n), seed + 1)
    ref, auto = reference(x, g, 2 * M, channels), reference(x, x, 2 * M, channels)
    for a in (x, g, ref, auto):
        a.setflags(write=False)
    return x, g, ref, auto


def all_cases():
    """Every (M, n, channels, batch) of the sweep"""
    for M in HALVES:
        for channels in CHANNELS:
            for batch in batches(M, channels):
                for n in n_values(2 * M):
                    yield M, n, channels, batch
    yield BEYOND_TARGET


def nu_lines(got, ref, m, prec):
    """accuracy_ref.nu per channel line over the m/2 + 1 bins, n_eff = m"""
    return A.nu(got, ref, m, prec, (1,))
