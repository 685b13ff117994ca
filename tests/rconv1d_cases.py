"""The cases of the batched 1-D real FFT convolution (dfft_rconv1d) shared by tests/test_rconv1d_host.py (which measures the CPU yardstick
on them) and tests/test_gpu_rconv1d.py (which runs the library on them): inputs, filters, longdouble references.  No GPU, no scipy.

Inputs come from accuracy_ref.rand_real (float32 values, so both precisions share one input and one reference).  Filters have modulus in
[0.5, 2] (float32 values): real ones uniform, as in accuracy_ref.conv_case; complex ones those moduli with random phases."""
import re
from functools import lru_cache
from pathlib import Path

import numpy as np

import accuracy_ref as A

ROOT = Path(__file__).resolve().parent.parent
LD, CLD = A.LD, A.CLD

# half-lengths M (m = 2M): 2 the smallest; 8 with G = 256 rows per workgroup; 25 odd (no self-paired bin); 48 with E = 24 (split twiddles
# from the table); 4096 with G = 1 and the largest tile
TUNED_HALVES = [2, 8, 25, 48, 64, 243, 512, 1000, 1024, 4096]
UNTUNED_HALF = 36                       # 7-smooth without a plan of its own: the composed route
HALVES = TUNED_HALVES + [UNTUNED_HALF]
KINDS = ("real", "complex")
CHANNELS = (1, 3)
LOOP_HALVES = {8: 200000, 4096: 400}    # M -> batch (x 3 channels): more rows than resident workgroups x G on 256 CUs, so a workgroup loops


def n_values(m):
    """n = m (circular), m/2, m/2 - 1 (odd: per-real accesses, the cut inside a pair), 1"""
    out = []
    for n in (m, m // 2, m // 2 - 1, 1):
        if n >= 1 and n not in out:
            out.append(n)
    return out


@lru_cache(maxsize=1)
def plan_points():
    """M -> E of the plan table"""
    text = (ROOT / "distributedfft_amd" / "csrc" / "dfft_plans.h").read_text()
    return {int(n): int(e) for n, e in re.findall(r"^\s*X\((\d+),\s*\d+,\s*(\d+),", text, re.M)}


def rows_per_group(M):
    """G of the fused kernel: thread groups of T = M / E threads, about 256 threads per workgroup (1 for an untuned M)"""
    e = plan_points().get(M)
    return max(1, 256 // (M // e)) if e else 1


def batch_for(M, channels):
    """A batch whose rows fill more than one workgroup and leave a ragged last row group (G > 1; where G divides the channel count,
    M = 729 with three channels, every row count is a whole number of groups)"""
    G = rows_per_group(M)
    rows = G + G // 2 + 1 if G > 1 else 4
    batch = -(-rows // channels)
    while G > 1 and channels % G and (batch * channels) % G == 0:
        batch += 1
    return batch


def make_filter(channels, m, kind, seed):
    rng = np.random.default_rng(seed)
    mod = rng.uniform(0.5, 2.0, (channels, m // 2 + 1)).astype(np.float32).astype(np.float64)
    if kind == "real":
        return mod
    ph = rng.uniform(0.0, 2 * np.pi, mod.shape)
    return (mod * np.exp(1j * ph)).astype(np.complex64).astype(np.complex128)


def reference(x, H, m):
    """irfft(rfft(x, m) * H, m)[:n] of rows [rows][n] in longdouble, row r with H[r % channels]"""
    rows, n = x.shape
    xp = np.zeros((rows, m), dtype=LD)
    xp[:, :n] = x
    Y = A.ld_rfft(xp, 1) * np.asarray(H).astype(CLD)[np.arange(rows) % H.shape[0]]
    return (A.ld_irfft(Y, m, 1) / LD(m))[:, :n]


@lru_cache(maxsize=16)
def case(M, n, channels, batch, kind):
    """-> (x [batch * channels][n] float64, H [channels][M + 1], reference longdouble), frozen"""
    m = 2 * M
    seed = 11000 + 16 * M + 4 * n + channels + (100 if kind == "complex" else 0)
    x = A.rand_real((batch * channels, n), seed)
    H = make_filter(channels, m, kind, seed + 1)
    ref = reference(x, H, m)
    for a in (x, H, ref):
        a.setflags(write=False)
    return x, H, ref


def all_cases():
    """Every (M, n, channels, batch, kind) of the sweep"""
    for M in HALVES:
        for kind in KINDS:
            for channels in CHANNELS:
                for n in n_values(2 * M):
                    yield M, n, channels, batch_for(M, channels), kind


def nu_rows(got, ref, m, prec):
    """accuracy_ref.nu per row, n_eff = m"""
    return A.nu(got, ref, m, prec, (1,))
