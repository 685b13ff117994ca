"""Helpers of the accuracy tests (tests/test_accuracy_host.py, tests/test_gpu_accuracy.py): longdouble references, structured inputs
with exact references, the error measure nu in units of eps * sqrt(log2 n), the shared case builders, and the constants YARDSTICK
(same-precision CPU FFT), CEILING and BOUND (what a GPU result must stay under).  No GPU, no scipy.

Directions follow the library: +1 is the forward transform (exp(-2 pi i jk/n)), -1 the unnormalised backward one."""
from functools import lru_cache

import numpy as np

LD, CLD = np.longdouble, np.clongdouble

# A float64 reference is worthless for fp64 bounds: fail loudly (never skip) where numpy.fft does not keep extended precision.
assert np.finfo(LD).eps < 2e-19, f"np.longdouble is not extended precision here (eps = {np.finfo(LD).eps})"
assert np.fft.fft(np.ones(8, dtype=CLD)).dtype == CLD, "numpy.fft does not keep clongdouble: the references would be float64"

EPS = {"f64": 2.0 ** -52, "f32": 2.0 ** -23}
CDT = {"f64": np.complex128, "f32": np.complex64}
RDT = {"f64": np.float64, "f32": np.float32}
PRECS = ("f64", "f32")
TWO_PI = 2 * np.arccos(LD(-1))

# ---- the cases both test modules run --------------------------------------------------------------------------------------------------
FOUR_STEP = [8192, 6561, 15625, 10000, 12288, 65536, 1048576]      # 2^24 is left out: its longdouble reference takes more than a few seconds
BLUESTEIN = [11, 97, 1009, 2039, 2053, 10007, 65537]               # 2039 / 2053: either side of the one-launch limit
REAL_N = [16, 125, 243, 375, 512, 1009, 2048, 16384]               # 1009 runs Bluestein: a family of its own ("real-bluestein", "r2r-bluestein")
REAL_S = [1, 6, 7]
REAL_2D = [(64, 96), (243, 125)]
R2R_KINDS = ["dct2", "dct3", "dst2", "dst3"]
ONE_LAUNCH_2D = [(256, 256, 5), (512, 512, 3), (768, 512, 2)]      # the one-launch stage with its hoisted twiddle products
PLAIN_2D = [(243, 729, 2), (8192, 8, 2)]
PLANS_3D = [((64, 64, 64), 1), ((64, 64, 64), 4), ((25, 10, 16), 4), ((2048, 4, 16), 2), ((4, 2048, 24), 1), ((16, 256, 256), 1),
            ((4096, 2, 8), 1), ((8192, 16, 24), 1)]
PLANS_R2C = [((64, 64, 64), 2), ((25, 10, 16), 4)]
PLANS_CONV = [((64, 64, 64), 2), ((1024, 8, 16), 1)]

# ---- constants ------------------------------------------------------------------------------------------------------------------------
# YARDSTICK: nu of the same-precision CPU FFT (scipy.fft, pocketfft) on exactly the inputs of the GPU tests, worst case of the family,
# rounded up to the next 0.05 (impulse families: nu_impulse in eps, to the next 0.5); tests/test_accuracy_host.py recomputes them and
# asserts they hold.  Measured (fp64 / fp32): tuned 0.618 / 0.701 and generic 0.537 / 0.497 (the worst of 96 lines at n = 9, 6, 18;
# from 64 points upwards 0.27 ... 0.40), four-step 0.428 / 0.374, Bluestein 1.098 / 0.679 (n = 65537), impulses 4.39 / 3.33 (tuned),
# 3.57 / 2.31 (generic), 4.72 / 4.04 (four-step), 12.8 / 9.9 (Bluestein, n = 65537: the largest of 65537 bins that went through a
# convolution of length M), real 0.413 / 0.381, real at n = 1009 0.776 / 0.674, r2r 0.491 / 0.502, r2r at n = 1009 0.801 / 0.699,
# 2-D 0.402 / 0.372, one-launch 2-D shapes 0.307 / 0.312, 3-D 0.325 / 0.311, R2C 3-D 0.296 / 0.307, conv 0.311 / 0.326.
YARDSTICK = {
    "tuned":             {"f64": 0.65, "f32": 0.75},
    "generic":           {"f64": 0.55, "f32": 0.55},
    "four-step":         {"f64": 0.45, "f32": 0.40},
    "bluestein":         {"f64": 1.15, "f32": 0.70},
    "tuned-impulse":     {"f64": 4.5, "f32": 3.5},
    "generic-impulse":   {"f64": 4.0, "f32": 2.5},
    "four-step-impulse": {"f64": 5.0, "f32": 4.5},
    "bluestein-impulse": {"f64": 13.0, "f32": 10.0},
    "real":              {"f64": 0.45, "f32": 0.40},
    "real-bluestein":    {"f64": 0.80, "f32": 0.70},
    "r2r":               {"f64": 0.50, "f32": 0.55},
    "r2r-bluestein":     {"f64": 0.85, "f32": 0.75},
    "2d":                {"f64": 0.45, "f32": 0.40},
    "2d-one-launch":     {"f64": 0.35, "f32": 0.35},
    "3d":                {"f64": 0.35, "f32": 0.35},
    "r2c-3d":            {"f64": 0.35, "f32": 0.35},
    "conv":              {"f64": 0.35, "f32": 0.35},
}
# CEILING: no bound may exceed 8 x the yardstick of its family -- room for radix-8 stages on products of stored powers, conj-forward-conj
# inverses and the extra twiddle multiply of the real routes.  The complex 1-D families take the fixed figures the bounds were specified
# with, for both precisions: 3.2 for 7-smooth lengths (8 x 0.40, the CPU FFT from 64 points upwards -- stricter than 8 x the
# worst-of-96-lines figures above), 9 for Bluestein, 40 eps for every impulse (8 x 4.8; Bluestein's own yardstick would allow 104).
FIXED_CEILING = {"tuned": 3.2, "generic": 3.2, "four-step": 3.2, "bluestein": 9.0, "tuned-impulse": 40.0, "generic-impulse": 40.0,
                 "four-step-impulse": 40.0, "bluestein-impulse": 40.0}
CEILING = {f: {p: FIXED_CEILING.get(f, round(8 * YARDSTICK[f][p], 2)) for p in PRECS} for f in YARDSTICK}

# BOUND: 2 x the worst nu measured on an MI355X, rounded up to two digits (rounding error is statistical: another reduction order or seed
# moves nu by tens of percent, not by factors); tests/test_accuracy_host.py holds every bound under its CEILING.  tests/test_gpu_accuracy.py
# prints every nu and, at the end, the worst per family.  Measured (fp64 / fp32, and the case):
#   tuned             0.576 / 0.593   columns n = 6 width 32 / n = 3 width 21, random forward
#   generic           0.491 / 0.499   columns n = 18 width 32, random backward
#   four-step         0.372 / 0.358   rows n = 6561 forward / columns n = 65536 backward
#   bluestein         0.956 / 0.677   n = 11 along the middle axis, random backward
#   tuned-impulse     3.58 / 3.13     n = 4096, rows / columns of width 32
#   generic-impulse   2.64 / 2.99     rows n = 2000 / n = 3600
#   four-step-impulse 4.76 / 4.58     rows n = 1048576, impulse at n - 1
#   bluestein-impulse 8.60 / 6.49     n = 65537 along the last axis
#   real              0.402 / 0.417   irfft n = 243 s = 6 / n = 16 s = 7
#   real-bluestein    0.634 / 0.494   rfft n = 1009, s = 6 / s = 7
#   r2r               0.574 / 0.547   dst2 / dct3 at n = 16, s = 6
#   r2r-bluestein     0.639 / 0.519   dst2 / dst3 at n = 1009, s = 6
#   2d                0.389 / 0.349   243 x 729
#   2d-one-launch     0.328 / 0.337   512 x 512 forward
#   3d                0.304 / 0.350   (25, 10, 16) P = 4 backward unfused / (64, 64, 64) P = 4 forward unfused
#   r2c-3d            0.291 / 0.346   (64, 64, 64) P = 2
#   conv              0.351 / 0.405   PlanConv (64, 64, 64) P = 2
BOUND = {
    "tuned":             {"f64": 1.2, "f32": 1.2},
    "generic":           {"f64": 0.99, "f32": 1.0},
    "four-step":         {"f64": 0.75, "f32": 0.72},
    "bluestein":         {"f64": 2.0, "f32": 1.4},
    "tuned-impulse":     {"f64": 7.2, "f32": 6.3},
    "generic-impulse":   {"f64": 5.3, "f32": 6.0},
    "four-step-impulse": {"f64": 9.6, "f32": 9.2},
    "bluestein-impulse": {"f64": 18.0, "f32": 13.0},
    "real":              {"f64": 0.81, "f32": 0.84},
    "real-bluestein":    {"f64": 1.3, "f32": 0.99},
    "r2r":               {"f64": 1.2, "f32": 1.1},
    "r2r-bluestein":     {"f64": 1.3, "f32": 1.1},
    "2d":                {"f64": 0.78, "f32": 0.70},
    "2d-one-launch":     {"f64": 0.66, "f32": 0.68},
    "3d":                {"f64": 0.61, "f32": 0.70},
    "r2c-3d":            {"f64": 0.59, "f32": 0.70},
    "conv":              {"f64": 0.71, "f32": 0.81},
}


# ---- longdouble references ------------------------------------------------------------------------------------------------------------
def ld_fft(x, axis=-1, sign=+1):
    """Unnormalised transform along `axis` in clongdouble: sign=+1 forward, sign=-1 backward."""
    x = np.asarray(x).astype(CLD)
    return np.fft.fft(x, axis=axis) if sign > 0 else np.fft.ifft(x, axis=axis, norm="forward")


def ld_fftn(x, axes=None, sign=+1):
    x = np.asarray(x).astype(CLD)
    return np.fft.fftn(x, axes=axes) if sign > 0 else np.fft.ifftn(x, axes=axes, norm="forward")


def reverse_bins(F, axes):
    """F[(-k) mod n] along every listed axis: the unnormalised backward transform of x from its forward transform, exactly."""
    for a in axes:
        F = np.roll(np.flip(F, axis=a), 1, axis=a)
    return F


def ld_rfft(x, axis=-1):
    n = x.shape[axis]
    return np.take(ld_fft(x, axis, +1), range(n // 2 + 1), axis=axis)


def ld_irfft(X, n, axis=-1):
    """n * irfft(X, n): the imaginary parts of bin 0 and (n even) bin n/2 are ignored, as the library and numpy do."""
    X = np.moveaxis(np.asarray(X).astype(CLD), axis, -1).copy()
    assert X.shape[-1] == n // 2 + 1
    X[..., 0] = X[..., 0].real
    if n % 2 == 0:
        X[..., -1] = X[..., -1].real
    full = np.empty(X.shape[:-1] + (n,), dtype=CLD)
    full[..., :n // 2 + 1] = X
    full[..., n // 2 + 1:] = np.conj(X[..., (n - 1) // 2:0:-1])
    return np.moveaxis(ld_fft(full, -1, -1).real, -1, axis)


def ld_r2r(x, kind):
    """The mirror reference of tests/test_r2r_host.py in longdouble: [b][n][s], along axis 1, scipy.fft's norm=None."""
    x = np.asarray(x).astype(LD)
    b, n, s = x.shape
    alt = ((-1) ** np.arange(n)).astype(LD)[None, :, None]
    if kind == "dct2":
        u = np.zeros((b, 4 * n, s), dtype=LD)
        u[:, 1:2 * n:2, :] = x
        u[:, 4 * n - 1:2 * n:-2, :] = x
        return ld_fft(u, 1, +1)[:, :n, :].real
    if kind == "dct3":
        v = np.zeros((b, 4 * n, s), dtype=LD)
        v[:, :n, :] = 2 * x
        v[:, 0, :] = x[:, 0, :]
        return ld_fft(v, 1, +1)[:, 1:2 * n:2, :].real
    if kind == "dst2":
        return ld_r2r(x * alt, "dct2")[:, ::-1, :]
    if kind == "dst3":
        return alt * ld_r2r(x[:, ::-1, :], "dct3")
    raise ValueError(kind)


def ld_conv(x, H, real=False):
    """ifftn(fftn(x) * H) with numpy's normalisation; real=True: H is the half spectrum [N0][N1][N2/2+1] of a real-field plan."""
    if not real:
        return ld_fftn(ld_fftn(x, None, +1) * np.asarray(H).astype(CLD), None, -1) / LD(x.size)
    n2 = x.shape[2]
    Y = np.take(ld_fftn(x, None, +1), range(n2 // 2 + 1), axis=2) * np.asarray(H).astype(CLD)
    return ld_irfft(ld_fftn(Y, (0, 1), -1), n2, axis=2) / LD(x.size)


def ld_phase(r, n, sign):
    """exp(-sign * 2 pi i r / n) for int64 r already reduced mod n, evaluated in longdouble."""
    t = TWO_PI * r.astype(LD) / LD(n)
    return (np.cos(t) - sign * 1j * np.sin(t)).astype(CLD)


# ---- the measure ----------------------------------------------------------------------------------------------------------------------
def nu(got, ref, n_eff, prec, axes=(-1,)):
    """Worst line of ||got - ref||_2 / ||ref||_2 / (eps sqrt(log2 max(n_eff, 2))); a line spans `axes` (None: the whole array)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = got.astype(CLD if np.iscomplexobj(ref) or np.iscomplexobj(got) else LD) - ref
    ax = None if axes is None else tuple(axes)
    num = np.sqrt(np.sum(d.real ** 2 + d.imag ** 2, axis=ax))          # (not abs() ** 2: hypot in longdouble is slow)
    den = np.sqrt(np.sum(ref.real ** 2 + ref.imag ** 2, axis=ax))
    assert np.all(den > 0), "a reference line is identically zero"
    return float(np.max(num / den) / (EPS[prec] * np.sqrt(np.log2(max(n_eff, 2)))))


def nu_parts(pairs, n_eff, prec):
    """nu over (got, ref) pairs, each pair one line (one rank's whole output)."""
    return max(nu(g, r, n_eff, prec, axes=None) for g, r in pairs)


def nu_impulse(got, ref, prec):
    """max |got - ref| / eps: every reference bin of an impulse has modulus 1."""
    return float(np.max(np.abs(np.asarray(got).astype(CLD) - ref)) / EPS[prec])


def old_measure(got, ref):
    """The suite's existing pass mark: max |got - ref| / max |ref| over the whole output."""
    return float(np.max(np.abs(np.asarray(got) - ref)) / np.max(np.abs(ref)))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def rand_real(shape, seed):
    """Seeded standard normals rounded through float32: both precisions share one input and one reference."""
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32).astype(np.float64)


def rand_complex(shape, seed):
    r = np.random.default_rng(seed).standard_normal(tuple(shape) + (2,)).astype(np.float32).astype(np.float64)
    return r[..., 0] + 1j * r[..., 1]


def line_scales(count):
    """2^s, s cycling through -8 ... 8: exact, and a line that picks up a fraction of its neighbour fails on its own norm."""
    return 2.0 ** ((np.arange(count) % 17) - 8)


def _shape_scales(shape, axis):
    """line_scales over every index but `axis`, broadcastable to `shape`."""
    rest = [v for i, v in enumerate(shape) if i != axis % len(shape)]
    sc = line_scales(int(np.prod(rest))).reshape(rest)
    return np.expand_dims(sc, axis % len(shape))


@lru_cache(maxsize=2)
def _base_lines(n, base, seed):
    """`base` random lines and their forward transforms: shared by the row and the column case of a long length."""
    b = rand_complex((base, n), seed)
    return b, ld_fft(b, -1, +1)


@lru_cache(maxsize=8)
def complex_lines(n, shape, axis, seed, base=0):
    """Scaled random lines of length n along `axis` of `shape` -> (x complex128, forward transform clongdouble); the backward transform
    is reverse_bins(F, [axis]).  base > 0: only `base` distinct random lines, repeated under the different scales (the long lengths)."""
    assert shape[axis] == n
    ax = axis % len(shape)
    rest = [v for i, v in enumerate(shape) if i != ax]
    count = int(np.prod(rest))
    sc = line_scales(count).reshape(rest)[..., None]
    if base:
        b, Fb = _base_lines(n, base, seed)
        pick = (np.arange(count) % base).reshape(rest)
        x, F = b[pick] * sc, Fb[pick] * sc.astype(LD)
    else:
        x = rand_complex(rest + [n], seed) * sc
        F = ld_fft(x, -1, +1)
    return _frozen(np.ascontiguousarray(np.moveaxis(x, -1, ax)), np.moveaxis(F, -1, ax))


def impulse_positions(n):
    return [1 % n, n - 1, n // 3]


@lru_cache(maxsize=4)
def _impulse_bins(n, j):
    """The forward transform of the unit impulse at j, in closed form: shared by the row and the column case of a length."""
    return ld_phase((np.int64(j) * np.arange(n, dtype=np.int64)) % n, n, +1)


@lru_cache(maxsize=8)
def impulse_lines(n, shape, axis, positions):
    """Unit impulses along `axis`, line i at positions[i % len] -> (x, forward transform); backward: the conjugate."""
    ax = axis % len(shape)
    rest = [v for i, v in enumerate(shape) if i != ax]
    j = np.asarray(positions, dtype=np.int64)[np.arange(int(np.prod(rest))) % len(positions)].reshape(rest)
    x = np.zeros(rest + [n], dtype=np.complex128)
    np.put_along_axis(x, j[..., None], 1.0, axis=-1)
    uniq, inv = np.unique(j, return_inverse=True)          # one evaluation per distinct position
    F = np.stack([_impulse_bins(n, int(u)) for u in uniq])[inv.reshape(j.shape)]
    return _frozen(np.ascontiguousarray(np.moveaxis(x, -1, ax)), np.moveaxis(F, -1, ax))


@lru_cache(maxsize=8)
def tone_lines(n, shape, axis, prec):
    """exp(+2 pi i j0 m / n), j0 = n // 3, made in longdouble, rounded to the working type and scaled per line -> (x, ld_fft(x))."""
    ax = axis % len(shape)
    m = np.arange(n, dtype=np.int64)
    t = ld_phase((m * (n // 3)) % n, n, -1).astype(CDT[prec]).astype(np.complex128)
    view = [1] * len(shape)
    view[ax] = n
    x = np.ascontiguousarray(np.broadcast_to(t.reshape(view), shape) * _shape_scales(shape, axis))
    return _frozen(x, ld_fft(x, axis, +1))


@lru_cache(maxsize=4)
def real_lines(n, batch, s, seed):
    """[batch][n][s] reals (equal line scales: two lines of a pair share one transform) -> (x, rfft along axis 1)."""
    x = rand_real((batch, n, s), seed)
    return _frozen(x, ld_rfft(x, 1))


@lru_cache(maxsize=4)
def half_spectra(n, batch, s, seed):
    """[batch][n//2+1][s] random bins -> (X, n * irfft(X, n) along axis 1)."""
    X = rand_complex((batch, n // 2 + 1, s), seed)
    return _frozen(X, ld_irfft(X, n, 1))


@lru_cache(maxsize=2)
def real_planes(n1, n2, batch, seed):
    """-> (x [batch][n1][n2], rfft2 of every plane)."""
    x = rand_real((batch, n1, n2), seed)
    return _frozen(x, ld_fft(ld_rfft(x, 2), 1, +1))


@lru_cache(maxsize=2)
def half_planes(n1, n2, batch, seed):
    """-> (X [batch][n1][n2//2+1], n1 n2 irfft2(X, s=(n1, n2)): backward along n1, then the real backward transform along n2)."""
    X = rand_complex((batch, n1, n2 // 2 + 1), seed)
    return _frozen(X, ld_irfft(ld_fft(X, 1, -1), n2, 2))


@lru_cache(maxsize=4)
def r2r_lines(n, batch, s, seed):
    x = rand_real((batch, n, s), seed)
    return (_frozen(x),) + tuple(_frozen(ld_r2r(x, k)) for k in R2R_KINDS)


@lru_cache(maxsize=2)
def complex_planes(n1, n2, batch, seed):
    """Scaled random planes -> (x, fft2 of every plane); backward: reverse_bins(F, (1, 2))."""
    x = rand_complex((batch, n1, n2), seed) * line_scales(batch)[:, None, None]
    return _frozen(x, ld_fftn(x, (1, 2), +1))


@lru_cache(maxsize=2)
def complex_volume(N, seed):
    """-> (x [N0][N1][N2], fftn(x)); the unnormalised inverse of x read as a spectrum is reverse_bins(F, (0, 1, 2))."""
    x = rand_complex(N, seed)
    return _frozen(x, ld_fftn(x, None, +1))


@lru_cache(maxsize=2)
def real_volume(N, seed):
    """-> (x real [N0][N1][N2], rfftn(x) [N0][N1][N2/2+1])."""
    x = rand_real(N, seed)
    return _frozen(x, np.take(ld_fftn(x, None, +1), range(N[2] // 2 + 1), axis=2))


@lru_cache(maxsize=2)
def conv_case(N, real, seed):
    """-> (x, H, ifftn(fftn(x) H)): H real, uniform in [0.5, 2] (float32 values), which keeps the reference norm away from cancellation."""
    x = rand_real(N, seed) if real else rand_complex(N, seed)
    hs = (N[0], N[1], N[2] // 2 + 1) if real else N
    H = np.random.default_rng(seed + 1).uniform(0.5, 2.0, hs).astype(np.float32).astype(np.float64)
    return _frozen(x, H, ld_conv(x, H, real))


def slab(n, P, g):
    blk = -(-n // P)
    return g * blk, (blk if g < P - 1 else n - (P - 1) * blk)


def split_x(x, P):
    """[N0][...] -> the devices' X slabs"""
    return [np.ascontiguousarray(x[s:s + c]) for s, c in (slab(x.shape[0], P, g) for g in range(P))]


def split_bins(F, P):
    """[N0][N1][W] -> per device [y_local][W][N0], a forward plan's output layout"""
    return [np.ascontiguousarray(F[:, s:s + c, :].transpose(1, 2, 0)) for s, c in (slab(F.shape[1], P, g) for g in range(P))]


# ---- bookkeeping of the GPU tests -----------------------------------------------------------------------------------------------------
WORST = {}   # (family, prec) -> (worst nu, case) of this process


def check(family, prec, value, what):
    """Print the figure (as the other GPU tests print their errors), keep the worst per family, and hold it against BOUND."""
    print(f"accuracy {family} {prec} {what}: nu {value:.3f}")
    if value > WORST.get((family, prec), (-1.0, ""))[0]:
        WORST[(family, prec)] = (value, what)
    assert value <= BOUND[family][prec], (family, prec, what, value, BOUND[family][prec])
