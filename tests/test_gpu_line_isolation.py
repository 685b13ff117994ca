"""Which lines of a batch share arithmetic, on the GPU (tests/line_isolation.py has the rules and the checks): every plan-less batched entry
point runs a clean case and the same case with ONE line poisoned -- all NaN, times 2^24, zero; one NaN sample where a family has
locality inside a row -- for the first line, an interior even line, its odd neighbour and the last line.  Every line outside the
documented dirty set must be bit-identical to the clean run, every element whose longdouble reference is non-finite must be
non-finite, an unpaired line is exactly 2^24 times its clean result / exactly zero, and the lines of the paired real routes stay under
their family's accuracy_ref.BOUND relative to the PAIR's norm (nu_pair).  One more case per family holds NaN in the INPUT guards, one
element past a 16-byte boundary: the result must be bit-identical to the run with sentinel guards (a read outside `in` that reaches a
result shows here).

Both precisions throughout; the shapes are the smallest that reach every route (tuned, run-time-scheduled, four-step, Bluestein, fused
and composed, ragged and odd ends).  DESIGN.md "Which lines share arithmetic" is the contract in words."""
import os

import numpy as np
import pytest

import accuracy_ref as A
import line_isolation as LI
import mem_contract as MC
import rconv1d_cases as RC
import rconv1d_os_cases as OC
import stft_cases as SC

pytestmark = pytest.mark.gpu
FWD, BWD = +1, -1
LD, CLD = A.LD, A.CLD

# The worst nu_pair per family measured on an MI355X (fp64 / fp32; the bound is the family's accuracy_ref.BOUND entry, whose measure -- a
# line's own norm at equal scales -- is about sqrt 2 tighter than this one).  The module prints every figure and, at its end, these:
#   rfft rows              0.582 / 0.453   n = 97 (Bluestein), batch 5  (bound real-bluestein 1.3 / 0.99; CPU model 0.400 / 0.391)
#   irfft rows             0.618 / 0.410   n = 97  (bound real-bluestein 1.3 / 0.99; CPU model 0.366 / 0.394)
#   rfft columns           0.600 / 0.440   n = 97, s = 5  (bound real-bluestein 1.3 / 0.99; CPU model 0.406 / 0.401)
#   irfft columns          0.561 / 0.416   n = 97, s = 5  (bound real-bluestein 1.3 / 0.99; CPU model 0.446 / 0.413)
#   rfft2 planes           0.288 / 0.329   5 x 15, batch 3  (bound real 0.81 / 0.84; CPU model 0.310 / 0.370)
#   irfft2 planes          0.289 / 0.333   5 x 15, batch 3  (bound real 0.81 / 0.84; CPU model 0.371 / 0.348)
#   r2r rows               0.621 / 0.458   dst3 / dst2 at n = 97, fused  (bound r2r-bluestein 1.3 / 1.1; CPU model 0.440 / 0.512)
#   r2r columns            0.635 / 0.515   dct2 at n = 97 s = 5 / n = 15 s = 4, fused  (bound r2r-bluestein 1.3 / r2r 1.1; CPU model 0.486 / 0.541)
#   rconv1d_long composed  0.410 / 0.352   m = 10240, n = 5121, 6 rows  (bound rconv1d_long 1.2 / 1.1; CPU model 0.371 / 0.348)
_REF = {}   # (case, poison key) -> longdouble reference, shared by both precisions and by the routes of a case


def _cached(case, fn):
    def ref(v, key):
        if (case, key) not in _REF:
            _REF[(case, key)] = fn(v)
        return _REF[(case, key)]
    return ref


@pytest.fixture(scope="module", autouse=True)
def _worst_per_family():
    yield
    _REF.clear()
    for (label, prec), (value, what) in sorted(LI.WORST.items()):
        print(f"line isolation worst {label} {prec}: nu_pair {value:.3f}  {what}")


class _env:
    """An environment variable the library reads per call, set for the calls inside"""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        if self.value is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.old


def _composed(name, on):
    """name=0 for the calls inside where `on`; else the variable as the caller's environment has it"""
    return _env(name, "0" if on else os.environ.get(name))


def _tdt(x, prec):
    import torch
    if np.iscomplexobj(x):
        return torch.complex128 if prec == "f64" else torch.complex64
    return torch.float64 if prec == "f64" else torch.float32


def _gpu(x, prec, gpu):
    """numpy (float32-exact values, or NaN) -> device tensor of the working precision"""
    import torch
    return torch.from_numpy(np.array(x, order="C")).to(_tdt(x, prec)).to(gpu)


def _host(t):
    return t.cpu().numpy()


# ---- the complex families: no partners --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("direction", [FWD, BWD])
@pytest.mark.parametrize("n", [16, 360, 8192])
def test_fft1d_rows(gpu, n, direction, prec):
    from distributedfft_amd import api
    x, _ = A.complex_lines(n, (LI.BATCH, n), 1, 1000 + n)
    LI.check_case(lambda v: _host(api.fft1d_rows(_gpu(v, prec, gpu), direction)), _cached(("rows", n, direction), lambda v: A.ld_fft(v, 1, direction)),
                  x, lambda q: (q,), LI.lines_rows, LI.partners_none, prec, f"fft1d_rows n={n} dir={direction}", "rows")


def _offset_tensor(x, prec, gpu, offset):
    """x in a guarded buffer, `offset` elements past a 16-byte boundary -> (buffer, view shaped like x)"""
    buf, view = MC.guarded(x.size, _tdt(x, prec), gpu, offset)
    view.copy_(_gpu(x, prec, gpu).reshape(-1))
    return buf, view.reshape(x.shape)


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("w", [4, 5])
@pytest.mark.parametrize("n", [16, 360, 8192])
def test_fft1d_cols(gpu, n, w, prec):
    """columns of (2, n, w); in fp32 once more with both pointers only 8-byte aligned (the scalar kernels instead of the column pairs)"""
    import torch
    from distributedfft_amd import api
    x, _ = A.complex_lines(n, (2, n, w), 1, 1000 + n)
    ref = _cached(("cols", n, w), lambda v: A.ld_fft(v, 1, +1))

    def run(v, offset=0):
        if not offset:
            return _host(api.fft1d_cols(_gpu(v, prec, gpu), FWD))
        _, xv = _offset_tensor(v, prec, gpu, 1)
        _, ov = MC.guarded(v.size, xv.dtype, gpu, 1)
        assert xv.data_ptr() % 16 == 8 and ov.data_ptr() % 16 == 8
        api.fft1d_cols(xv, FWD, out=ov.reshape(v.shape))
        torch.cuda.synchronize()
        return _host(ov.reshape(v.shape))
    LI.check_case(run, ref, x, lambda q: LI.cols_index(x.shape, q), LI.lines_cols, LI.partners_none, prec, f"fft1d_cols n={n} w={w}", "cols")
    if prec == "f32":
        LI.check_case(lambda v: run(v, 1), ref, x, lambda q: LI.cols_index(x.shape, q), LI.lines_cols, LI.partners_none, prec,
                      f"fft1d_cols n={n} w={w} 8-byte base", "cols")
    LI.check_case(lambda v: _host(api.fft1d_cols(_gpu(v, prec, gpu), BWD)), _cached(("cols", n, w, BWD), lambda v: A.ld_fft(v, 1, -1)), x,
                  lambda q: LI.cols_index(x.shape, q), LI.lines_cols, LI.partners_none, prec, f"fft1d_cols n={n} w={w} bwd", "cols")


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("n", [11, 4099])
def test_fft1d_any(gpu, n, prec):
    """Bluestein, one launch and multi-pass: the last axis of (5, n) and the middle axis of (2, n, 3)"""
    from distributedfft_amd import api
    assert api.length_kind(n) == 3
    x, _ = A.complex_lines(n, (LI.BATCH, n), 1, 1000 + n)
    for d in (FWD, BWD):
        LI.check_case(lambda v: _host(api.fft1d_any(_gpu(v, prec, gpu), -1, d)), _cached(("any", n, d), lambda v: A.ld_fft(v, 1, d)), x,
                      lambda q: (q,), LI.lines_rows, LI.partners_none, prec, f"fft1d_any n={n} last axis dir={d}", "any")
    y, _ = A.complex_lines(n, (2, n, 3), 1, 1000 + n)
    LI.check_case(lambda v: _host(api.fft1d_any(_gpu(v, prec, gpu), 1, FWD)), _cached(("any", n, "mid"), lambda v: A.ld_fft(v, 1, +1)), y,
                  lambda q: LI.cols_index(y.shape, q), LI.lines_cols, LI.partners_none, prec, f"fft1d_any n={n} middle axis s=3", "any")


@pytest.mark.parametrize("n1,n2,prec", [(n1, n2, p) for n1, n2 in [(7, 8), (8192, 8)] for p in A.PRECS] + [(256, 256, "f64")])
def test_fft2d_batch(gpu, n1, n2, prec):
    """planes of (3, n1, n2): two launches per group, four-step columns, and (fp64 only: the route is built for it) the one-launch stage"""
    from distributedfft_amd import api
    x, _ = A.complex_planes(n1, n2, LI.PLANES, 7000 + n1)
    for d in (FWD, BWD):
        LI.check_case(lambda v: _host(api.fft2d_batch(_gpu(v, prec, gpu), d)), _cached(("2d", n1, n2, d), lambda v: A.ld_fftn(v, (1, 2), d)), x,
                      lambda q: (q,), LI.lines_planes, LI.partners_none, prec, f"fft2d_batch {n1}x{n2} dir={d}", "2d", lines=[0, 1, 2])


# ---- the paired real routes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("n", LI.RFFT_ROWS_N)
def test_rfft1d_rows(gpu, n, prec):
    """(5, n): form 1 rows are independent; forms 2 and 3 pair rows (0, 1) and (2, 3), row 4 goes with zeros"""
    from distributedfft_amd import api
    paired = n not in LI.UNPAIRED_ROWS_N
    assert (api.real_form(n) != 1) == paired
    partners = (lambda q: LI.partners_rows(q, LI.BATCH)) if paired else LI.partners_none
    fam = LI.real_family(n) if paired else None
    assert (api.length_kind(n) == 3) == (n in LI.BLUESTEIN_N)
    x, _ = A.real_lines(n, LI.BATCH, 1, 2000 + n)
    X, _ = A.half_spectra(n, LI.BATCH, 1, 3000 + n)
    x, X = x[:, :, 0], X[:, :, 0]
    LI.check_case(lambda v: _host(api.rfft1d(_gpu(v, prec, gpu))), _cached(("rfft", n), lambda v: A.ld_rfft(v, 1)), x, lambda q: (q,),
                  LI.lines_rows, partners, prec, f"rfft1d n={n}", "rfft rows", fam, n)
    LI.check_case(lambda v: _host(api.irfft1d(_gpu(v, prec, gpu), n)), _cached(("irfft", n), lambda v: A.ld_irfft(v, n, 1)), X, lambda q: (q,),
                  LI.lines_rows, partners, prec, f"irfft1d n={n}", "irfft rows", fam, n)


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("s", LI.STRIDED_S)
@pytest.mark.parametrize("n", LI.STRIDED_N)
def test_rfft1d_strided(gpu, n, s, prec):
    """dim 1 of (2, n, s): columns 2c / 2c + 1 inside an item; with s = 5 column 4 goes with zeros, never with the next item's column 0"""
    from distributedfft_amd import api
    partners = lambda q: LI.partners_cols(q, 2, s)   # noqa: E731
    fam = LI.real_family(n)
    x, _ = A.real_lines(n, 2, s, 2000 + n)
    X, _ = A.half_spectra(n, 2, s, 3000 + n)
    LI.check_case(lambda v: _host(api.rfft1d(_gpu(v, prec, gpu), dim=1)), _cached(("rfft-s", n, s), lambda v: A.ld_rfft(v, 1)), x,
                  lambda q: LI.cols_index(x.shape, q), LI.lines_cols, partners, prec, f"rfft1d dim=1 n={n} s={s}", "rfft cols", fam, n)
    LI.check_case(lambda v: _host(api.irfft1d(_gpu(v, prec, gpu), n, dim=1)), _cached(("irfft-s", n, s), lambda v: A.ld_irfft(v, n, 1)), X,
                  lambda q: LI.cols_index(X.shape, q), LI.lines_cols, partners, prec, f"irfft1d dim=1 n={n} s={s}", "irfft cols", fam, n)


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("n1,n2", LI.RFFT_2D)
def test_rfft2d_batch(gpu, n1, n2, prec):
    """planes of (3, n1, n2).  n2 = 16 (real form 1) and even n1: the planes are independent.  (5, 15): the rows of the plane group go
    through the paired row transform flattened, so plane 0's last row shares a transform with plane 1's first row and the column
    pass spreads that over the plane -- planes 0 and 1 are partners, plane 2 (its last row with zeros) has none.  Both directions."""
    from distributedfft_amd import api
    b = LI.PLANES
    paired = api.real_form(n2) != 1
    assert paired == (n2 == 15)
    coupled = paired and n1 % 2 == 1
    partners = lambda q: LI.partners_planes(q, b, n1, paired)   # noqa: E731
    assert [partners(q) for q in range(b)] == ([{1}, {0}, set()] if coupled else [set()] * 3)
    fam = "real" if coupled else None
    x, _ = A.real_planes(n1, n2, b, 4000 + n1)
    X, _ = A.half_planes(n1, n2, b, 5000 + n1)
    LI.check_case(lambda v: _host(api.rfft2d_batch(_gpu(v, prec, gpu))), _cached(("rfft2", n1, n2), lambda v: A.ld_fft(A.ld_rfft(v, 2), 1, +1)), x,
                  lambda q: (q,), LI.lines_planes, partners, prec, f"rfft2d_batch {n1}x{n2}", "rfft2", fam, n1 * n2, lines=[0, 1, 2])
    LI.check_case(lambda v: _host(api.irfft2d_batch(_gpu(v, prec, gpu), n2)),
                  _cached(("irfft2", n1, n2), lambda v: A.ld_irfft(A.ld_fft(v, 1, -1), n2, 2)), X, lambda q: (q,), LI.lines_planes, partners, prec,
                  f"irfft2d_batch {n1}x{n2}", "irfft2", fam, n1 * n2, lines=[0, 1, 2])


@pytest.mark.parametrize("prec", A.PRECS)
def test_rfft2d_batch_couples_planes_as_documented(gpu, prec):
    """(3, 5, 15), the coupling itself (include/dfft.h, dfft_rfft2d_batch): a NaN plane 0 reaches plane 1 through the one transform
    that plane 0's last row shares with plane 1's first row.  Forward the column pass then spreads it over ALL of plane 1; backward
    the rows come last, so only row 0 of plane 1 dies and its other rows are bit-identical.  Plane 1 reaches plane 0 the same way
    (its row 4), plane 2 -- whose last row goes with zeros -- reaches nobody and is reached by nobody."""
    from distributedfft_amd import api
    n1, n2 = 5, 15
    x, _ = A.real_planes(n1, n2, LI.PLANES, 4000 + n1)
    X, _ = A.half_planes(n1, n2, LI.PLANES, 5000 + n1)
    fwd = lambda v: _host(api.rfft2d_batch(_gpu(v, prec, gpu)))   # noqa: E731
    bwd = lambda v: _host(api.irfft2d_batch(_gpu(v, prec, gpu), n2))   # noqa: E731
    cf, cb = fwd(x), bwd(X)
    for plane, mate, row in ((0, 1, 0), (1, 0, n1 - 1)):
        gf, gb = fwd(LI.poison(x, (plane,), "nan")), bwd(LI.poison(X, (plane,), "nan"))
        assert not np.isfinite(gf[plane]).any() and not np.isfinite(gb[plane]).any()
        assert not np.isfinite(gf[mate]).any(), f"forward: plane {mate} is not NaN throughout although it shares a row transform with plane {plane}"
        assert not np.isfinite(gb[mate][row]).any(), f"backward: row {row} of plane {mate} shares its transform with a NaN row"
        rest = [r for r in range(n1) if r != row]
        assert LI.bits_equal(gb[mate][rest], cb[mate][rest]), f"backward: rows of plane {mate} other than row {row} changed"
        assert LI.bits_equal(gf[2], cf[2]) and LI.bits_equal(gb[2], cb[2])
    gf, gb = fwd(LI.poison(x, (2,), "nan")), bwd(LI.poison(X, (2,), "nan"))
    assert LI.bits_equal(gf[:2], cf[:2]) and LI.bits_equal(gb[:2], cb[:2])


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("route", ["fused", "composed"])
@pytest.mark.parametrize("kind", A.R2R_KINDS)
@pytest.mark.parametrize("n", LI.R2R_N)
def test_r2r(gpu, n, kind, route, prec):
    """rows of (5, n) (s = 1: rows 2p / 2p + 1) and columns of (2, n, s), on the one-launch route and under DFFT_R2R_FUSED=0"""
    from distributedfft_amd import api
    fam = LI.real_family(n, "r2r")
    with _composed("DFFT_R2R_FUSED", route == "composed"):
        x = A.r2r_lines(n, LI.BATCH, 1, 6000 + n)[0][:, :, 0]
        LI.check_case(lambda v: _host(api.r2r(_gpu(v, prec, gpu), kind, dim=-1)),
                      _cached(("r2r", n, kind), lambda v: A.ld_r2r(np.asarray(v).T[None], kind)[0].T), x, lambda q: (q,), LI.lines_rows,
                      lambda q: LI.partners_rows(q, LI.BATCH), prec, f"{kind} n={n} rows {route}", "r2r rows", fam, n)
        for s in LI.STRIDED_S:
            xs = A.r2r_lines(n, 2, s, 6000 + n)[0]
            LI.check_case(lambda v: _host(api.r2r(_gpu(v, prec, gpu), kind, dim=1)), _cached(("r2r", n, kind, s), lambda v: A.ld_r2r(v, kind)), xs,
                          lambda q: LI.cols_index(xs.shape, q), LI.lines_cols, lambda q: LI.partners_cols(q, 2, s), prec,
                          f"{kind} n={n} s={s} {route}", "r2r cols", fam, n)


# ---- the convolutions: rows are independent; a filter row reaches exactly its channel -------------------------------------------------------
def _filter(H, prec, gpu):
    return _gpu(H, prec, gpu)


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("hkind", RC.KINDS)
@pytest.mark.parametrize("route", ["fused", "composed"])
@pytest.mark.parametrize("M", [8, 25, 512])
def test_rconv1d(gpu, M, route, hkind, prec):
    """(2, 3, n) with n = m/2 and m/2 - 1; then filter row H[1] poisoned: exactly the rows of channel 1 are dirty"""
    from distributedfft_amd import api
    m, channels, batch = 2 * M, 3, 2
    with _composed("DFFT_RCONV_FUSED", route == "composed"):
        for n in (M, M - 1):
            x, H, _ = RC.case(M, n, channels, batch, hkind)
            Ht = _filter(H, prec, gpu)
            what = f"rconv1d M={M} n={n} {hkind} H {route}"
            run = lambda v, h=Ht: _host(api.rconv1d(_gpu(v, prec, gpu).reshape(batch, channels, n), h, m))   # noqa: E731
            LI.check_case(run, _cached(("rconv", M, n, hkind), lambda v: RC.reference(v, H, m)), x, lambda q: (q,), LI.lines_rows, LI.partners_none,
                          prec, what, "rconv1d")
            clean = LI.lines_rows(run(x))
            for kind in ("nan", "big"):
                Hp = LI.poison(H, (1,), kind)
                got = LI.lines_rows(run(x, _filter(Hp, prec, gpu)))
                with np.errstate(all="ignore"):
                    rp = RC.reference(x, Hp, m)
                rows1 = {r for r in range(batch * channels) if r % channels == 1}
                dirty = LI.dirty_set(rp, rows1)
                assert dirty == rows1
                LI.same_outside(clean, got, dirty, None, f"{what} H[1] {kind}")
                LI.dead_inside(got, LI.nonfinite(rp), f"{what} H[1] {kind}")
                if kind == "big":
                    for r in sorted(rows1):
                        assert LI.bits_equal(got[r], LI.scale_exact(clean[r], LI.BIG)), f"{what} H[1] big: row {r} is not 2^24 times the clean row"


def _os_taps_case(M, d, n, channels, batch, seed):
    """rows, `d + 1` taps per channel and their spectrum (longdouble, rounded by the caller)"""
    x = A.rand_real((batch * channels, n), seed)
    k = A.rand_real((channels, d + 1), seed + 1)
    return x, k, OC.taps_spectrum(k, 2 * M)


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("route", ["fused", "composed"])
@pytest.mark.parametrize("M,d", [(2, 2), (8, 6)])
def test_rconv1d_os(gpu, M, d, route, prec):
    """(2, 3, n) in blocks of m = 2 M with taps = d + 1 taps: whole rows poisoned, and ONE NaN at sample j in the middle of row 3 --
    y[j ... j + taps - 1] of that row must be NaN (the rest of the row is unspecified: a block transform may spread it), every other
    row is bit-identical"""
    from distributedfft_amd import api
    m, S, channels, batch, taps = 2 * M, 2 * M - d, 3, 2, d + 1
    n = 2 * S + S // 2 + 4 * m
    x, k, Hld = _os_taps_case(M, d, n, channels, batch, 8000 + M)
    H = Hld.astype(A.CDT[prec]).astype(np.complex128)       # the filter the library sees
    Ht = _gpu(H, prec, gpu)
    what = f"rconv1d_os M={M} d={d} n={n} {route}"
    run = lambda v: _host(api.rconv1d_os(_gpu(v, prec, gpu).reshape(batch, channels, n), Ht, m, d))   # noqa: E731
    with _composed("DFFT_RCONV_FUSED", route == "composed"):
        LI.check_case(run, _cached(("os", M, d, prec), lambda v: OC.reference(v, H, m, d, n)), x, lambda q: (q,), LI.lines_rows, LI.partners_none,
                      prec, what, "rconv1d_os")
        clean = LI.lines_rows(run(x))
        row, j = 3, n // 2
        got = LI.lines_rows(run(LI.poison(x, (row,), "nan1", sample=j)))
    must = np.zeros(got.shape, dtype=bool)
    must[row, j:min(j + taps, n)] = True
    LI.same_outside(clean, got, {row}, row, f"{what} nan1 at {j}")
    LI.dead_inside(got, must, f"{what} nan1 at {j}")


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("route", ["fused", "composed"])
@pytest.mark.parametrize("inplace", [False, True])
def test_rconv1d_long(gpu, inplace, route, prec):
    """m = rconv1d_long_length(8193), (2, 3, n), out of place and in place.  The three-launch route keeps rows apart.  The composed
    route (DFFT_RCONV_LONG_FUSED=0) runs "the real rows of length m as dfft_rfft1d runs them" -- real form 3 beyond 8192 points --, so
    there rows 2p and 2p + 1 of the batch * channels rows share their transforms, judged with nu_pair under the route's own bound
    (rconv1d_long_cases.BOUND: a row's own norm at equal scales, n_eff = m)."""
    import rconv1d_long_cases as LC
    from distributedfft_amd import _lib, api
    m, channels, batch = api.rconv1d_long_length(8193), 3, 2
    assert m == LI.long_length() and api.real_form(m) == 3
    code = 0 if prec == "f64" else 1
    n = m // 2 + 1
    x = A.rand_real((batch * channels, n), 9000)
    H = RC.make_filter(channels, m, "complex", 9001)
    Hp = api.rconv1d_long_filter(_gpu(H, prec, gpu))

    def run(v):
        t = _gpu(v, prec, gpu).reshape(batch, channels, n)
        return _host(api.rconv1d_long(t, Hp, m, out=t if inplace else None))
    what = f"rconv1d_long m={m} n={n} {'in place' if inplace else 'out of place'} {route}"
    with _composed("DFFT_RCONV_LONG_FUSED", route == "composed"):
        paired = not _lib.load().dfft_rconv1d_long_fused_applies(m, code)
        assert paired == (route == "composed"), "the default route of this length is the three-launch one in both precisions"
        LI.check_case(run, _cached(("long", m), lambda v: RC.reference(v, H, m)), x, lambda q: (q,), LI.lines_rows,
                      (lambda q: LI.partners_rows(q, batch * channels)) if paired else LI.partners_none, prec, what, f"rconv1d_long {route}",
                      LC.BOUND if paired else None, m)


# ---- STFT: the line is a (row, frame); inverse: a (row, sample) --------------------------------------------------------------------------
STFT_CASES = [(8, 4, 100), (512, 256, 3 * 1024 + 2)]   # (M, hop, n): n_fft = 16 with hop 4, and one tuned n_fft = 1024 with hop 256


def _stft_run(api, gpu, prec, n_fft, hop, win, center, okind):
    wt = _gpu(win, prec, gpu)
    return lambda v: _host(api.stft(_gpu(v, prec, gpu), n_fft, hop, window=wt, center=center, pad_mode="reflect", frames_last=False,
                                    power=2 if okind == "power" else None))


def _stft_ref(win, m, hop, center, okind):
    def ref(v):
        pad = m // 2 if center else 0
        X = SC.reference(v, win, m, hop, pad, SC.frames_of(v.shape[1], m, hop, pad), "reflect" if center else "zero")
        return SC.power(X) if okind == "power" else X
    return ref


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("okind", SC.KINDS)
@pytest.mark.parametrize("route", ["fused", "composed"])
@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("M,hop,n", STFT_CASES)
def test_stft(gpu, M, hop, n, center, route, okind, prec):
    """One NaN at a sample away from the ends of row 1: the frames whose support holds it die, every other frame of every row is
    bit-identical.  With center (reflect padding) once more at sample 1, where the frames that see its MIRROR image die too -- which
    frames, the reference says."""
    from distributedfft_amd import api
    m, rows = 2 * M, SC.ROWS
    x = A.rand_real((rows, n), 31000 + M)
    win = SC.window(m, "hann")
    assert win.min() > 0
    ref = _stft_ref(win, m, hop, center, okind)
    run = _stft_run(api, gpu, prec, m, hop, win, center, okind)
    pad = m // 2 if center else 0
    frames = SC.frames_of(n, m, hop, pad)
    lines = lambda y: LI.to_numpy(y).reshape(rows * frames, M + 1)   # noqa: E731
    with _composed("DFFT_STFT_FUSED", route == "composed"):
        clean = lines(run(x))
        for j in [n // 2 + 1] + ([1] if center else []):
            what = f"stft m={m} hop={hop} n={n} center={center} {okind} {route} NaN at sample {j} of row 1"
            xp = LI.poison(x, (1,), "nan1", sample=j)
            got = lines(run(xp))
            with np.errstate(all="ignore"):
                rp = lines(ref(xp))
            dirty = LI.dirty_set(rp, set())
            hold = {frames + f for f in range(frames) if f * hop - pad <= j < f * hop - pad + m}    # the frames whose support holds j
            assert hold <= dirty and all(frames <= q < 2 * frames for q in dirty), (hold, dirty)
            assert dirty == hold or (center and j == 1)                                           # only the mirror adds frames
            LI.same_outside(clean, got, dirty, min(hold), what)
            LI.dead_inside(got, LI.nonfinite(rp), what)


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("M,hop,frames", [(8, 4, 22), (512, 256, 9)])
def test_istft(gpu, M, hop, frames, center, prec):
    """One whole frame of row 1 NaN: the samples under that frame's support die, every other sample -- of the same row too -- is
    bit-identical"""
    from distributedfft_amd import api
    m, rows = 2 * M, SC.ROWS
    pad = m // 2 if center else 0
    X = A.rand_complex((rows, frames, M + 1), 33000 + M)
    win = SC.window(m, "hann")
    wt = _gpu(win, prec, gpu)
    run = lambda v: _host(api.istft(_gpu(v, prec, gpu), m, hop, window=wt, center=center, frames_last=False))   # noqa: E731
    clean = run(X)
    n = clean.shape[1]
    assert n == (frames - 1) * hop + m - 2 * pad
    for f in (0, frames // 2, frames - 1):
        what = f"istft m={m} hop={hop} frames={frames} center={center} frame {f} of row 1 NaN"
        got = run(LI.poison(X, (1, f), "nan"))
        t = np.arange(n)
        under = (t + pad >= f * hop) & (t + pad < f * hop + m)
        with np.errstate(all="ignore"):
            rp = SC.inverse_reference(LI.poison(X, (1, f), "nan"), win, np.ones(n), n, m, hop, pad)
        must = LI.nonfinite(rp)
        assert np.array_equal(must[1], under) and not must[[0, 2]].any()
        LI.same_outside(clean.reshape(-1, 1), got.reshape(-1, 1), {int(v) for v in np.nonzero(must.reshape(-1))[0]}, None, what)
        LI.dead_inside(got, must, what)


# ---- NaN in the input guards --------------------------------------------------------------------------------------------------------------
def _nan_guards(buf, view):
    """NaN in front of and behind the view: a read outside the input that reaches a result shows"""
    start = MC.view_start(buf, view)
    buf[:start] = float("nan")
    buf[start + view.numel():] = float("nan")


def _guard_identity(gpu, prec, inputs, call, what):
    """Every input in a guarded buffer one element past a 16-byte boundary; call(*tensors) with sentinel guards and with NaN guards:
    the same bytes"""
    import torch
    held = [_offset_tensor(np.asarray(a), prec, gpu, 1) for a in inputs]
    first = call(*[v for _, v in held]).clone()
    torch.cuda.synchronize()
    for buf, view in held:
        _nan_guards(buf, view.reshape(-1))
    second = call(*[v for _, v in held])
    torch.cuda.synchronize()
    assert MC.bits_equal(first, second), f"{what}: NaN in the input guards changed the result"


@pytest.mark.parametrize("prec", A.PRECS)
def test_nan_input_guards_complex(gpu, prec):
    from distributedfft_amd import api
    for n in (16, 360, 8192):
        _guard_identity(gpu, prec, [A.rand_complex((5, n), n)], lambda t: api.fft1d_rows(t, FWD), f"fft1d_rows n={n}")
        _guard_identity(gpu, prec, [A.rand_complex((2, n, 5), n)], lambda t: api.fft1d_cols(t, BWD), f"fft1d_cols n={n} w=5")
    for n in (11, 4099):
        _guard_identity(gpu, prec, [A.rand_complex((5, n), n)], lambda t: api.fft1d_any(t, -1, FWD), f"fft1d_any n={n}")
        _guard_identity(gpu, prec, [A.rand_complex((2, n, 3), n)], lambda t: api.fft1d_any(t, 1, BWD), f"fft1d_any n={n} s=3")
    for n1, n2 in [(7, 8), (8192, 8)] + ([(256, 256)] if prec == "f64" else []):
        _guard_identity(gpu, prec, [A.rand_complex((3, n1, n2), n1)], lambda t: api.fft2d_batch(t, FWD), f"fft2d_batch {n1}x{n2}")


@pytest.mark.parametrize("prec", A.PRECS)
def test_nan_input_guards_real(gpu, prec):
    from distributedfft_amd import api
    for n in LI.RFFT_ROWS_N:
        _guard_identity(gpu, prec, [A.rand_real((5, n), n)], lambda t: api.rfft1d(t), f"rfft1d n={n}")
        _guard_identity(gpu, prec, [A.rand_complex((5, n // 2 + 1), n)], lambda t: api.irfft1d(t, n), f"irfft1d n={n}")
    for n in LI.STRIDED_N:
        _guard_identity(gpu, prec, [A.rand_real((2, n, 5), n)], lambda t: api.rfft1d(t, dim=1), f"rfft1d dim=1 n={n} s=5")
        _guard_identity(gpu, prec, [A.rand_complex((2, n // 2 + 1, 5), n)], lambda t: api.irfft1d(t, n, dim=1), f"irfft1d dim=1 n={n} s=5")
    for n1, n2 in LI.RFFT_2D:
        _guard_identity(gpu, prec, [A.rand_real((3, n1, n2), n1)], lambda t: api.rfft2d_batch(t), f"rfft2d_batch {n1}x{n2}")
        _guard_identity(gpu, prec, [A.rand_complex((3, n1, n2 // 2 + 1), n1)], lambda t: api.irfft2d_batch(t, n2), f"irfft2d_batch {n1}x{n2}")
    for route in ("fused", "composed"):
        with _composed("DFFT_R2R_FUSED", route == "composed"):
            for n in LI.R2R_N:
                for kind in A.R2R_KINDS:
                    _guard_identity(gpu, prec, [A.rand_real((5, n), n)], lambda t: api.r2r(t, kind, dim=-1), f"{kind} n={n} rows {route}")
                    _guard_identity(gpu, prec, [A.rand_real((2, n, 5), n)], lambda t: api.r2r(t, kind, dim=1), f"{kind} n={n} s=5 {route}")


@pytest.mark.parametrize("prec", A.PRECS)
def test_nan_input_guards_convolutions_and_stft(gpu, prec):
    from distributedfft_amd import api
    for route in ("fused", "composed"):
        with _composed("DFFT_RCONV_FUSED", route == "composed"):
            for M in (8, 25, 512):
                for hkind in RC.KINDS:
                    x, H, _ = RC.case(M, M - 1, 3, 2, hkind)
                    _guard_identity(gpu, prec, [x.reshape(2, 3, M - 1), H], lambda t, h: api.rconv1d(t, h, 2 * M), f"rconv1d M={M} {hkind} {route}")
            for M, d in [(2, 2), (8, 6)]:
                m, S = 2 * M, 2 * M - d
                n = 2 * S + S // 2 + 4 * m
                x, _, Hld = _os_taps_case(M, d, n, 3, 2, 8000 + M)
                H = Hld.astype(np.complex64).astype(np.complex128)
                _guard_identity(gpu, prec, [x.reshape(2, 3, n), H], lambda t, h: api.rconv1d_os(t, h, m, d), f"rconv1d_os M={M} d={d} {route}")
    m = api.rconv1d_long_length(8193)
    Hp = api.rconv1d_long_filter(_gpu(RC.make_filter(3, m, "complex", 9001), prec, gpu))
    _guard_identity(gpu, prec, [A.rand_real((2, 3, m // 2 + 1), 9000)], lambda t: api.rconv1d_long(t, Hp, m), f"rconv1d_long m={m}")
    for route in ("fused", "composed"):
        with _composed("DFFT_STFT_FUSED", route == "composed"):
            for M, hop, n in STFT_CASES:
                win = SC.window(2 * M, "hann")
                for center in (True, False):
                    for okind in SC.KINDS:
                        _guard_identity(gpu, prec, [A.rand_real((3, n), M), win],
                                        lambda t, w: api.stft(t, 2 * M, hop, window=w, center=center, frames_last=False,
                                                              power=2 if okind == "power" else None).contiguous(),
                                        f"stft m={2 * M} center={center} {okind} {route}")
    for M, hop, frames in [(8, 4, 22), (512, 256, 9)]:
        win = SC.window(2 * M, "hann")
        for center in (True, False):
            _guard_identity(gpu, prec, [A.rand_complex((3, frames, M + 1), M), win],
                            lambda t, w: api.istft(t, 2 * M, hop, window=w, center=center, frames_last=False), f"istft m={2 * M} center={center}")
