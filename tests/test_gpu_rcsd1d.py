"""Framed (Welch) 1-D real cross-spectrum (dfft_rcsd1d, api.rcsd1d, api.csd / welch / coherence) on the GPU, against longdouble
references (numpy frames times the window, accuracy_ref.ld_rfft, conjugate-multiplied and summed over the frames;
tests/rcsd1d_cases.py): both precisions over the half-lengths of rcsd1d_cases.HALVES, one and three rows, one frame and several slices
with a ragged last slice and a ragged last workgroup, hops of m/2, m, an odd hop and 1, rows with and without samples behind the last
frame, the Hann and the rectangular window, one case whose workgroups loop; every fused case once more on the composed route
(DFFT_RCSD_FUSED=0) in one and in several chunks; the auto-spectrum; bit-identical repeats; every tuned length; which rows share
arithmetic; the buffer contract on guarded buffers; rows past 2^31 elements; the Python forms.

Error measure: accuracy_ref.nu per row over the m/2 + 1 bins with n_eff = m."""
import contextlib
import ctypes as C
import os
import re
from pathlib import Path

import numpy as np
import pytest

import accuracy_ref as A
import large_extent as LE
import line_isolation as LI
import mem_contract as MC
import rcsd1d_cases as WC
import tuned_sweep as TS

pytestmark = pytest.mark.gpu

# BOUND: 2 x the worst nu measured on an MI355X, rounded up to two digits; tests/test_rcsd1d_host.py holds it under 8 x the nu of the
# same-precision CPU pipeline on the same cases.  Every test here prints its nu.  Measured (fp64 / fp32, and the case):
#   worst                       1.494 / 2.490    M = 5, hop = 5, three rows of three frames, fused (the tuned sweep) / M = 2, hop = 2, three
#                                                rows of 17 frames, Hann, composed
#   worst of the other route    1.281 / 1.855    M = 2, hop = 3, three rows of 17 frames, rectangular, composed / M = 5, hop = 5, fused
#   fused against composed      1.714 / 1.513    M = 2, 17 frames, Hann
#   api.csd / api.welch         0.761 / 0.480 and below (M = 64 and 36, both scalings)
# The shortest frames set the bound: with m = 4 or 10 a line holds three or six bins, and the 17 (or 3) signed products of a bin cancel
# to a fraction of the sum of their moduli.  The same-precision CPU pipeline measures 1.281 / 2.522 on these cases, also at M = 2
# (tests/test_rcsd1d_host.py).
BOUND = {"f64": 3.0, "f32": 5.0}

ROOT = Path(__file__).resolve().parent.parent
INVENTORY = ROOT / "profiles" / "2026-10-20_rcsd1d" / "kernel_resources.txt"
CODE = {"f64": 0, "f32": 1}


def _rdt(prec):
    import torch
    return torch.float64 if prec == "f64" else torch.float32


def _cdt(prec):
    import torch
    return torch.complex128 if prec == "f64" else torch.complex64


def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


def _raw(x, g, out, win, n, m, hop, rows, prec, scale=1.0):
    lib = _lib()
    frames = 1 + (n - m) // hop
    rc = lib.dfft_rcsd1d(C.c_void_p(x), C.c_void_p(g), C.c_void_p(out), C.c_void_p(win), n, m, hop, frames, rows, scale, CODE[prec], None)
    return rc, lib.dfft_last_error().decode()


@contextlib.contextmanager
def _env(**kw):
    """environment variables for the calls inside (the library reads DFFT_RCSD_FUSED and DFFT_RCSD_CHUNK_BYTES per call)"""
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _composed(**kw):
    return _env(DFFT_RCSD_FUSED=0, **kw)


def _check(value, prec, what, factor=1.0):
    print(f"rcsd1d {prec} {what}: nu {value:.3f}")
    assert value <= factor * BOUND[prec], (prec, what, value, factor * BOUND[prec])


def _dev(a, prec, gpu):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(_rdt(prec)).to(gpu)


def _item_bytes(m, prec):
    cs = 16 if prec == "f64" else 8
    return m * cs // 2 + 2 * (m // 2 + 1) * cs


def _sweep_case(gpu, M, rows, frames, hop, tail, wname, prec):
    """One case: route rules, against the reference, bit-identical on a second call, inputs untouched, exact-zero imaginary parts at DC
    and Nyquist; the auto-spectrum; a fused case once more on the composed route -- within the bound, within twice the bound of the fused
    result, and bit-identical when the frames are cut into several chunks."""
    import torch
    from distributedfft_amd import api
    lib, m = _lib(), 2 * M
    fused, fused_auto = WC.fused(M, prec), WC.fused(M, prec, True)
    x, g, win, ref, auto = WC.case(M, rows, frames, hop, tail, wname)
    what = f"M={M} rows={rows} frames={frames} hop={hop} tail={tail} {wname}"
    xt, gt, wt = _dev(x, prec, gpu), _dev(g, prec, gpu), _dev(win, prec, gpu)
    assert lib.dfft_rcsd1d_fused_applies(m, CODE[prec], 0) == int(fused) and lib.dfft_rcsd1d_fused_applies(m, CODE[prec], 1) == int(fused_auto), what
    assert lib.dfft_rcsd1d_slices(m, rows, frames, CODE[prec]) == WC.slices_rule(M, rows, frames), what
    assert api.stft_frames(x.shape[1], m, hop, 0) == frames
    xk, gk, wk = xt.clone(), gt.clone(), wt.clone()
    got = api.rcsd1d(xt, gt, m, hop, wt)
    assert got.shape == (rows, M + 1) and got.dtype == _cdt(prec)
    assert torch.equal(xt, xk) and torch.equal(gt, gk) and torch.equal(wt, wk), "an input was written"
    assert MC.bits_equal(api.rcsd1d(xt, gt, m, hop, wt), got), ("a second call differs", what)
    s = got.cpu().numpy()
    assert np.all(s[:, 0].imag == 0) and np.all(s[:, M].imag == 0), what
    _check(WC.nu_lines(s, ref, m, prec), prec, what + (" fused" if fused else " composed"))
    at = api.rcsd1d(xt, xt, m, hop, wt)
    a = at.cpu().numpy()
    assert np.all(a.imag == 0) and np.all(a.real >= 0), what + " auto-spectrum"
    _check(WC.nu_lines(a, auto, m, prec), prec, what + " auto-spectrum" + (" fused" if fused_auto else " composed"))
    with _composed():
        assert lib.dfft_rcsd1d_fused_applies(m, CODE[prec], 0) == 0 == lib.dfft_rcsd1d_fused_applies(m, CODE[prec], 1)
        comp = api.rcsd1d(xt, gt, m, hop, wt)
        assert MC.bits_equal(api.rcsd1d(xt, gt, m, hop, wt), comp), ("composed: a second call differs", what)
        ca = api.rcsd1d(xt, xt, m, hop, wt)
    if frames > 1 and rows * frames <= 64:
        # chunks of five items: rows are cut inside, and a chunk holds the end of one row and the start of the next
        with _composed(DFFT_RCSD_CHUNK_BYTES=5 * _item_bytes(m, prec)):
            assert lib.dfft_rcsd1d_scratch_bytes(m, frames, rows, CODE[prec], 0) == 5 * _item_bytes(m, prec)
            assert lib.dfft_rcsd1d_scratch_bytes(m, frames, rows, CODE[prec], 1) == 5 * _item_bytes(m, prec)
            assert MC.bits_equal(api.rcsd1d(xt, gt, m, hop, wt), comp), ("composed: several chunks differ from one", what)
            assert MC.bits_equal(api.rcsd1d(xt, xt, m, hop, wt), ca), ("composed auto-spectrum: several chunks differ from one", what)
    if fused:
        c = comp.cpu().numpy()
        assert np.all(c[:, 0].imag == 0) and np.all(c[:, M].imag == 0), what
        _check(WC.nu_lines(c, ref, m, prec), prec, what + " composed")
        _check(WC.nu_lines(s, c.astype(A.CLD), m, prec), prec, what + " fused against composed", factor=2.0)
    else:
        assert MC.bits_equal(comp, got), what
    if fused_auto:
        cn = ca.cpu().numpy()
        assert np.all(cn.imag == 0) and np.all(cn.real >= 0), what
        _check(WC.nu_lines(cn, auto, m, prec), prec, what + " composed auto-spectrum")
        _check(WC.nu_lines(a, cn.astype(A.CLD), m, prec), prec, what + " auto-spectrum fused against composed", factor=2.0)
    else:
        assert MC.bits_equal(ca, at), what


# ---- the sweep --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("M", WC.HALVES)
def test_against_the_longdouble_reference(gpu, M, prec):
    for case in WC.cases_of(M):
        _sweep_case(gpu, *case, prec)


@pytest.mark.parametrize("prec", A.PRECS)
def test_more_rows_than_resident_thread_groups(gpu, prec):
    """M = 8 with more rows than a part holds thread groups: every workgroup loops over several item groups, the last one ragged"""
    M, rows, frames, hop, tail, wname = WC.BEYOND_TARGET
    assert WC.slices_rule(M, rows, frames) == 1
    _sweep_case(gpu, M, rows, frames, hop, tail, wname, prec)


def test_scale_argument(gpu):
    from distributedfft_amd import api
    for M, prec in ((64, "f64"), (64, "f32"), (36, "f64")):
        x, g, win, ref, _ = WC.case(M, 3, 17, M, 0, "hann")
        xt, gt, wt = _dev(x, prec, gpu), _dev(g, prec, gpu), _dev(win, prec, gpu)
        one = api.rcsd1d(xt, gt, 2 * M, M, wt)
        assert MC.bits_equal(api.rcsd1d(xt, gt, 2 * M, M, wt, scale=0.25), one * 0.25)      # a power of two: exact
        _check(WC.nu_lines(api.rcsd1d(xt, gt, 2 * M, M, wt, scale=1 / 3).cpu().numpy(), ref / 3, 2 * M, prec), prec, f"M={M} scale=1/3")


# ---- every tuned length -----------------------------------------------------------------------------------------------------------------
def _inventory_fused(kind):
    """(M, prec) whose `kind` ("auto" or "cross") kernel the inventory lists as built, in both access forms"""
    text = INVENTORY.read_text()
    seen = {(int(n), t, a) for t, n, a in re.findall(r"^rcsd_frames_kernel (f64|f32) M=(\d+) E=\d+ form=((?:vec|real)-(?:auto|cross)) ", text, re.M)}
    seen = {(n, t, a) for n, t, a in seen if a.endswith(kind)}
    assert all((n, t, "vec-" + kind) in seen and (n, t, "real-" + kind) in seen for n, t, _ in seen)
    return {(n, t) for n, t, _ in seen}


@pytest.mark.parametrize("M", [M for M in TS.plan_lengths() if M >= 2])
def test_every_tuned_length(gpu, M):
    """Every tuned half-length once per precision with two reals per access (n and hop even) and real by real (hop odd), three frames,
    three rows; the lengths the inventory does not list take the composed route."""
    from distributedfft_amd import api
    m, rows, frames = 2 * M, 3, 3
    built, built_auto = _inventory_fused("cross"), _inventory_fused("auto")
    for hop in ((M, M + 1) if M % 2 == 0 else (m, M)):      # even: n = 2 hop + m is even too; odd
        x, g, win, ref, auto = WC.case(M, rows, frames, hop, 0, "hann")
        for prec in A.PRECS:
            xt, gt, wt = _dev(x, prec, gpu), _dev(g, prec, gpu), _dev(win, prec, gpu)
            fused = (M, prec) in built
            assert _lib().dfft_rcsd1d_fused_applies(m, CODE[prec], 0) == int(fused) == int(WC.fused(M, prec)), (M, prec)
            assert _lib().dfft_rcsd1d_fused_applies(m, CODE[prec], 1) == int((M, prec) in built_auto) == int(WC.fused(M, prec, True)), (M, prec)
            got = api.rcsd1d(xt, gt, m, hop, wt)
            assert MC.bits_equal(api.rcsd1d(xt, gt, m, hop, wt), got)
            _check(WC.nu_lines(got.cpu().numpy(), ref, m, prec), prec, f"M={M} hop={hop} rows={rows} frames={frames}" + (" fused" if fused else " composed"))
            a = api.rcsd1d(xt, xt, m, hop, wt)
            assert MC.bits_equal(api.rcsd1d(xt, xt, m, hop, wt), a) and bool((a.imag == 0).all())
            _check(WC.nu_lines(a.cpu().numpy(), auto, m, prec), prec, f"M={M} hop={hop} rows={rows} frames={frames} auto-spectrum" +
                   (" fused" if (M, prec) in built_auto else " composed"))


# ---- which rows share arithmetic --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["fused", "composed"])
@pytest.mark.parametrize("prec", A.PRECS)
def test_a_row_reaches_its_own_line_and_no_other(gpu, prec, route):
    """One row of three poisoned in x, or in g -- all NaN, times 2^24, zero (line_isolation): the other rows stay bit-identical, the
    poisoned row is NaN where the reference is, exactly 2^24 times the clean line, or exactly zero.  A NaN behind the last whole frame
    changes nothing, and with hop = m + 3 neither does a NaN between two frames."""
    import torch
    from distributedfft_amd import api
    for M in (64, 25):
        m, rows = 2 * M, 3
        frames = WC.frame_counts(M, rows)[1]
        for hop, tail in ((M + 1, 3), (m + 3, 3)):
            x, g, win, _, _ = WC.case(M, rows, frames, hop, tail, "hann")
            wt = _dev(win, prec, gpu)
            with (_composed() if route == "composed" else contextlib.nullcontext()):
                assert _lib().dfft_rcsd1d_fused_applies(m, CODE[prec], 0) == int(route == "fused")
                for field in (0, 1):
                    other = _dev((g, x)[field], prec, gpu)

                    def run(v, field=field, other=other):
                        t = _dev(v, prec, gpu)
                        return api.rcsd1d(t, other, m, hop, wt) if field == 0 else api.rcsd1d(other, t, m, hop, wt)

                    def ref(v, key, field=field):
                        return WC.reference(v, g, win, m, hop) if field == 0 else WC.reference(x, v, win, m, hop)

                    src = (x, g)[field]
                    LI.check_case(run, ref, src, lambda line: LI.rows_index(src.shape, line), LI.lines_rows, LI.partners_none, prec,
                                  f"rcsd1d M={M} hop={hop} field {field} {route}", "rcsd1d", lines=(0, 1, 2))
                    clean = run(src)
                    n = src.shape[1]
                    spots = [n - 1, n - tail] + ([m, hop - 1, (frames - 2) * hop + m + 1] if hop > m else [])
                    for r in range(rows):
                        for j in spots:
                            v = np.array(src)
                            v[r, j] = np.nan
                            got = run(v)
                            assert MC.bits_equal(got, clean) and bool(torch.isfinite(got.real).all()), (M, hop, field, r, j, "a sample outside every frame is read")


# ---- the buffer contract ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["fused", "composed"])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("prec", A.PRECS)
def test_buffer_contract(gpu, prec, offset, route):
    """x, g, the window and out in guarded buffers, on a 16-byte boundary (two-real accesses) and one element past it (per-real accesses):
    nothing outside out is written, the fields and the window are untouched, and the result is right -- on the fused kernel with one slice
    and with several, on the composed route of the same length and on that of an untuned half-length.  An out that overlaps an input is
    refused."""
    import torch
    from distributedfft_amd import _lib as L
    lib = _lib()
    for M in (64, 36):
        m, rows, hop = 2 * M, 3, M
        for frames in WC.frame_counts(M, rows):
            x, g, win, ref, _ = WC.case(M, rows, frames, hop, 0, "hann")
            n = x.shape[1]
            xb, xv = MC.guarded(rows * n, _rdt(prec), gpu, offset, n)
            gb, gv = MC.guarded(rows * n, _rdt(prec), gpu, offset, n)
            wb, wv = MC.guarded(m, _rdt(prec), gpu, offset, m)
            ob, ov = MC.guarded(rows * (M + 1), _cdt(prec), gpu, offset, M + 1)
            xv.copy_(_dev(x, prec, gpu).reshape(-1))
            gv.copy_(_dev(g, prec, gpu).reshape(-1))
            wv.copy_(_dev(win, prec, gpu))
            xkeep, gkeep, wkeep = xb.clone(), gb.clone(), wb.clone()
            vec = int(xv.data_ptr() % (2 * xv.element_size()) == 0 and gv.data_ptr() % (2 * gv.element_size()) == 0)
            assert vec == int(offset == 0) and n % 2 == 0 and hop % 2 == 0
            what = f"M={M} n={n} frames={frames} offset={offset} {route}"
            with (_composed() if route == "composed" else contextlib.nullcontext()):
                assert lib.dfft_rcsd1d_fused_applies(m, CODE[prec], 0) == int(route == "fused" and M == 64)
                rc, msg = _raw(xv.data_ptr(), gv.data_ptr(), ov.data_ptr(), wv.data_ptr(), n, m, hop, rows, prec)
                assert rc == 0, msg
                torch.cuda.synchronize()
                MC.guards_intact(ob, ov, what + " out")
                assert MC.bits_equal(xb, xkeep) and MC.bits_equal(gb, gkeep) and MC.bits_equal(wb, wkeep), what + ": an input (or its guards) was written"
                _check(WC.nu_lines(ov.cpu().numpy().reshape(rows, M + 1), ref, m, prec), prec, what)
                # out inside x, inside g, reaching into either from in front, and over the window: refused, nothing written
                cs = ov.element_size()
                for bad in (xv.data_ptr(), gv.data_ptr() + (rows * n - 1) * xv.element_size(), xv.data_ptr() - rows * (M + 1) * cs + cs, wv.data_ptr()):
                    rc, msg = _raw(xv.data_ptr(), gv.data_ptr(), bad, wv.data_ptr(), n, m, hop, rows, prec)
                    assert rc == L.EINVAL and "overlaps" in msg, (what, rc, msg)
                torch.cuda.synchronize()
                assert MC.bits_equal(xb, xkeep) and MC.bits_equal(gb, gkeep) and MC.bits_equal(wb, wkeep)


# ---- rows past 2^31 elements ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
def test_large_extent(gpu, prec):
    """Three rows of 2^30 + 2^20 samples, frames of 128 that advance by 2^26: 17 frames per row, two slices, and the frames of the last
    row start past element 2^31 and byte 2^32 of either field.  Both fields are tiled from 61 base lines of 128 samples
    (large_extent.fill), so frame (r, f) is base line (r n + f hop) / 128 mod 61 and every row's reference is a sum of 17 of the 61
    one-tile products."""
    import torch
    from distributedfft_amd import api
    M, K, rows = 64, LE.K_DEFAULT, 3
    m, n, hop = 2 * M, (1 << 30) + (1 << 20), 1 << 26
    frames = 1 + (n - m) // hop
    eb = 8 if prec == "f64" else 4
    assert frames == 17 and WC.slices_rule(M, rows, frames) == 2 and n % m == 0 and hop % m == 0
    assert 2 * n + (frames - 1) * hop > 2 * n > 1 << 31 and 2 * n * eb > 1 << 32
    assert LE.wrap_distinct(rows * n // m, m, 1, K, eb)
    assert LE.peak_bytes(2 * rows * n * eb, 0, 0) <= LE.CAP_80
    bx, bg = A.rand_real((K, m), 71000), A.rand_real((K, m), 71001)
    win = WC.window("hann", m)
    prod = np.conj(A.ld_rfft(bx.astype(A.LD) * win, 1)) * A.ld_rfft(bg.astype(A.LD) * win, 1)           # [K][M + 1]
    cls = np.array([[((r * n + f * hop) // m) % K for f in range(frames)] for r in range(rows)])
    assert len({tuple(c) for c in cls}) == rows, "the rows hold different frames"
    ref = prod[cls].sum(axis=1)
    bxT, bgT = LE.base_tensor(bx, prec, gpu), LE.base_tensor(bg, prec, gpu)
    xt = torch.empty((rows * n // m, m, 1), dtype=_rdt(prec), device=gpu)
    gt = torch.empty((rows * n // m, m, 1), dtype=_rdt(prec), device=gpu)
    LE.fill(xt, bxT, K)
    LE.fill(gt, bgT, K)
    try:
        got = api.rcsd1d(xt.view(rows, n), gt.view(rows, n), m, hop, _dev(win, prec, gpu))
        assert LE.input_intact(xt, bxT, K) is None and LE.input_intact(gt, bgT, K) is None
        for r in range(rows):
            _check(WC.nu_lines(got[r:r + 1].cpu().numpy(), ref[r:r + 1], m, prec), prec, f"large extent row {r} (first sample {r * n})")
    finally:
        del xt, gt
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


# ---- the Python forms -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
def test_csd_welch_and_coherence(gpu, prec):
    """api.csd / api.welch against the reference with the normalisation applied, both scalings; api.coherence against the formula on the
    references; the defaults hop_length = n_fft // 2 and window = periodic Hann; a window shorter than the frame; leading dimensions."""
    import torch
    from distributedfft_amd import api
    fs = 48000.0
    for M in (64, 36):
        m, rows, frames = 2 * M, 6, 17
        x, g, _, _, _ = WC.case(M, rows, frames, M, 3, "hann")
        hann = torch.hann_window(m, periodic=True, dtype=torch.float64).to(_rdt(prec)).double().numpy()     # the default, as the library sees it
        xt, gt = _dev(x, prec, gpu).reshape(2, 3, -1), _dev(g, prec, gpu).reshape(2, 3, -1)
        dbl = np.full(M + 1, 2.0)
        dbl[0] = dbl[M] = 1.0
        wl = m - 16
        short = np.zeros(m)
        short[8:8 + wl] = WC.window("hann", wl)
        for name, win, kw in (("defaults", hann, {}),
                              ("hop m, rectangular", np.ones(m), dict(hop_length=m, window=torch.ones(m, device=gpu))),
                              ("win_length", short, dict(hop_length=M + 1, window=_dev(WC.window("hann", wl), prec, gpu), win_length=wl))):
            hop = kw.get("hop_length", M)
            nf = 1 + (x.shape[1] - m) // hop
            pxy, pxx, pyy = WC.reference(x, g, win, m, hop), WC.reference(x, x, win, m, hop), WC.reference(g, g, win, m, hop)
            for scaling, norm in (("density", 1 / (fs * (win.astype(A.LD) ** 2).sum())), ("spectrum", 1 / win.astype(A.LD).sum() ** 2)):
                what = f"M={M} {name} {scaling}"
                c = api.csd(xt, gt, m, fs=fs, scaling=scaling, **kw)
                w = api.welch(xt, m, fs=fs, scaling=scaling, **kw)
                assert c.shape == w.shape == (2, 3, M + 1) and c.dtype == _cdt(prec) and w.dtype == _rdt(prec)
                _check(WC.nu_lines(c.reshape(rows, -1).cpu().numpy(), pxy * dbl * norm / nf, m, prec), prec, what + " csd")
                _check(WC.nu_lines(w.reshape(rows, -1).cpu().numpy(), pxx.real * dbl * norm / nf, m, prec), prec, what + " welch")
                assert bool((w >= 0).all())
            coh = api.coherence(xt, gt, m, **kw).reshape(rows, -1).cpu().numpy()
            want = (np.abs(pxy) ** 2 / (pxx.real * pyy.real))
            # Three results within BOUND eps sqrt(log2 m) ||line|| of their lines enter a quotient.  A bin of such a result is off by at
            # most that much, relative to itself by unit ||line|| / |bin|; to first order the quotient |Pxy|^2 / (Pxx Pyy) is then off,
            # relative to itself, by twice that of Pxy plus those of Pxx and Pyy, and by 4 eps for the square, the product and the quotient.
            unit = BOUND[prec] * A.EPS[prec] * np.sqrt(np.log2(m))
            rel = lambda p: np.sqrt((np.abs(p) ** 2).sum(1, keepdims=True)) / np.abs(p)   # noqa: E731
            tol = (want * (unit * (2 * rel(pxy) + rel(pxx) + rel(pyy)) + 4 * A.EPS[prec])).astype(np.float64)
            err = np.abs(coh - want).astype(np.float64)
            print(f"rcsd1d {prec} M={M} {name} coherence: worst error / tolerance {np.max(err / tol):.3f}")
            assert np.all(err <= tol) and coh.dtype == A.RDT[prec] and np.all(coh >= 0) and np.all(coh <= 1 + 1e-4)
        # one frame: conj(X) Y is off by at most 2 eps |X| |Y| in either part (two products and a sum each), |.|^2 of it by 8 eps of
        # itself with its own square and sum; |X|^2 and |Y|^2 by 2 eps each, their product and the quotient by one more each: 14 eps
        one = api.coherence(xt[..., :m].contiguous(), gt[..., :m].contiguous(), m).cpu().numpy()
        print(f"rcsd1d {prec} M={M} one-frame coherence: worst |c - 1| / eps {np.abs(one - 1).max() / A.EPS[prec]:.2f}")
        assert np.abs(one - 1).max() <= 16 * A.EPS[prec]
        with pytest.raises(ValueError):
            api.welch(xt[..., :m - 1].contiguous(), m)
