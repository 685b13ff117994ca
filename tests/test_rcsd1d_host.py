"""Framed (Welch) 1-D real cross-spectrum (dfft_rcsd1d), host side (no GPU): the four symbols, the refusals that are decided before the
device is queried, the slice, route and scratch rules against their restatement in tests/rcsd1d_cases.py, the committed resource
inventory of the fused kernels, the normalisation of api.csd / api.welch / api.coherence on a numpy model of api.rcsd1d, and the CPU
yardstick that the GPU bound of tests/test_gpu_rcsd1d.py is held against."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import accuracy_ref as A
import fused_inventory as FI
import rconv1d_cases as RC
import rcsd1d_cases as WC

try:
    import scipy.fft as sf
except ImportError:   # pragma: no cover
    sf = None

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "distributedfft_amd" / "csrc"
INVENTORY = ROOT / "profiles" / "2026-10-20_rcsd1d" / "kernel_resources.txt"
SYMBOLS = ("dfft_rcsd1d", "dfft_rcsd1d_fused_applies", "dfft_rcsd1d_scratch_bytes", "dfft_rcsd1d_slices")
X, G, OUT, WIN = 0x10000000, 0x20000000, 0x30000000, 0x40000000
F64, F32 = 0, 1
CODE = {"f64": F64, "f32": F32}


def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


def _call(x=X, g=G, out=OUT, win=WIN, n=1000, m=128, hop=64, frames=None, rows=3, scale=1.0, dtype=F64):
    lib = _lib()
    vp = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    if frames is None:
        frames = 1 + (n - m) // hop if hop >= 1 and n >= m >= 1 else 1
    rc = lib.dfft_rcsd1d(vp(x), vp(g), vp(out), vp(win), n, m, hop, frames, rows, scale, dtype, None)
    return rc, lib.dfft_last_error().decode()


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_signatures_agree_on_the_symbols():
    from distributedfft_amd import _lib as L
    header = (ROOT / "include" / "dfft.h").read_text()
    lib = _lib()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES, name
        assert getattr(lib, name) is not None
    for path in (L.LIB_PATH, L.LIB_PATH_SYSTEM):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
        assert set(SYMBOLS) <= set(re.findall(r" T (dfft_[a-z0-9_]+)", out)), path
    assert L.SIGNATURES["dfft_rcsd1d"] == (C.c_int, [C.c_void_p] * 4 + [C.c_longlong] * 5 + [C.c_double, C.c_int, C.c_void_p])
    assert L.SIGNATURES["dfft_rcsd1d_fused_applies"] == (C.c_int, [C.c_longlong, C.c_int, C.c_int])
    assert L.SIGNATURES["dfft_rcsd1d_scratch_bytes"] == (C.c_ulonglong, [C.c_longlong] * 3 + [C.c_int] * 2)
    assert L.SIGNATURES["dfft_rcsd1d_slices"] == (C.c_longlong, [C.c_longlong] * 3 + [C.c_int])
    assert "DFFT_RCSD_FUSED" in header and "DFFT_RCSD_CHUNK_BYTES" in header


def test_the_not_built_notes_about_a_welch_form_are_gone():
    for path in ("README.md", "DESIGN.md", "include/dfft.h", "distributedfft_amd/api.py"):
        text = " ".join((ROOT / path).read_text().split())
        assert not re.search(r"[Aa] windowed \(Welch\) form[^.]*(not|NOT) built", text), path


def test_refusals_are_decided_before_the_device_is_queried():
    from distributedfft_amd import _lib as L
    for dtype in (F64, F32):
        kw = dict(dtype=dtype)
        for p in ("x", "g", "out", "win"):                           # NULL pointers
            assert _call(**{p: 0}, **kw)[0] == L.EINVAL, p
        for bad in (0, -3):                                           # sizes below 1
            assert _call(n=bad, **kw)[0] == L.EINVAL
            assert _call(m=bad, **kw)[0] == L.EINVAL
            assert _call(hop=bad, **kw)[0] == L.EINVAL
            assert _call(rows=bad, **kw)[0] == L.EINVAL
            assert _call(frames=bad, **kw)[0] == L.EINVAL
        assert _call(n=127, m=128, frames=1, **kw)[0] == L.EINVAL    # a row shorter than one frame
        assert _call(n=100, m=194, frames=1, **kw)[0] == L.EINVAL    # ... before m is judged
        for frames in (13, 15, 1):                                    # 1 + (1000 - 128) / 64 = 14 frames, no other count
            assert _call(frames=frames, **kw)[0] == L.EINVAL
        assert _call(n=128 + 5 * 200, hop=200, frames=7, **kw)[0] == L.EINVAL      # hop > m: 6 frames
        rs = 8 if dtype == F64 else 4
        data, ob, wb = 1000 * 3 * rs, 3 * 65 * 2 * rs, 128 * rs
        for field in (X, G):                                          # out overlaps x or g, either end
            assert _call(out=field, **kw)[0] == L.EINVAL
            assert _call(out=field + data - rs, **kw)[0] == L.EINVAL
            assert _call(out=field - ob + rs, **kw)[0] == L.EINVAL
        assert _call(g=X, out=X + rs, **kw)[0] == L.EINVAL            # ... also for the auto-spectrum
        for bad in (OUT, OUT + ob - rs, OUT - wb + rs):               # the window overlaps out
            rc, msg = _call(win=bad, **kw)
            assert rc == L.EINVAL and "window" in msg, (rc, msg)
        for m in (9, 194, 22, 2, 8194, 16384, 2 * 4099, 1 << 30):    # odd, Bluestein half, 11 | m/2, m/2 = 1, above 8192
            rc, msg = _call(n=1 << 31, m=m, hop=m, **kw)
            assert rc == L.EUNSUPPORTED and f"m = {m}" in msg, (m, rc, msg)
            assert _lib().dfft_real_form(m) != 1
    for dtype in (-1, 2, 7):
        assert _call(dtype=dtype)[0] == L.EINVAL
    rc, msg = _call(n=4, m=4, hop=1, rows=1 << 31)                    # 2^31 items or more
    assert rc == L.EUNSUPPORTED and "split the rows" in msg, (rc, msg)
    assert _call(n=4, m=4, hop=1, rows=1 << 40)[0] == L.EUNSUPPORTED
    rc, msg = _call(n=(1 << 31) + 3, m=4, hop=1, rows=1)              # 2^31 frames
    assert rc == L.EUNSUPPORTED and "frames" in msg and "split" in msg, (rc, msg)
    assert _call(n=(1 << 33) + 4, m=4, hop=2, rows=1)[0] == L.EUNSUPPORTED


def test_valid_calls_reach_the_device_query():
    from distributedfft_amd import _lib as L
    if _lib().dfft_device_count() > 0:
        return
    for M in WC.HALVES + [3125, 1536, 1280]:
        for hop in WC.hops(M):
            for dtype in (F64, F32):
                n = 16 * hop + 2 * M + 1
                assert _call(n=n, m=2 * M, hop=hop, dtype=dtype, out=1 << 44, win=1 << 45)[0] == L.ENOGPU, (M, hop)
                assert _call(g=X, n=n, m=2 * M, hop=hop, dtype=dtype, out=1 << 44, win=1 << 45)[0] == L.ENOGPU     # g is x: the auto-spectrum
    # ranges that merely touch do not overlap: 3 rows of 1000 doubles = 24000 bytes; 3 x 65 complex doubles = 3120 bytes
    assert _call(out=X + 24000)[0] == L.ENOGPU
    assert _call(out=G - 3120)[0] == L.ENOGPU
    assert _call(win=OUT + 3120)[0] == L.ENOGPU
    assert _call(win=OUT - 1024)[0] == L.ENOGPU
    assert _call(g=X + 8, win=X + 16)[0] == L.ENOGPU                 # x, g and the window may overlap: none is written
    assert _call(n=4, m=4, hop=1, rows=(1 << 31) - 1, out=1 << 44)[0] == L.ENOGPU
    assert _call(n=(1 << 31) + 2, m=4, hop=1, rows=1, out=1 << 44)[0] == L.ENOGPU   # 2^31 - 1 frames
    assert _call(n=128 + 5 * 200 + 199, hop=200, frames=6)[0] == L.ENOGPU           # hop > m


# ---- slices, route, scratch -------------------------------------------------------------------------------------------------------------
def test_slices_match_the_rule_and_cover_the_frames_once():
    """slices = max(1, min(target / rows, frames / 8)), target = 512 * min(G, 32) with G the thread groups per workgroup of the m/2-point
    kernel (1 for an untuned m/2) -- whatever the precision and the environment; the ranges are contiguous and cover the frames."""
    lib = _lib()
    for M in sorted(set(RC.plan_points()) | {36, 6, 18, 3600}):
        target = 512 * min(RC.rows_per_group(M), 32)
        for rows in (1, 2, 3, 16, 511, 512, 513, 4096, 5000, 16384, 16385, (1 << 31) - 1):
            for frames in (1, 7, 8, 15, 16, 17, 100, 4096, 32775, 1 << 20, (1 << 31) - 1):
                want = 1
                for s in range(1, target + 1):       # brute force: the most slices with s * rows <= target and 8 s <= frames
                    if s * rows > target or WC.MIN_FRAMES * s > frames:
                        break
                    want = s
                for dtype in (F64, F32):
                    got = lib.dfft_rcsd1d_slices(2 * M, rows, frames, dtype)
                    assert got == want == WC.slices_rule(M, rows, frames), (M, rows, frames, got, want)
                assert rows * want < 1 << 31
                if frames <= 1 << 20:
                    ranges = WC.slice_ranges(frames, want)
                    assert ranges[0][0] == 0 and sum(r for _, r in ranges) == frames
                    assert all(a + r == b for (a, r), (b, _) in zip(ranges, ranges[1:]))
                    assert max(r for _, r in ranges) - min(r for _, r in ranges) <= 1 and (want == 1 or ranges[-1][1] >= WC.MIN_FRAMES)
    for args in ((22, 1, 1, F64), (9, 1, 1, F64), (8194, 1, 1, F64), (128, 0, 1, F64), (128, 1, 0, F64), (128, 1, 1, 5), (4, 1 << 31, 1, F64),
                 (4, 1, 1 << 31, F64)):
        assert lib.dfft_rcsd1d_slices(*args) == 0, args
    # the frame counts of the sweep do what they are chosen for, and every case of the table agrees with the library
    for M in sorted(set(WC.HALVES) | set(RC.plan_points())):
        G = RC.rows_per_group(M)
        for rows in WC.ROWS:
            one, many = WC.frame_counts(M, rows)
            s = WC.slices_rule(M, rows, many)
            assert one == 1 and WC.slices_rule(M, rows, 1) == 1 and s >= 2 and many % s and many < 64
            assert G == 1 or rows % G == 0 or (rows * s) % G, (M, rows)
            assert many == 17 or (rows * 2) % G == 0, "17 frames wherever two slices leave a ragged workgroup"
            assert M not in WC.HALVES or G == 1 or (rows * s) % G, "the sweep's own cases do leave a ragged workgroup"
    for M, rows, frames, hop, tail, wname in WC.all_cases():
        for prec, dtype in CODE.items():
            assert lib.dfft_rcsd1d_slices(2 * M, rows, frames, dtype) == WC.slices_rule(M, rows, frames)
            for autos in (0, 1):
                assert lib.dfft_rcsd1d_fused_applies(2 * M, dtype, autos) == int(WC.fused(M, prec, autos))
    M, rows, frames, hop, tail, wname = WC.BEYOND_TARGET
    assert WC.slices_rule(M, rows, frames) == 1 and RC.rows_per_group(M) == 256 and rows > 256 * 8 * 256 and rows % 256


def test_route_and_scratch_rules(monkeypatch):
    """Fused: m/2 tuned and not in the routed list; 0 under DFFT_RCSD_FUSED=0 (read per call).  Scratch: the partial sums of the slices
    (0 for one slice) on the fused route, else chunk items x (m reals + 2 (m/2 + 1) complex) within max(cap, one item's), cap = 256 MiB
    or DFFT_RCSD_CHUNK_BYTES."""
    lib = _lib()
    monkeypatch.delenv("DFFT_RCSD_FUSED", raising=False)
    monkeypatch.delenv("DFFT_RCSD_CHUNK_BYTES", raising=False)
    monkeypatch.delenv("DFFT_SCRATCH_CHUNK_BYTES", raising=False)
    tuned = set(RC.plan_points())

    def lease(m, items, dtype, cap=256 << 20):
        cs = 16 if dtype == F64 else 8
        ib = m * cs // 2 + 2 * (m // 2 + 1) * cs
        return min(items, max(cap, ib) // ib) * ib

    for M in sorted(tuned | {36, 6, 18, 3600}):
        m = 2 * M
        for prec, dtype in CODE.items():
          for autos in (0, 1):
            fused = WC.fused(M, prec, autos)
            assert fused == (M in tuned and (M, prec) not in (WC.ROUTED_AUTO if autos else WC.ROUTED))
            assert lib.dfft_rcsd1d_fused_applies(m, dtype, autos) == int(fused), (M, prec, autos)
            for rows, frames in ((1, 1), (3, 5), (3, 19), (16, 4096), (4096, 63)):
                got = lib.dfft_rcsd1d_scratch_bytes(m, frames, rows, dtype, autos)
                s = WC.slices_rule(M, rows, frames)
                want = (s * rows * (M + 1) * (16 if dtype == F64 else 8) if s > 1 else 0) if fused else lease(m, rows * frames, dtype)
                assert got == want, (M, prec, autos, rows, frames, got, want)
    assert lib.dfft_rcsd1d_fused_applies(128, 5, 0) == 0
    assert lib.dfft_rcsd1d_fused_applies(22, F64, 1) == 0
    assert lib.dfft_rcsd1d_scratch_bytes(22, 1, 1, F64, 0) == 0
    assert lib.dfft_rcsd1d_scratch_bytes(128, 0, 1, F64, 0) == 0
    assert lib.dfft_rcsd1d_scratch_bytes(4, 1, 1 << 31, F64, 1) == 0
    monkeypatch.setenv("DFFT_RCSD_FUSED", "0")
    assert lib.dfft_rcsd1d_fused_applies(128, F64, 0) == 0 == lib.dfft_rcsd1d_fused_applies(128, F64, 1)
    assert lib.dfft_rcsd1d_scratch_bytes(128, 5, 3, F32, 0) == 15 * (128 * 4 + 2 * 65 * 8) == lib.dfft_rcsd1d_scratch_bytes(128, 5, 3, F32, 1)
    monkeypatch.setenv("DFFT_RCSD_CHUNK_BYTES", "5000")              # three items of 1552 bytes
    assert lib.dfft_rcsd1d_scratch_bytes(128, 5, 3, F32, 0) == lease(128, 15, F32, 5000) == 3 * 1552
    monkeypatch.setenv("DFFT_RCSD_CHUNK_BYTES", "1")                 # never less than one item
    assert lib.dfft_rcsd1d_scratch_bytes(128, 5, 3, F32, 1) == 1552
    assert lib.dfft_rcsd1d_slices(128, 3, 19, F64) == 2              # the slice count does not depend on the route
    monkeypatch.setenv("DFFT_RCSD_FUSED", "1")
    assert lib.dfft_rcsd1d_fused_applies(128, F64, 0) == 1 == lib.dfft_rcsd1d_fused_applies(128, F64, 1)


# ---- build ------------------------------------------------------------------------------------------------------------------------------
def test_units_of_the_build():
    from distributedfft_amd import build
    from distributedfft_amd.build import NUM_INST_GROUPS
    names = [u[1].name for u in build.units()]
    assert [f"dfft_csd_{g}.o" for g in range(NUM_INST_GROUPS + 1)] == [n for n in names if n.startswith("dfft_csd_") and n != "dfft_csd_api.o"]
    assert "dfft_csd_api.o" in names


# ---- resource inventory -----------------------------------------------------------------------------------------------------------------
def test_inventory_belongs_to_the_sources_and_no_fused_kernel_spills():
    """profiles/2026-10-20_rcsd1d/kernel_resources.txt (tools/fused_resources.py rcsd) must carry the sha256 of the sources in the tree and
    list every fused instantiation -- tuned M x fp64 / fp32 x two-real / per-real accesses x auto / cross kernel, less the ones
    rcsd_fused_ok sends to the composed route, which it names -- with zero scratch; dfft_rcsd1d_fused_applies agrees with it."""
    text = FI.current_text("rcsd")
    fused = [ln for ln in text.splitlines() if ln.startswith("rcsd_frames_kernel ")]
    m = re.search(r"^# composed-route \(M, type, form\): (.*)$", text, re.M)
    assert m, "the inventory names the instantiations rcsd_fused_ok sends to the composed route"
    routed = {(int(n), t, a) for n, t, a in re.findall(r"\((\d+), (f64|f32), ((?:vec|real)-(?:auto|cross))\)", m.group(1))}
    forms = ("vec-auto", "vec-cross", "real-auto", "real-cross")
    assert {(n, t) for n, t, a in routed if a.endswith("cross")} == WC.ROUTED
    assert {(n, t) for n, t, a in routed if a.endswith("auto")} == WC.ROUTED_AUTO <= WC.ROUTED
    assert len(routed) == 2 * (len(WC.ROUTED) + len(WC.ROUTED_AUTO))
    tuned = sorted(RC.plan_points())
    want = {(n, t, a) for n in tuned for t in ("f64", "f32") for a in forms} - routed
    seen = set()
    for ln in fused:
        g = re.match(r"rcsd_frames_kernel (f64|f32) M=(\d+) E=\d+ form=((?:vec|real)-(?:auto|cross)) ", ln)
        assert g, ln
        seen.add((int(g.group(2)), g.group(1), g.group(3)))
    assert seen == want and len(fused) == len(want)
    # the gather and accumulating kernels of the unit, and the reduction kernel of the common unit
    helpers = [ln for ln in text.splitlines() if ln.startswith(("rcsd_gather_", "rcsd_mac_"))] + FI.common_lines("slice_reduce_")
    assert len(helpers) == 6
    for ln in fused + helpers:
        assert re.search(r"scratch=(\d+)", ln).group(1) == "0", ln
    src = (CSRC / "dfft_csd.hip").read_text()
    body = re.search(r"constexpr bool rcsd_fused_ok\(int M, bool f64, bool autos\) \{(.*?)\n\}", src, re.S).group(1)
    lib = _lib()
    for n, t, _ in routed:
        assert re.search(rf"\b{n}\b", body), n
    for n in tuned:
        for t in ("f64", "f32"):
            for autos, form in ((0, "vec-cross"), (1, "vec-auto")):
                assert lib.dfft_rcsd1d_fused_applies(2 * n, CODE[t], autos) == int((n, t, form) in seen), (n, t, form)


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
def test_reference_is_numpy_rfft_of_the_windowed_frames():
    for M, rows, frames, hop, tail, wname in ((8, 3, 17, 9, 3, "hann"), (25, 1, 17, 50, 0, "rect"), (36, 3, 17, 36, 3, "hann"), (8, 3, 5, 40, 3, "hann")):
        x, g, win, ref, auto = WC.case(M, rows, frames, hop, tail, wname)
        m = 2 * M
        assert x.shape == (rows, (frames - 1) * hop + m + tail)
        want = np.zeros((rows, M + 1), dtype=complex)
        wauto = np.zeros((rows, M + 1))
        for f in range(frames):
            Xf, Gf = np.fft.rfft(x[:, f * hop:f * hop + m] * win), np.fft.rfft(g[:, f * hop:f * hop + m] * win)
            want += np.conj(Xf) * Gf
            wauto += np.abs(Xf) ** 2
        assert np.abs(ref.astype(np.complex128) - want).max() <= 1e-12 * np.abs(want).max()
        assert np.abs(auto.astype(np.complex128) - wauto).max() <= 1e-12 * wauto.max()
        assert _lib().dfft_stft1d_frames(x.shape[1], m, hop, 0) == frames
    assert np.all(WC.window("hann", 8) == np.float32(0.5) - np.float32(0.5) * np.cos(2 * np.pi * np.arange(8) / 8).astype(np.float32))


# ---- the Python forms on a numpy model of rcsd1d ----------------------------------------------------------------------------------------
def _rcsd1d_model(x, g, n_fft, hop_length, window=None, scale=1.0, out=None, win_length=None):
    """api.rcsd1d on CPU tensors: the window through api._stft_window, frames and transforms by numpy"""
    import torch
    from distributedfft_amd import api
    w = api._stft_window(window, n_fft, win_length, x.dtype, x.device).numpy()
    lead = tuple(x.shape[:-1])
    P = WC.reference(x.reshape(-1, x.shape[-1]).numpy(), x.reshape(-1, x.shape[-1]).numpy() if g is x else g.reshape(-1, g.shape[-1]).numpy(),
                     w, n_fft, hop_length) * scale
    return torch.from_numpy(P.astype(np.complex128)).reshape(lead + (n_fft // 2 + 1,))


def test_normalisation_of_csd_welch_and_coherence(monkeypatch):
    """On white noise of unit variance the one-sided density is 2 / fs off the end bins (1 / fs at bins 0 and n_fft / 2) and the
    "spectrum" scaling differs from it by fs sum w^2 / (sum w)^2; csd of x with itself is welch; one frame gives coherence 1; the
    defaults are hop_length = n_fft // 2 and the periodic Hann window; win_length pads the window."""
    import torch
    from distributedfft_amd import api
    monkeypatch.setattr(api, "rcsd1d", _rcsd1d_model)
    n_fft, fs = 64, 250.0
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 40000, dtype=torch.float64, generator=gen)
    y = torch.randn(2, 3, 40000, dtype=torch.float64, generator=gen)
    hann = torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
    P = api.welch(x, n_fft, fs=fs)
    assert P.shape == (2, 3, n_fft // 2 + 1) and P.dtype == torch.float64 and not P.is_complex()
    frames = 1 + (40000 - n_fft) // (n_fft // 2)
    # a mean of `frames` chi-square variables, overlapping by half: a few per cent at 1249 frames
    assert ((P[..., 1:-1] * fs / 2 - 1).abs().max() < 0.2) and ((P[..., 1:-1] * fs / 2).mean() - 1).abs() < 0.01
    assert (P[..., 0] * fs).mean() < 1.5 and (P[..., -1] * fs).mean() < 1.5
    X = torch.stft(x.reshape(-1, 40000), n_fft, n_fft // 2, window=hann, center=False, return_complex=True).reshape(2, 3, n_fft // 2 + 1, frames)
    Y = torch.stft(y.reshape(-1, 40000), n_fft, n_fft // 2, window=hann, center=False, return_complex=True).reshape(2, 3, n_fft // 2 + 1, frames)
    dbl = torch.full((n_fft // 2 + 1,), 2.0, dtype=torch.float64)
    dbl[0] = dbl[-1] = 1.0
    want = (X.abs() ** 2).mean(-1) * dbl / (fs * (hann ** 2).sum())
    assert (P - want).abs().max() <= 1e-12 * want.max()
    S = api.welch(x, n_fft, fs=fs, scaling="spectrum")
    assert (S - want * fs * (hann ** 2).sum() / hann.sum() ** 2).abs().max() <= 1e-12 * S.max()
    Pxy = api.csd(x, y, n_fft, fs=fs)
    wxy = (X.conj() * Y).mean(-1) * dbl / (fs * (hann ** 2).sum())
    assert Pxy.is_complex() and (Pxy - wxy).abs().max() <= 1e-12 * wxy.abs().max()
    assert (api.csd(x, x, n_fft, fs=fs).real - P).abs().max() <= 1e-12 * P.max()
    coh = api.coherence(x, y, n_fft)
    wcoh = wxy.abs() ** 2 / (want * (Y.abs() ** 2).mean(-1) * dbl / (fs * (hann ** 2).sum()))
    assert (coh - wcoh).abs().max() <= 1e-10 and coh.max() < 0.1                       # independent rows: about 1 / frames
    assert (api.coherence(x[..., :n_fft], y[..., :n_fft], n_fft) - 1).abs().max() <= 1e-12   # one frame
    # an explicit hop and window, and a window shorter than the frame
    w48 = torch.hann_window(48, periodic=True, dtype=torch.float64)
    Pw = api.welch(x, n_fft, hop_length=20, window=w48, fs=fs, win_length=48)
    Xw = torch.stft(x.reshape(-1, 40000), n_fft, 20, win_length=48, window=w48, center=False, return_complex=True)
    ww = ((Xw.abs() ** 2).mean(-1) * dbl / (fs * (w48 ** 2).sum())).reshape(2, 3, -1)
    assert (Pw - ww).abs().max() <= 1e-12 * ww.max()
    assert (api.welch(x, n_fft, fs=fs, win_length=48) - api.welch(x, n_fft, window=w48, fs=fs, win_length=48)).abs().max() == 0
    with pytest.raises(ValueError):
        api.welch(x, n_fft, scaling="power")


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------------
_MEASURED = {}


def _yardstick():
    """The same-precision CPU pipeline (frames times the window in that precision, scipy.fft's rfft in that precision, numpy's for fp64
    where scipy is missing; conjugate-multiply; sum over the frames in that precision) on exactly the cases of tests/test_gpu_rcsd1d.py:
    worst nu per precision."""
    if _MEASURED:
        return _MEASURED
    precs = A.PRECS if sf is not None else ("f64",)
    mod = sf if sf is not None else np.fft
    for M, rows, frames, hop, tail, wname in WC.all_cases():
        x, g, win, ref, _ = WC.case(M, rows, frames, hop, tail, wname)
        m = 2 * M
        for prec in precs:
            w = win.astype(A.RDT[prec])
            Xs = mod.rfft(WC.frames_of(x.astype(A.RDT[prec]), m, hop) * w, axis=2)
            Gs = mod.rfft(WC.frames_of(g.astype(A.RDT[prec]), m, hop) * w, axis=2)
            assert Xs.dtype == A.CDT[prec]
            got = (np.conj(Xs) * Gs).sum(axis=1, dtype=A.CDT[prec])
            v = WC.nu_lines(got, ref, m, prec)
            if v > _MEASURED.get(prec, (-1.0, ""))[0]:
                _MEASURED[prec] = (v, f"M={M} rows={rows} frames={frames} hop={hop} tail={tail} {wname}")
    return _MEASURED


@pytest.mark.parametrize("prec", A.PRECS)
def test_gpu_bound_is_at_most_eight_times_the_cpu_yardstick(prec):
    if prec == "f32" and sf is None:
        pytest.skip("the fp32 yardstick needs scipy.fft: numpy computes float32 transforms in double")
    from test_gpu_rcsd1d import BOUND
    value, what = _yardstick()[prec]
    print(f"yardstick rcsd1d {prec}: {value:.3f}  ({what})")
    assert 0 < BOUND[prec] <= 8 * value, (prec, BOUND[prec], value, what)
