"""Batched short-time Fourier transform (dfft_stft1d / dfft_istft1d), host side (no GPU): the six symbols, the frame count against a brute
force, the refusals that are decided before the device is queried, the route and scratch rules, the cross-compilation of the new unit,
the committed resource inventory of its kernels, and the references of tests/stft_cases.py against torch.stft / torch.istft on the CPU."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

import accuracy_ref as A
import fused_inventory as FI
import rconv1d_cases as RC
import stft_cases as SC

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "distributedfft_amd" / "csrc"
INVENTORY = ROOT / "profiles" / "2026-10-20_stft" / "kernel_resources.txt"
SYMBOLS = ("dfft_stft1d", "dfft_istft1d", "dfft_stft1d_frames", "dfft_stft1d_fused_applies", "dfft_stft1d_scratch_bytes", "dfft_istft1d_scratch_bytes")
X, Y, W, E = 0x10000000, 0x20000000, 0x30000000, 0x38000000
F64, F32, ZERO, REFLECT, CPLX, POWER = 0, 1, 0, 1, 0, 1
PREC = {F64: "f64", F32: "f32"}


def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


def _tuned():
    return sorted(RC.plan_points())


def _vp(p):
    return C.c_void_p(p) if p else None


def _fwd(inp=X, out=Y, win=W, n=386, m=128, hop=32, pad=64, frames=None, rows=3, dtype=F64, mode=REFLECT, kind=CPLX, scale=1.0):
    lib = _lib()
    if frames is None:
        frames = max(1, lib.dfft_stft1d_frames(n, m, hop, pad))
    rc = lib.dfft_stft1d(_vp(inp), _vp(out), _vp(win), n, m, hop, pad, frames, rows, dtype, mode, kind, scale, None)
    return rc, lib.dfft_last_error().decode()


def _inv(inp=X, out=Y, win=W, env=E, n=320, m=128, hop=32, pad=64, frames=9, rows=3, dtype=F64):
    lib = _lib()
    rc = lib.dfft_istft1d(_vp(inp), _vp(out), _vp(win), _vp(env), n, m, hop, pad, frames, rows, dtype, None)
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
    LL, VP = C.c_longlong, C.c_void_p
    assert L.SIGNATURES["dfft_stft1d"] == (C.c_int, [VP] * 3 + [LL] * 6 + [C.c_int] * 3 + [C.c_double, VP])
    assert L.SIGNATURES["dfft_istft1d"] == (C.c_int, [VP] * 4 + [LL] * 6 + [C.c_int, VP])
    assert L.SIGNATURES["dfft_stft1d_frames"] == (LL, [LL] * 4)
    assert L.SIGNATURES["dfft_stft1d_fused_applies"] == (C.c_int, [LL, C.c_int])
    assert L.SIGNATURES["dfft_stft1d_scratch_bytes"] == (C.c_ulonglong, [LL] * 3 + [C.c_int, C.c_int])
    assert L.SIGNATURES["dfft_istft1d_scratch_bytes"] == (C.c_ulonglong, [LL] * 3 + [C.c_int])
    for name, value in (("DFFT_STFT_PAD_ZERO", 0), ("DFFT_STFT_PAD_REFLECT", 1), ("DFFT_STFT_OUT_COMPLEX", 0), ("DFFT_STFT_OUT_POWER", 1)):
        assert re.search(rf"#define {name} {value}\b", header), name
    from distributedfft_amd import api
    for name in ("stft", "istft", "stft_frames"):
        assert callable(getattr(api, name))
    assert (api.STFT_PAD_ZERO, api.STFT_PAD_REFLECT, api.STFT_OUT_COMPLEX, api.STFT_OUT_POWER) == (0, 1, 0, 1)


def test_frame_count_against_a_brute_force():
    from distributedfft_amd import api
    lib = _lib()
    for n in range(1, 41):
        for m in range(1, 17):
            for hop in range(1, 19):
                for pad in range(m):
                    # frames f >= 0 whose m samples from f hop - pad on lie inside the padded row [-pad, n + pad)
                    brute = sum(1 for f in range(n + 2 * pad + 1) if f * hop - pad + m <= n + pad)
                    assert lib.dfft_stft1d_frames(n, m, hop, pad) == brute == SC.frames_of(n, m, hop, pad), (n, m, hop, pad)
    for bad in ((0, 8, 2, 0), (10, 0, 2, 0), (10, 8, 0, 0), (10, 8, 2, -1), (10, 8, 2, 8), (-5, 8, 2, 7)):
        assert lib.dfft_stft1d_frames(*bad) == 0, bad
    assert lib.dfft_stft1d_frames(1 << 40, 8192, 1, 4096) == (1 << 40) + 1
    assert api.stft_frames(65536, 1024, 256, 512) == 257


def test_refusals_are_decided_before_the_device_is_queried():
    from distributedfft_amd import _lib as L
    for dtype in (F64, F32):
        rs = 8 if dtype == F64 else 4
        for kind in (CPLX, POWER):
            kw = dict(dtype=dtype, kind=kind)
            for name in ("inp", "out", "win"):                              # NULL pointers
                assert _fwd(**{name: 0}, **kw)[0] == L.EINVAL
            for bad in (0, -3):                                             # sizes below 1
                for name in ("n", "m", "hop", "frames", "rows"):
                    assert _fwd(**{name: bad}, **kw)[0] == L.EINVAL, (name, bad)
            assert _fwd(pad=-1, **kw)[0] == L.EINVAL                        # 0 <= pad < m
            assert _fwd(pad=128, **kw)[0] == L.EINVAL
            assert _fwd(pad=194, m=194, **kw)[0] == L.EINVAL               # ... before m is judged
            assert _fwd(frames=14, **kw)[0] == L.EINVAL                     # 386 samples padded by 64 on both sides give 13 frames
            assert _fwd(frames=1 << 20, **kw)[0] == L.EINVAL
            assert _fwd(n=100, pad=0, frames=1, **kw)[0] == L.EINVAL        # shorter than one frame: no frames at all
            assert _fwd(n=64, pad=64, mode=REFLECT, **kw)[0] == L.EINVAL    # reflect needs pad < n
            assert _fwd(n=10, pad=64, mode=REFLECT, **kw)[0] == L.EINVAL
            for mode in (-1, 2):
                assert _fwd(mode=mode, **kw)[0] == L.EINVAL
            ib = 3 * 386 * rs
            ob = 3 * 13 * 65 * (rs if kind == POWER else 2 * rs)
            wb = 128 * rs
            assert _fwd(out=X, **kw)[0] == L.EINVAL                         # in, out and win overlapping
            assert _fwd(out=X + ib - rs, **kw)[0] == L.EINVAL
            assert _fwd(inp=Y + ob - rs, **kw)[0] == L.EINVAL
            assert _fwd(win=Y, **kw)[0] == L.EINVAL
            assert _fwd(win=Y + ob - rs, **kw)[0] == L.EINVAL
            assert _fwd(win=Y - wb + rs, **kw)[0] == L.EINVAL
            assert _fwd(win=X + rs, **kw)[0] == L.EINVAL
            assert _fwd(win=X - wb + rs, **kw)[0] == L.EINVAL
            for m in (9, 194, 22, 2, 8194, 16384, 2 * 4099, 1 << 30):       # odd, Bluestein half, 11 | m/2, m/2 = 1, above 8192
                rc, msg = _fwd(n=1 << 31, m=m, hop=1, pad=0, frames=1, rows=1, mode=ZERO, **kw)
                assert rc == L.EUNSUPPORTED and f"m = {m}" in msg, (m, rc, msg)
                assert _lib().dfft_real_form(m) != 1
        for name in ("inp", "out", "win", "env"):
            assert _inv(**{name: 0}, dtype=dtype)[0] == L.EINVAL
        for bad in (0, -3):
            for name in ("n", "m", "hop", "frames", "rows"):
                assert _inv(**{name: bad}, dtype=dtype)[0] == L.EINVAL, (name, bad)
        assert _inv(pad=-1, dtype=dtype)[0] == L.EINVAL
        assert _inv(pad=128, dtype=dtype)[0] == L.EINVAL
        assert _inv(n=321, dtype=dtype)[0] == L.EINVAL                      # n <= (frames - 1) hop + m - pad = 320
        assert _inv(n=385, pad=0, dtype=dtype)[0] == L.EINVAL
        assert _inv(n=1 << 62, hop=1 << 61, frames=3, dtype=dtype)[0] == L.EINVAL   # frames * hop is held below 2^62
        ib, ob, wb, eb = 3 * 9 * 65 * 2 * rs, 3 * 320 * rs, 128 * rs, 320 * rs
        assert _inv(out=X, dtype=dtype)[0] == L.EINVAL
        assert _inv(out=X + ib - rs, dtype=dtype)[0] == L.EINVAL
        assert _inv(inp=Y + ob - rs, dtype=dtype)[0] == L.EINVAL
        assert _inv(win=Y + ob - rs, dtype=dtype)[0] == L.EINVAL
        assert _inv(env=Y - eb + rs, dtype=dtype)[0] == L.EINVAL
        assert _inv(win=X + rs, dtype=dtype)[0] == L.EINVAL
        assert _inv(env=X + ib - rs, dtype=dtype)[0] == L.EINVAL
        assert _inv(env=W + wb - rs, dtype=dtype)[0] == L.EINVAL
        for m in (9, 194, 22, 2, 8194, 16384):
            rc, msg = _inv(n=1, m=m, hop=1, pad=0, frames=1, rows=1, dtype=dtype)
            assert rc == L.EUNSUPPORTED and f"m = {m}" in msg, (m, rc, msg)
    for dtype in (-1, 2, 7):
        assert _fwd(dtype=dtype)[0] == L.EINVAL
        assert _inv(dtype=dtype)[0] == L.EINVAL
    for kind in (-1, 2):
        assert _fwd(kind=kind)[0] == L.EINVAL
    # 2^31 items or more: by the rows alone, and by rows x frames
    far = dict(out=1 << 59, win=1 << 58)
    assert _fwd(n=4, m=4, hop=1, pad=0, frames=1, rows=1 << 31, mode=ZERO, **far)[0] == L.EUNSUPPORTED
    assert _fwd(n=1 << 33, m=4, hop=1, pad=0, frames=1 << 31, rows=1, mode=ZERO, **far)[0] == L.EUNSUPPORTED
    assert _fwd(n=1 << 20, m=128, hop=32, pad=0, frames=1 << 14, rows=1 << 17, mode=ZERO, **far)[0] == L.EUNSUPPORTED
    assert _inv(n=4, m=4, hop=1, pad=0, frames=1, rows=1 << 31, env=1 << 57, **far)[0] == L.EUNSUPPORTED
    assert _inv(n=1 << 31, m=4, hop=1, pad=0, frames=1 << 31, rows=1, env=1 << 57, **far)[0] == L.EUNSUPPORTED


def test_valid_calls_reach_the_device_query():
    from distributedfft_amd import _lib as L
    if _lib().dfft_device_count() > 0:
        return
    far = dict(out=1 << 44, win=1 << 42)
    for case in SC.FORWARD + sorted(SC.LOOP):
        M, hop, pad, n, _ = case
        for mode in (ZERO, REFLECT):
            if mode == REFLECT and pad >= n:
                continue
            for dtype in (F64, F32):
                for kind in (CPLX, POWER):
                    assert _fwd(n=n, m=2 * M, hop=hop, pad=pad, dtype=dtype, mode=mode, kind=kind, **far)[0] == L.ENOGPU, case
    for M, hop, pad, frames, _ in SC.INVERSE:
        for dtype in (F64, F32):
            n = (frames - 1) * hop + 2 * M - pad
            assert _inv(n=n, m=2 * M, hop=hop, pad=pad, frames=frames, dtype=dtype, env=1 << 40, **far)[0] == L.ENOGPU
            assert _inv(n=1, m=2 * M, hop=hop, pad=pad, frames=frames, dtype=dtype, env=1 << 40, **far)[0] == L.ENOGPU
    # ranges that merely touch do not overlap: 3 rows of 386 doubles = 9264 bytes in, 3 x 12 frames x 65 complex = 37440 bytes out
    assert _fwd(frames=12, out=X + 9264)[0] == L.ENOGPU
    assert _fwd(frames=12, inp=Y + 37440)[0] == L.ENOGPU
    assert _fwd(frames=12, win=Y + 37440)[0] == L.ENOGPU
    assert _fwd(frames=12, win=X - 1024)[0] == L.ENOGPU
    assert _fwd(frames=1)[0] == L.ENOGPU                              # fewer frames than the rows give
    assert _fwd(n=65, pad=64, frames=1)[0] == L.ENOGPU                # reflect with pad = n - 1
    assert _fwd(n=1, pad=127, mode=ZERO)[0] == L.ENOGPU
    assert _fwd(n=(1 << 31) + 2, m=4, hop=1, pad=0, rows=1, mode=ZERO, **far)[0] == L.ENOGPU    # 2^31 - 1 items
    assert _inv(n=320)[0] == L.ENOGPU
    assert _inv(n=384, pad=0)[0] == L.ENOGPU


def test_route_and_scratch_rules(monkeypatch):
    """Fused: m/2 tuned and not in the routed list; 0 under DFFT_STFT_FUSED=0 (read per call).  Scratch: 0 for the fused route and for
    refused sizes, else chunk items x one item's bytes, chunk = min(items, max(cap, one item's) / one item's), cap 256 MiB or
    DFFT_STFT_CHUNK_BYTES."""
    lib = _lib()
    monkeypatch.delenv("DFFT_STFT_FUSED", raising=False)
    monkeypatch.delenv("DFFT_STFT_CHUNK_BYTES", raising=False)
    monkeypatch.delenv("DFFT_SCRATCH_CHUNK_BYTES", raising=False)
    tuned = set(_tuned())

    def lease(ib, items, cap=256 << 20):
        return min(items, max(cap, ib) // ib) * ib

    for M in sorted(tuned | {36, 6, 18, 3600, 2000, 4000}):
        m = 2 * M
        assert lib.dfft_real_form(m) == 1, m
        for dtype in (F64, F32):
            cs = 16 if dtype == F64 else 8
            fused = M in tuned and (M, PREC[dtype]) not in SC.ROUTED
            assert lib.dfft_stft1d_fused_applies(m, dtype) == int(fused), (M, dtype)
            for frames, rows in ((1, 1), (13, 3), (1 << 16, 4096)):
                for kind in (CPLX, POWER):
                    ib = m * cs // 2 + ((M + 1) * cs if kind == POWER else 0)
                    got = lib.dfft_stft1d_scratch_bytes(m, frames, rows, dtype, kind)
                    assert got == (0 if fused else lease(ib, frames * rows)), (M, dtype, frames, rows, kind, got)
                ib = m * cs // 2 + (0 if M in tuned else (M + 1) * cs)
                assert lib.dfft_istft1d_scratch_bytes(m, frames, rows, dtype) == lease(ib, frames * rows), (M, dtype, frames, rows)
    # not a call the entry points would accept: no route, no lease
    assert lib.dfft_stft1d_fused_applies(22, F64) == 0
    assert lib.dfft_stft1d_fused_applies(128, 5) == 0
    assert lib.dfft_stft1d_fused_applies(16384, F64) == 0
    assert lib.dfft_stft1d_fused_applies(2, F64) == 0
    for bad in ((22, 10, 1, F64, CPLX), (72, 0, 1, F64, CPLX), (72, 10, 0, F64, CPLX), (72, 10, 1, 3, CPLX), (72, 10, 1, F64, 2), (72, 1 << 31, 1, F64, CPLX),
                (72, 1 << 16, 1 << 15, F64, POWER)):
        assert lib.dfft_stft1d_scratch_bytes(*bad) == 0, bad
        assert lib.dfft_istft1d_scratch_bytes(*bad[:4]) == 0 or bad[4] == 2, bad
    assert lib.dfft_stft1d_scratch_bytes(8192, 1000, 1000, F64, CPLX) == 0      # fused
    monkeypatch.setenv("DFFT_STFT_FUSED", "0")
    assert lib.dfft_stft1d_fused_applies(128, F64) == 0
    # more than one chunk: 8192-point items of 64 KiB (and 64 KiB + 16 bytes of bins for the power form)
    assert lib.dfft_stft1d_scratch_bytes(8192, 1000, 1000, F64, CPLX) == 4096 * 65536
    assert lib.dfft_stft1d_scratch_bytes(8192, 1000, 1000, F64, POWER) == 2047 * (65536 + 65552)
    assert lib.dfft_stft1d_scratch_bytes(128, 13, 3, F32, POWER) == 39 * (128 * 4 + 65 * 8)
    monkeypatch.setenv("DFFT_STFT_CHUNK_BYTES", "5000")
    assert lib.dfft_stft1d_scratch_bytes(128, 13, 3, F32, CPLX) == 9 * 512
    assert lib.dfft_istft1d_scratch_bytes(128, 13, 3, F64) == 4 * 1024
    assert lib.dfft_istft1d_scratch_bytes(8192, 13, 3, F64) == 65536          # one item's where the cap is below it
    monkeypatch.setenv("DFFT_STFT_FUSED", "1")
    assert lib.dfft_stft1d_fused_applies(128, F64) == 1


# ---- build ------------------------------------------------------------------------------------------------------------------------------
def test_new_unit_cross_compiles(tmp_path):
    """The dispatcher unit of dfft_stft.hip (the composed-route kernels, the inverse and the host code) builds for gfx950; build()
    compiles one object per group plus the dispatcher, under names that do not collide with dfft_rconv_*."""
    from distributedfft_amd.build import NUM_INST_GROUPS
    obj = tmp_path / "dfft_stft_dispatch.o"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}", f"-I{CSRC}",
                        f"-DDFFT_INST_GROUP={NUM_INST_GROUPS}", "-c", str(CSRC / "dfft_stft.hip"), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert obj.stat().st_size > 0
    from distributedfft_amd import build
    names = [u[1].name for u in build.units()]
    assert [f"dfft_stft_{g}.o" for g in range(NUM_INST_GROUPS + 1)] + ["dfft_stft_api.o"] == [n for n in names if n.startswith("dfft_stft_")]
    assert not any(n.startswith("dfft_rconv_") for n in names if "stft" in n)


# ---- the resource inventory -------------------------------------------------------------------------------------------------------------
def test_inventory_belongs_to_the_sources_and_no_frame_kernel_spills():
    """profiles/2026-10-20_stft/kernel_resources.txt (tools/fused_resources.py stft) must carry the sha256 of the sources in the tree and list
    every frame-kernel instantiation -- tuned M x fp64 / fp32 x complex / power x two-real / per-real loads, less the ones on the
    composed route, which it names -- with zero scratch; the routed lengths are the ones stft_fused_ok names and the library routes."""
    text = FI.current_text("stft")
    fused = [ln for ln in text.splitlines() if ln.startswith("stft_frames_kernel ")]
    m = re.search(r"^# composed-route \(M, type, out, form\), stft_fused_ok: (.*)$", text, re.M)
    assert m
    routed = {(int(n), t, o, a) for n, t, o, a in re.findall(r"\((\d+), (f64|f32), (complex|power), (vec|real)\)", m.group(1))}
    assert {(n, t) for n, t, _, _ in routed} == SC.ROUTED
    assert len(routed) == 4 * len(SC.ROUTED) <= 24, "a few instantiations, all four forms of an (M, dtype) together"
    want = {(n, t, o, a) for n in _tuned() for t in ("f64", "f32") for o in ("complex", "power") for a in ("vec", "real")} - routed
    seen = set()
    for ln in fused:
        g = re.match(r"stft_frames_kernel (f64|f32) M=(\d+) E=\d+ out=(complex|power) form=(vec|real) ", ln)
        assert g, ln
        seen.add((int(g.group(2)), g.group(1), g.group(3), g.group(4)))
    assert seen == want and len(fused) == len(want)
    helpers = [ln for ln in text.splitlines() if ln.startswith(("stft_gather_", "stft_power_", "istft_ola_"))]
    assert len(helpers) == 6
    for ln in fused + helpers:
        assert re.search(r"scratch=(\d+)", ln).group(1) == "0", ln
    src = (CSRC / "dfft_stft.hip").read_text()
    body = re.search(r"constexpr bool stft_fused_ok\(int M, bool f64\) \{(.*?)\n\}", src, re.S).group(1)
    lib = _lib()
    for n, t, _, _ in routed:
        assert re.search(rf"\b{n}\b", body), n
        assert lib.dfft_stft1d_fused_applies(2 * n, F64 if t == "f64" else F32) == 0
    for n, t, _, _ in want:
        assert lib.dfft_stft1d_fused_applies(2 * n, F64 if t == "f64" else F32) == 1
    for M, prec in [(M, p) for M in SC.TUNED_HALVES + SC.UNTUNED_HALVES for p in A.PRECS]:
        assert SC.fused(M, prec) == bool(lib.dfft_stft1d_fused_applies(2 * M, F64 if prec == "f64" else F32)), (M, prec)


def test_pinned_sources_are_untouched_and_only_included():
    """dfft_stft.hip takes RconvGeom from dfft_rconv_impl.h and launch_real_rows from dfft_real.h; it defines neither."""
    src = (CSRC / "dfft_stft.hip").read_text()
    assert '#include "dfft_rconv_impl.h"' in src and '#include "dfft_real.h"' in src
    assert "struct RconvGeom" not in src and "RconvGeom<V, P>" in src


# ---- the references ---------------------------------------------------------------------------------------------------------------------
def test_cases_cover_what_they_claim():
    """Every half length, hop, pad and row-length class of the table; n, hop and pad all even at least once and each odd at least once; no
    reference frame identically zero (accuracy_ref.nu would refuse it)."""
    cases = SC.FORWARD
    assert {c[0] for c in cases} >= {2, 8, 25, 64, 512, 4096, 18} and {c[0] for c in cases} & {M for M, _ in SC.ROUTED}
    base = [c for c in cases if c[0] == 64]
    assert {c[1] for c in base} >= {1, 7, 32, 128, 131} and {c[2] for c in base} >= {0, 1, 64, 127}
    assert any(c[3] < 128 for c in base) and any(c[3] == 128 for c in base) and any(c[3] % 2 for c in base)
    assert any(c[1] % 2 == 0 and c[2] % 2 == 0 and c[3] % 2 == 0 for c in cases)
    for k in (1, 2, 3):
        assert any(c[k] % 2 for c in cases)
    for case in [c for c in cases if c[0] <= 64]:
        for mode in SC.MODES:
            if SC.usable(case, mode):
                _, _, frames, ref = SC.forward_case(*case, mode)
                assert frames == SC.frames_of(case[3], 2 * case[0], case[1], case[2])
                assert np.all(np.sum(SC.power(ref), axis=-1) > 0)
    for case in SC.LOOP:
        assert SC.frames_of(case[3], 2 * case[0], case[1], case[2]) * SC.ROWS * SC.LOOP[case] > 256 * (2 if case[0] > 64 else 8 * 256)


def _torch_cpu_stft_runs():
    import torch
    try:
        torch.stft(torch.ones(64, dtype=torch.float64), 16, window=torch.ones(16, dtype=torch.float64), return_complex=True)
        return True
    except RuntimeError:
        return False


def test_reference_is_torch_stft_and_istft_on_the_cpu():
    """The longdouble reference against torch.stft / torch.istft (float64, CPU): reflect and constant padding, a Hann window, hop = m / 4
    and m / 2.  Where this build of torch has no CPU FFT the test compares with a second, independent numpy formulation (a direct DFT
    matrix on frames cut from a padded copy) instead."""
    import torch
    rng = np.random.default_rng(11)
    x = rng.standard_normal((2, 300))
    have_torch = _torch_cpu_stft_runs()
    print("torch CPU stft runs on this build:", have_torch)
    for m in (16, 50, 128):
        for hop in (m // 4, m // 2):
            win = torch.hann_window(m, dtype=torch.float64).numpy()
            for mode, tmode in (("reflect", "reflect"), ("zero", "constant")):
                pad = m // 2
                frames = SC.frames_of(300, m, hop, pad)
                ref = SC.reference(x, win, m, hop, pad, frames, mode)
                if have_torch:
                    want = torch.stft(torch.from_numpy(x), m, hop, window=torch.from_numpy(win), center=True, pad_mode=tmode, onesided=True,
                                      return_complex=True).numpy().transpose(0, 2, 1)
                else:
                    xp = np.pad(x, ((0, 0), (pad, pad)), mode="reflect" if mode == "reflect" else "constant")
                    fr = np.stack([xp[:, f * hop:f * hop + m] for f in range(frames)], axis=1) * win
                    dft = np.exp(-2j * np.pi * np.outer(np.arange(m), np.arange(m // 2 + 1)) / m)
                    want = fr @ dft
                assert want.shape == ref.shape
                assert np.abs(ref.astype(np.complex128) - want).max() < 1e-11 * np.abs(want).max(), (m, hop, mode)
                # the inverse: torch.istft of the spectra gives the rows back, and so does the overlap-add reference
                env = SC.envelope(win, m, hop, frames)[pad:pad + 300 - 300 % hop]
                n = len(env)
                back = SC.inverse_reference(ref, win, 1 / env, n, m, hop, pad).astype(np.float64)
                assert np.abs(back - x[:, :n]).max() < 1e-11, (m, hop, mode)
                if have_torch:
                    tb = torch.istft(torch.from_numpy(np.ascontiguousarray(want.transpose(0, 2, 1))), m, hop, window=torch.from_numpy(win), center=True,
                                     length=n).numpy()
                    assert np.abs(back - tb).max() < 1e-11, (m, hop, mode)
    # random half spectra (not the transform of any signal): the least-squares overlap-add itself
    X = A.rand_complex((2, 7, 33), 12)
    win = SC.window(64, "hann")
    env = SC.envelope(win, 64, 16, 7)
    mine = SC.inverse_reference(X, win, 1 / env[32:32 + 96], 96, 64, 16, 32).astype(np.float64)
    if have_torch:
        tb = torch.istft(torch.from_numpy(np.ascontiguousarray(X.transpose(0, 2, 1))), 64, 16, window=torch.from_numpy(win), center=True, length=96).numpy()
        assert np.abs(mine - tb).max() < 1e-11 * np.abs(tb).max()
