"""Overlap-save 1-D real FFT convolution (dfft_rconv1d_os), host side (no GPU): the four symbols, the refusals that are decided before
the device is queried, the route and scratch rules, the block chooser, a numpy model of the kernel's item -> (row, block, load window,
store window) arithmetic, the reference against numpy.convolve, the cross-compilation of the new unit, the committed resource inventory
of its kernels, and the CPU yardstick that the GPU bound of tests/test_gpu_rconv1d_os.py is held against."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import accuracy_ref as A
import fused_inventory as FI
import rconv1d_cases as RC
import rconv1d_os_cases as OC

try:
    import scipy.fft as sf
except ImportError:   # pragma: no cover
    sf = None

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "distributedfft_amd" / "csrc"
INVENTORY = ROOT / "profiles" / "2026-10-20_rconv1d_os" / "kernel_resources.txt"
OLD_INVENTORY = ROOT / "profiles" / "2026-10-19_rconv1d" / "kernel_resources.txt"
SYMBOLS = ("dfft_rconv1d_os", "dfft_rconv1d_os_fused_applies", "dfft_rconv1d_os_scratch_bytes", "dfft_rconv1d_os_block")
X, Y, HP = 0x10000000, 0x20000000, 0x30000000
F64, F32, CPLX, REAL = 0, 1, 0, 1
# (M, dtype) on the composed route although M is tuned: those of dfft_rconv1d (rconv_fused_ok) and any whose block kernels would spill
ROUTED = {(3125, F64), (3125, F32), (1536, F64), (2401, F32)}


def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


def _tuned():
    return sorted(RC.plan_points())


def _call(inp=X, out=Y, h=HP, n=200, n_out=200, m=128, d=32, channels=3, batch=4, dtype=F64, kind=CPLX):
    lib = _lib()
    vp = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    rc = lib.dfft_rconv1d_os(vp(inp), vp(out), vp(h), n, n_out, m, d, channels, batch, dtype, kind, None)
    return rc, lib.dfft_last_error().decode()


def _block(taps, n_out, dtype=F64):
    m, d = C.c_longlong(-1), C.c_longlong(-1)
    rc = _lib().dfft_rconv1d_os_block(taps, n_out, dtype, C.byref(m), C.byref(d))
    return rc, m.value, d.value


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
    LL = C.c_longlong
    assert L.SIGNATURES["dfft_rconv1d_os"] == (C.c_int, [C.c_void_p] * 3 + [LL] * 6 + [C.c_int, C.c_int, C.c_void_p])
    assert L.SIGNATURES["dfft_rconv1d_os_fused_applies"] == (C.c_int, [LL, C.c_int])
    assert L.SIGNATURES["dfft_rconv1d_os_scratch_bytes"] == (C.c_ulonglong, [LL] * 5 + [C.c_int])
    assert L.SIGNATURES["dfft_rconv1d_os_block"] == (C.c_int, [LL, LL, C.c_int, C.POINTER(LL), C.POINTER(LL)])
    from distributedfft_amd import api
    for name in ("rconv1d_os", "rconv1d_os_block", "fftfilt1d"):
        assert callable(getattr(api, name))


def test_refusals_are_decided_before_the_device_is_queried():
    from distributedfft_amd import _lib as L
    for dtype in (F64, F32):
        for kind in (CPLX, REAL):
            kw = dict(dtype=dtype, kind=kind)
            assert _call(inp=0, **kw)[0] == L.EINVAL                      # NULL pointers
            assert _call(out=0, **kw)[0] == L.EINVAL
            assert _call(h=0, **kw)[0] == L.EINVAL
            for bad in (0, -3):                                           # sizes below 1
                assert _call(n=bad, n_out=1, **kw)[0] == L.EINVAL
                assert _call(n_out=bad, **kw)[0] == L.EINVAL
                assert _call(m=bad, d=0, **kw)[0] == L.EINVAL
                assert _call(channels=bad, **kw)[0] == L.EINVAL
                assert _call(batch=bad, **kw)[0] == L.EINVAL
            assert _call(d=-1, **kw)[0] == L.EINVAL                       # 0 <= discard <= m - 1
            assert _call(d=128, **kw)[0] == L.EINVAL
            assert _call(d=200, **kw)[0] == L.EINVAL
            assert _call(n=200, n_out=233, **kw)[0] == L.EINVAL           # n_out <= n + discard
            assert _call(n=1, n_out=34, **kw)[0] == L.EINVAL
            assert _call(n=200, n_out=233, m=194, **kw)[0] == L.EINVAL    # ... before m is judged
            rs = 8 if dtype == F64 else 4
            ib, ob = 200 * 12 * rs, 150 * 12 * rs                         # n = 200, n_out = 150
            ov = dict(n=200, n_out=150, **kw)
            assert _call(out=X, inp=X, **ov)[0] == L.EINVAL               # in and out overlapping at all: no in-place form
            assert _call(out=X + rs, **ov)[0] == L.EINVAL
            assert _call(out=X + ib - rs, **ov)[0] == L.EINVAL
            assert _call(inp=Y + ob - rs, **ov)[0] == L.EINVAL
            assert _call(inp=Y + rs, **ov)[0] == L.EINVAL
            hb = 3 * 65 * (rs if kind == REAL else 2 * rs)
            assert _call(h=Y, **ov)[0] == L.EINVAL                        # h overlaps out
            assert _call(h=Y + ob - rs, **ov)[0] == L.EINVAL
            assert _call(h=Y - hb + rs, **ov)[0] == L.EINVAL
            for m in (9, 194, 22, 2, 8194, 16384, 2 * 4099, 1 << 30):    # odd, Bluestein half, 11 | m/2, m/2 = 1, above 8192
                rc, msg = _call(n=1, n_out=1, m=m, d=0, **kw)
                assert rc == L.EUNSUPPORTED and f"m = {m}" in msg, (m, rc, msg)
                assert _lib().dfft_real_form(m) != 1
    for dtype in (-1, 2, 7):
        assert _call(dtype=dtype)[0] == L.EINVAL
    for kind in (-1, 2):
        assert _call(kind=kind)[0] == L.EINVAL
    # 2^31 items or more: by the rows alone, and by rows x blocks
    assert _call(n=1, n_out=1, m=4, d=0, channels=1 << 16, batch=1 << 15)[0] == L.EUNSUPPORTED
    assert _call(n=1, n_out=1, m=4, d=0, channels=1 << 40, batch=1 << 40)[0] == L.EUNSUPPORTED
    assert _call(n=1 << 33, n_out=1 << 33, m=4, d=0, channels=1, batch=1)[0] == L.EUNSUPPORTED       # 2^31 blocks of 4
    assert _call(n=1 << 20, n_out=1 << 20, m=128, d=64, channels=1 << 8, batch=1 << 9, h=1 << 50)[0] == L.EUNSUPPORTED  # 2^17 rows x 2^14 blocks
    assert _call(n=1 << 62, n_out=1 << 62, m=4, d=3, channels=1, batch=1)[0] == L.EUNSUPPORTED


def test_valid_calls_reach_the_device_query():
    from distributedfft_amd import _lib as L
    if _lib().dfft_device_count() > 0:
        return
    far = dict(h=1 << 44, out=1 << 42)
    for M, d in OC.ENTRIES + [(3125, 100)]:
        for c in OC.entry_cases(M, d):
            _, _, n, n_out, channels, batch = c
            for dtype in (F64, F32):
                for kind in (CPLX, REAL):
                    assert _call(n=n, n_out=n_out, m=2 * M, d=d, channels=channels, batch=batch, dtype=dtype, kind=kind, **far)[0] == L.ENOGPU, c
    # ranges that merely touch do not overlap: 12 rows of 200 doubles = 19200 bytes in, 12 x 150 = 14400 bytes out; 3 x 65 complex = 3120
    assert _call(n=200, n_out=150, out=X + 19200)[0] == L.ENOGPU
    assert _call(n=200, n_out=150, inp=Y + 14400)[0] == L.ENOGPU
    assert _call(n=200, n_out=150, h=Y + 14400)[0] == L.ENOGPU
    assert _call(n=200, n_out=150, h=Y - 3120)[0] == L.ENOGPU
    assert _call(n=200, n_out=232)[0] == L.ENOGPU                    # n_out = n + discard
    assert _call(n=1, n_out=33)[0] == L.ENOGPU
    assert _call(m=128, d=127)[0] == L.ENOGPU                        # S = 1
    assert _call(n=1 << 31, n_out=(1 << 31) - 4, m=4, d=0, channels=1, batch=1, **far)[0] == L.ENOGPU   # 2^29 - 1 ... just under 2^31 items
    assert _call(n=((1 << 31) - 1) * 4096, n_out=((1 << 31) - 1) * 4096, m=8192, d=4096, channels=1, batch=1, h=1 << 60, out=1 << 59)[0] == L.ENOGPU


def test_route_and_scratch_rules(monkeypatch):
    """Fused: m/2 tuned and not in the routed list; 0 under DFFT_RCONV_FUSED=0 (read per call).  Scratch: 0 for the fused route, else
    chunk items x (m reals + (m/2 + 1) complex), chunk = min(items, max(256 MiB, one item's) / one item's), items = rows x blocks."""
    lib = _lib()
    monkeypatch.delenv("DFFT_RCONV_FUSED", raising=False)
    tuned = set(_tuned())

    def lease(m, items, dtype):
        cs = 16 if dtype == F64 else 8
        ib = m * cs // 2 + (m // 2 + 1) * cs
        return min(items, max(256 << 20, ib) // ib) * ib

    for M in sorted(tuned | {36, 6, 18, 3600, 2000, 4000}):
        m = 2 * M
        assert lib.dfft_real_form(m) == 1, m
        for dtype in (F64, F32):
            fused = M in tuned and (M, dtype) not in ROUTED
            assert lib.dfft_rconv1d_os_fused_applies(m, dtype) == int(fused), (M, dtype)
            # the rule of dfft_rconv1d, less what is routed here
            assert fused <= bool(lib.dfft_rconv1d_fused_applies(1, m, dtype, CPLX, 0))
            for d in (0, 1, M, m - 1):
                for n_out, channels, batch in ((1, 1, 1), (5 * m + 3, 3, 5), (1 << 20, 16, 8)):
                    items = channels * batch * OC.blocks(n_out, m, d)
                    if items >= 1 << 31:
                        continue
                    got = lib.dfft_rconv1d_os_scratch_bytes(n_out, m, d, channels, batch, dtype)
                    assert got == (0 if fused else lease(m, items, dtype)), (M, dtype, d, n_out, channels, batch, got)
    # not a call the entry point would accept: no route, no lease
    assert lib.dfft_rconv1d_os_fused_applies(22, F64) == 0
    assert lib.dfft_rconv1d_os_fused_applies(128, 5) == 0
    assert lib.dfft_rconv1d_os_fused_applies(16384, F64) == 0
    assert lib.dfft_rconv1d_os_scratch_bytes(100, 22, 0, 1, 1, F64) == 0
    assert lib.dfft_rconv1d_os_scratch_bytes(100, 72, 72, 1, 1, F64) == 0
    assert lib.dfft_rconv1d_os_scratch_bytes(0, 72, 0, 1, 1, F64) == 0
    assert lib.dfft_rconv1d_os_scratch_bytes(1 << 33, 72, 71, 1, 1, F64) == 0           # 2^31 items or more
    assert lib.dfft_rconv1d_os_scratch_bytes(100, 72, 0, 1 << 16, 1 << 15, F64) == 0
    assert lib.dfft_rconv1d_os_scratch_bytes(1 << 20, 8192, 4096, 1, 1000, F64) == 0    # fused
    monkeypatch.setenv("DFFT_RCONV_FUSED", "0")
    assert lib.dfft_rconv1d_os_fused_applies(128, F64) == 0
    # more than one chunk: 8192-point items of 64 KiB + 64 KiB + 16 bytes, 256 blocks a row
    assert lib.dfft_rconv1d_os_scratch_bytes(1 << 20, 8192, 4096, 1, 1000, F64) == lease(8192, 256000, F64) == 2047 * (65536 + 65552)
    assert lib.dfft_rconv1d_os_scratch_bytes(200, 128, 32, 3, 5, F32) == 15 * 3 * (128 * 4 + 65 * 8)
    monkeypatch.setenv("DFFT_RCONV_FUSED", "1")
    assert lib.dfft_rconv1d_os_fused_applies(128, F64) == 1


# ---- the block chooser ------------------------------------------------------------------------------------------------------------------
def test_block_chooser():
    from distributedfft_amd import _lib as L
    from distributedfft_amd import api
    lib = _lib()
    for dtype in (F64, F32):
        for taps in (1, 2, 3, 7, 100, 257, 300, 1025, 4000, 4097, 8190, 8191):
            for n_out in (1, 5, 100, 1000, 8192 - taps, 8192 - taps + 2, 8193, 20000, 65536, 1 << 20, 10 ** 8):
                if n_out < 1:
                    continue
                rc, m, d = _block(taps, n_out, dtype)
                assert rc == 0, (taps, n_out)
                assert d >= taps - 1 and d % 2 == 0 and d - (taps - 1) <= 1, (taps, d)
                assert m > d and lib.dfft_real_form(m) == 1, (taps, n_out, m, d)
                # the entry point accepts it: head (n = n_out) and full (n = n_out - taps + 1) forms
                for n in {n_out, max(1, n_out - taps + 1)}:
                    want = L.ENOGPU if lib.dfft_device_count() < 1 else None
                    if want is not None:
                        assert _call(n=n, n_out=n_out, m=m, d=d, channels=1, batch=1, dtype=dtype, h=1 << 60, out=1 << 59)[0] == want, (taps, n_out, m, d)
                # one block where one fits
                one = lib.dfft_rconv1d_length(n_out + d)
                assert (OC.blocks(n_out, m, d) == 1) == (one != 0), (taps, n_out, m, d, one)
                # long rows are not filtered in blocks that are mostly overlap
                if n_out >= 20000 and taps <= 2048:
                    assert m - d >= d, (taps, n_out, m, d)
        for taps in (8192, 8193, 10 ** 6):
            rc, m, d = _block(taps, 1000, dtype)
            assert rc == L.EUNSUPPORTED and "taps" in lib.dfft_last_error().decode()
    assert _block(0, 100)[0] == L.EINVAL
    assert _block(5, 0)[0] == L.EINVAL
    assert _block(5, 100, 3)[0] == L.EINVAL
    assert lib.dfft_rconv1d_os_block(5, 100, F64, None, None) == L.EINVAL
    assert api.rconv1d_os_block(300, 20299, F64) == _block(300, 20299, F64)[1:]
    with pytest.raises(ValueError):
        api.rconv1d_os_block(8192, 100, F32)


def test_block_times_table_is_one_table_with_a_cited_profile():
    """t(m) comes from one table in dfft_osconv.hip, between two markers, next to the profile it was measured in; every entry is a
    power-of-two block length with positive times that grow with m."""
    src = (CSRC / "dfft_osconv.hip").read_text()
    body = re.search(r"OSCONV_BLOCK_TIMES_BEGIN(.*?)OSCONV_BLOCK_TIMES_END", src, re.S).group(1)
    rows = [(int(m), float(a), float(b)) for m, a, b in re.findall(r"\{(\d+), \{([0-9.]+), ([0-9.]+)\}\}", body)]
    assert [r[0] for r in rows] == [256, 512, 1024, 2048, 4096, 8192]
    for (m0, a0, b0), (m1, a1, b1) in zip(rows, rows[1:]):
        assert 0 < a0 < a1 and 0 < b0 < b1
    cited = re.search(r"profiles/(\d{4}-\d\d-\d\d_rconv1d_os)/README\.md", src)
    assert cited and (ROOT / "profiles" / cited.group(1) / "README.md").exists()


# ---- numpy model of the kernel's item arithmetic ----------------------------------------------------------------------------------------
def kernel_model(xflat, H, rows, n, n_out, m, d, channels, G):
    """The persistent loop of osconv_blocks_kernel over items it = row * nb + b, G items per workgroup step, on FLAT buffers: per item the
    64-bit bases row * n + s0 / row * n_out + s0 with s0 = b S - d, the load window [lo, hi) and the store window [d, he) clamped to
    [0, m].  The block itself is numpy's irfft(rfft * H) (tests/test_rconv1d_host.py models the pairing step).  xflat carries NaN outside
    its rows * n values, so a load outside a row's window shows in the result; a store outside the window trips the assertion."""
    S = m - d
    nb = -(-n_out // S)
    items = rows * nb
    guard = (len(xflat) - rows * n) // 2
    out = np.full(rows * n_out, np.nan)
    written = np.zeros(rows * n_out, dtype=int)
    for i0 in range(0, items, G):
        for g in range(G):
            it = i0 + g
            valid = it < items
            row = it // nb if valid else 0
            b = it - row * nb if valid else 0
            s0 = b * S - d
            clamp = lambda v: min(max(v, 0), m)  # noqa: E731
            lo, hi, he = (clamp(-s0), clamp(n - s0), clamp(n_out - s0)) if valid else (0, 0, 0)
            ibase, obase = row * n + s0, row * n_out + s0
            xb = np.array([xflat[guard + ibase + i] if lo <= i < hi else 0.0 for i in range(m)])
            cb = np.fft.irfft(np.fft.rfft(xb) * H[row % channels], m)
            for i in range(d, m):
                if i < he:
                    assert 0 <= obase + i < rows * n_out
                    out[obase + i] = cb[i]
                    written[obase + i] += 1
    assert np.all(written == 1), "every output real is stored exactly once"
    return out.reshape(rows, n_out)


@pytest.mark.parametrize("kind", OC.KINDS)
@pytest.mark.parametrize("M,d", [(2, 0), (2, 3), (4, 2), (4, 3), (8, 5), (8, 6), (8, 15), (25, 10), (25, 49)])
def test_kernel_model_matches_the_reference(M, d, kind):
    """d even and odd, n_out below, equal to and above n, S = 1, more than one workgroup step with a ragged last one.  Not library code:
    tests/test_gpu_rconv1d_os.py runs the kernels."""
    m, channels, rows = 2 * M, 3, 4
    H = RC.make_filter(channels, m, kind, 7 * M + d)
    for n in OC.n_values(m, d) + [6]:
        for n_out in OC.n_out_values(n, d):
            x = A.rand_real((rows, n), 100 * M + n)
            guard = 2 * m
            xflat = np.concatenate([np.full(guard, np.nan), x.reshape(-1), np.full(guard, np.nan)])
            want = OC.reference(x, H, m, d, n_out).astype(np.float64)
            got = kernel_model(xflat, H, rows, n, n_out, m, d, channels, G=3)
            assert not np.isnan(got).any(), (M, d, n, n_out)
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (M, d, n, n_out, kind)


def test_reference_with_tap_filters_is_numpy_convolve():
    rng = np.random.default_rng(5)
    for n, taps, m, d in ((100, 7, 16, 6), (100, 8, 16, 8), (1000, 33, 128, 32), (50, 1, 4, 0), (37, 20, 72, 20), (5, 3, 8, 7)):
        x, k = rng.standard_normal((4, n)), rng.standard_normal((2, taps))
        H = OC.taps_spectrum(k, m)
        for n_out in (n, n + taps - 1, n - 1):
            want = np.stack([np.convolve(x[r], k[r % 2])[:n_out] for r in range(4)])
            got = OC.reference(x, H, m, d, n_out).astype(np.float64)
            assert np.abs(got - want).max() < 1e-12 * max(1.0, np.abs(want).max()), (n, taps, m, d, n_out)
            assert np.abs(OC.convolve_reference(x, k, n_out).astype(np.float64) - want).max() < 1e-12 * max(1.0, np.abs(want).max())
    # H == 1 and no discard: the identity, block by block
    x = rng.standard_normal((3, 50))
    assert np.abs(OC.reference(x, np.ones((1, 9)), 16, 0, 50).astype(np.float64) - x).max() < 1e-15


# ---- build ------------------------------------------------------------------------------------------------------------------------------
def test_new_unit_cross_compiles(tmp_path):
    """The dispatcher unit of dfft_osconv.hip (composed-route kernels, chooser and host code) builds for gfx950; build() compiles every
    group, under object names that do not collide with dfft_rconv_*."""
    from distributedfft_amd.build import NUM_INST_GROUPS
    obj = tmp_path / "dfft_osconv_dispatch.o"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}", f"-I{CSRC}",
                        f"-DDFFT_INST_GROUP={NUM_INST_GROUPS}", "-c", str(CSRC / "dfft_osconv.hip"), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert obj.stat().st_size > 0
    from distributedfft_amd import build
    names = [u[1].name for u in build.units()]
    assert [f"dfft_osconv_{g}.o" for g in range(NUM_INST_GROUPS + 1)] == [n for n in names if n.startswith("dfft_osconv_")]
    assert not any(n.startswith("dfft_rconv_") for n in names if "osconv" in n)


# ---- resource inventories ---------------------------------------------------------------------------------------------------------------
def test_inventory_belongs_to_the_sources_and_no_block_kernel_spills():
    """profiles/2026-10-20_rconv1d_os/kernel_resources.txt (tools/fused_resources.py osconv) must carry the sha256 of the sources in the tree
    and list every block-kernel instantiation -- tuned M x fp64 / fp32 x complex / real filter x two-real / per-real accesses, less the
    ones on the composed route, which it names -- with zero scratch."""
    text = FI.current_text("osconv")
    fused = [ln for ln in text.splitlines() if ln.startswith("osconv_blocks_kernel ")]
    m = re.search(r"^# composed-route \(M, type, filter, form\): (.*)$", text, re.M)
    assert m
    routed = {(int(n), t, f, a) for n, t, f, a in re.findall(r"\((\d+), (f64|f32), (complex|real), (vec|real)\)", m.group(1))}
    assert {(n, F64 if t == "f64" else F32) for n, t, _, _ in routed} == ROUTED
    assert len(routed) == 4 * len(ROUTED) <= 24, "a few instantiations, all four forms of an (M, dtype) together"
    want = {(n, t, f, a) for n in _tuned() for t in ("f64", "f32") for f in ("complex", "real") for a in ("vec", "real")} - routed
    seen = set()
    for ln in fused:
        g = re.match(r"osconv_blocks_kernel (f64|f32) M=(\d+) E=\d+ filter=(complex|real) form=(vec|real) ", ln)
        assert g, ln
        seen.add((int(g.group(2)), g.group(1), g.group(3), g.group(4)))
    assert seen == want and len(fused) == len(want)
    helpers = [ln for ln in text.splitlines() if ln.startswith(("osconv_gather_", "osconv_mul_", "osconv_scatter_"))]
    assert len(helpers) == 8
    for ln in fused + helpers:
        assert re.search(r"scratch=(\d+)", ln).group(1) == "0", ln
    # the routed lengths are lengths the source names, and the library routes them
    src = (CSRC / "dfft_osconv.hip").read_text()
    body = re.search(r"constexpr bool osconv_fused_ok\(int M, bool f64\) \{(.*?)\n\}", src, re.S).group(1)
    lib = _lib()
    for n, t, _, _ in routed:
        assert re.search(rf"\b{n}\b", body), n
        assert lib.dfft_rconv1d_os_fused_applies(2 * n, F64 if t == "f64" else F32) == 0


def test_row_kernel_takes_the_shared_types_and_its_inventory_was_regenerated():
    """dfft_rconv.hip takes RconvGeom / RconvFilter from dfft_rconv_impl.h, which the block kernel shares; its inventory was regenerated
    for the new sources (tests/test_rconv1d_host.py holds its contents)."""
    FI.current_text("rconv")   # (asserts that the inventory carries the hash of the sources in the tree)
    assert '#include "dfft_rconv_impl.h"' in (CSRC / "dfft_rconv.hip").read_text()
    assert "struct RconvGeom" not in (CSRC / "dfft_rconv.hip").read_text() and "struct RconvGeom" in (CSRC / "dfft_rconv_impl.h").read_text()


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------------
_MEASURED = {}


def _yardstick():
    """The same-precision CPU FFT pipeline (scipy.fft per block; numpy for fp64 where scipy is missing) on exactly the cases of
    tests/test_gpu_rconv1d_os.py: worst nu per precision."""
    if _MEASURED:
        return _MEASURED
    precs = A.PRECS if sf is not None else ("f64",)
    mod = sf if sf is not None else np.fft
    for M, d, n, n_out, channels, batch, kind in OC.all_cases():
        x, H, ref = OC.case(M, d, n, n_out, channels, batch, kind)
        m = 2 * M
        for prec in precs:
            Hp = H.astype(A.RDT[prec] if kind == "real" else A.CDT[prec])[np.arange(x.shape[0]) % channels][:, None, :]
            xb = OC.gather(x.astype(A.RDT[prec]), m, d, n_out)
            cb = mod.irfft(mod.rfft(xb, m, axis=2) * Hp, m, axis=2)
            assert cb.dtype == A.RDT[prec] or sf is None
            got = cb[:, :, d:].reshape(x.shape[0], -1)[:, :n_out]
            v = OC.nu_rows(got, ref, m, prec)
            if v > _MEASURED.get(prec, (-1.0, ""))[0]:
                _MEASURED[prec] = (v, f"M={M} d={d} n={n} n_out={n_out} channels={channels} {kind}")
    return _MEASURED


@pytest.mark.parametrize("prec", A.PRECS)
def test_gpu_bound_is_at_most_eight_times_the_cpu_yardstick(prec):
    if prec == "f32" and sf is None:
        pytest.skip("the fp32 yardstick needs scipy.fft: numpy computes float32 transforms in double")
    from test_gpu_rconv1d_os import BOUND
    value, what = _yardstick()[prec]
    print(f"yardstick rconv1d_os {prec}: {value:.3f}  ({what})")
    assert 0 < BOUND[prec] <= 8 * value, (prec, BOUND[prec], value, what)
