"""Long 1-D real FFT convolution (dfft_rconv1d_long), host side (no GPU): the symbols, a numpy restatement of the three passes held
against numpy's irfft(rfft(x, m) * H, m)[:n], dfft_rconv1d_long_length and the split, the refusals that are decided before the device is
queried, the scratch rule, the build units and the committed resource inventory of the kernels."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fused_inventory as FI
import rconv1d_long_cases as LC

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "distributedfft_amd" / "csrc"
INVENTORY = ROOT / "profiles" / "2026-10-20_rconv1d_long" / "kernel_resources.txt"
SYMBOLS = ("dfft_rconv1d_long", "dfft_rconv1d_long_length", "dfft_rconv1d_long_split", "dfft_rconv1d_long_filter",
           "dfft_rconv1d_long_fused_applies", "dfft_rconv1d_long_scratch_bytes")
X, Y, HP = 0x10000000, 0x20000000, 0x30000000
F64, F32, CPLX, REAL = 0, 1, 0, 1
# (N, dtype) that tools/fused_resources.py lconv found spilling or tools/lconv_bench.py slower: the composed route (lconv_fused_ok of dfft_lconv.hip)
ROUTED = set()


def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


def _call(inp=X, out=Y, hp=HP, n=9000, m=16384, channels=3, batch=4, dtype=F64, kind=CPLX):
    lib = _lib()
    vp = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    rc = lib.dfft_rconv1d_long(vp(inp), vp(out), vp(hp), n, m, channels, batch, dtype, kind, None)
    return rc, lib.dfft_last_error().decode()


def _split(m):
    a, b = C.c_int(0), C.c_int(0)
    return (a.value, b.value) if _lib().dfft_rconv1d_long_split(m, C.byref(a), C.byref(b)) == 1 else None


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_signatures_agree_on_the_symbols():
    from distributedfft_amd import _lib as L
    from distributedfft_amd import api
    header = (ROOT / "include" / "dfft.h").read_text()
    lib = _lib()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES, name
        assert getattr(lib, name) is not None
    for path in (L.LIB_PATH, L.LIB_PATH_SYSTEM):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
        assert set(SYMBOLS) <= set(re.findall(r" T (dfft_[a-z0-9_]+)", out)), path
    assert L.SIGNATURES["dfft_rconv1d_long"][1] == [C.c_void_p] * 3 + [C.c_longlong] * 4 + [C.c_int, C.c_int, C.c_void_p]
    assert L.SIGNATURES["dfft_rconv1d_long_length"] == (C.c_longlong, [C.c_longlong])
    assert L.SIGNATURES["dfft_rconv1d_long_scratch_bytes"][0] == C.c_ulonglong
    assert "DFFT_RCONV_LONG_FUSED" in header
    for name in ("rconv1d_long_length", "rconv1d_long_filter", "rconv1d_long", "fftconv1d_long"):
        assert callable(getattr(api, name)), name


# ---- numpy model of the three passes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LC.KINDS)
@pytest.mark.parametrize("n1,n2", [(4, 8), (3, 8), (5, 5), (8, 4), (2, 3)])
def test_pipeline_model_matches_numpy(n1, n2, kind):
    """The identity on a numpy restatement of the kernels -- the [k1][k2] layout, the partner map, rows 0 and N1/2, the factored pairing
    twiddle, the filter permutation; odd N1 and odd M included.  Not library code: tests/test_gpu_rconv1d_long.py runs the kernels."""
    M = n1 * n2
    m = 2 * M
    rng = np.random.default_rng(100 * n1 + n2 + (kind == "complex"))
    H = LC.make_filter(1, m, kind, M)
    hp = LC.permute_filter(H, n1, n2)[0]
    for k1 in range(n1):
        for k2 in range(n2):
            assert hp[k1 * n2 + k2] == H[0, k1 + n1 * k2]
    assert hp[M] == H[0, M] and sorted(hp.tolist(), key=lambda v: (v.real, v.imag)) == sorted(H[0].tolist(), key=lambda v: (v.real, v.imag))
    for n in (m, m // 2, m // 2 + 1, 5, 1):
        x = rng.standard_normal(n)
        want = np.fft.irfft(np.fft.rfft(x, m) * H[0], m)[:n]
        got = LC.pipeline_model(x, hp, n1, n2)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (n1, n2, n, kind)
    x = rng.standard_normal(m)                # H == 1: the identity
    assert np.abs(LC.pipeline_model(x, np.ones(M + 1), n1, n2) - x).max() <= 1e-12 * np.abs(x).max()


# ---- length and split -------------------------------------------------------------------------------------------------------------------
def test_length_and_split():
    lib = _lib()
    from distributedfft_amd import api
    accepted = sorted({2 * a * b for a in LC.FACTORS for b in LC.FACTORS if 8192 < 2 * a * b <= 1 << 23})
    assert accepted[0] == 10240 <= 16384 and accepted[-1] == 1 << 23
    assert lib.dfft_rconv1d_long_length(0) == lib.dfft_rconv1d_long_length(-7) == lib.dfft_rconv1d_long_length(8193) == accepted[0]
    prev = 0
    for a in list(range(8000, 70000, 37)) + [1 << 20, (1 << 20) + 1, 3000001, (1 << 23) - 1, 1 << 23]:
        got = lib.dfft_rconv1d_long_length(a)
        want = next(v for v in accepted if v >= a)
        assert got == want >= prev, (a, got, want)              # accepted, >= a, no accepted m in between, monotone
        assert lib.dfft_rconv1d_long_length(got) == got         # idempotent
        prev = got
    for a in ((1 << 23) + 1, 1 << 24, 1 << 40):
        assert lib.dfft_rconv1d_long_length(a) == 0
    for m in accepted:
        n1, n2 = _split(m)
        assert n1 * n2 * 2 == m and n1 <= n2 <= 2048 and n1 in LC.FACTORS and n2 in LC.FACTORS, m
        assert (n1, n2) == LC.split(m), m                       # the most balanced pair
    for m, want in LC.SPLITS.items():
        assert _split(m) == want
    for m in (8192, 16386, 16385, 2 * 64 * 63, 2 * 4096 * 4096, 2 * 2048 * 4096, 0, -4, 2 * 49 * 256, 2 * 343 * 64):
        assert _split(m) is None, m
    assert lib.dfft_rconv1d_long_split(16384, None, None) == 1
    assert api.rconv1d_long_length(6000 + 6000 - 1) == lib.dfft_rconv1d_long_length(11999) == 12288


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_are_decided_before_the_device_is_queried():
    from distributedfft_amd import _lib as L
    lib = _lib()
    for dtype in (F64, F32):
        for kind in (CPLX, REAL):
            kw = dict(dtype=dtype, kind=kind)
            assert _call(inp=0, **kw)[0] == L.EINVAL                      # NULL pointers
            assert _call(out=0, **kw)[0] == L.EINVAL
            assert _call(hp=0, **kw)[0] == L.EINVAL
            for bad in (0, -3):                                           # sizes below 1
                assert _call(n=bad, **kw)[0] == L.EINVAL
                assert _call(m=bad, **kw)[0] == L.EINVAL
                assert _call(channels=bad, **kw)[0] == L.EINVAL
                assert _call(batch=bad, **kw)[0] == L.EINVAL
            assert _call(n=16385, m=16384, **kw)[0] == L.EINVAL           # m < n
            assert _call(n=20000, m=16386, **kw)[0] == L.EINVAL           # ... before m is judged
            rs = 8 if dtype == F64 else 4
            data = 9000 * 3 * 4 * rs
            assert _call(out=X + rs, **kw)[0] == L.EINVAL                 # in and out overlap partly, both orders
            assert _call(inp=X + rs, out=X, **kw)[0] == L.EINVAL
            assert _call(out=X + data - rs, **kw)[0] == L.EINVAL
            hb = 3 * 8193 * (rs if kind == REAL else 2 * rs)
            assert _call(hp=Y, **kw)[0] == L.EINVAL                       # hp overlaps out
            assert _call(hp=Y + data - rs, **kw)[0] == L.EINVAL
            assert _call(hp=Y - hb + rs, **kw)[0] == L.EINVAL
            for m in (8192, 128, 16385, 16386, 2 * 64 * 63, 2 * 343 * 64, (1 << 23) + 2, 1 << 30):
                rc, msg = _call(n=1, m=m, **kw)
                assert rc == L.EUNSUPPORTED and f"m = {m}" in msg, (m, rc, msg)
    for dtype in (-1, 2, 7):
        assert _call(dtype=dtype)[0] == L.EINVAL
    for kind in (-1, 2):
        assert _call(kind=kind)[0] == L.EINVAL
    # 2^31 rows or more
    assert _call(n=1, channels=1 << 16, batch=1 << 15)[0] == L.EUNSUPPORTED
    assert _call(n=1, channels=1 << 40, batch=1 << 40)[0] == L.EUNSUPPORTED
    # the filter permutation
    vp = C.c_void_p
    assert lib.dfft_rconv1d_long_filter(None, vp(Y), 16384, 3, F64, CPLX, None) == L.EINVAL
    assert lib.dfft_rconv1d_long_filter(vp(X), None, 16384, 3, F64, CPLX, None) == L.EINVAL
    assert lib.dfft_rconv1d_long_filter(vp(X), vp(Y), 16384, 0, F64, CPLX, None) == L.EINVAL
    assert lib.dfft_rconv1d_long_filter(vp(X), vp(Y), 16384, 3, 5, CPLX, None) == L.EINVAL
    assert lib.dfft_rconv1d_long_filter(vp(X), vp(Y), 16384, 3, F64, 2, None) == L.EINVAL
    assert lib.dfft_rconv1d_long_filter(vp(X), vp(X + 16), 16384, 3, F64, CPLX, None) == L.EINVAL      # hp overlaps h
    assert lib.dfft_rconv1d_long_filter(vp(X), vp(X), 16384, 3, F64, CPLX, None) == L.EINVAL
    assert lib.dfft_rconv1d_long_filter(vp(X), vp(Y), 8192, 3, F64, CPLX, None) == L.EUNSUPPORTED
    assert "m = 8192" in lib.dfft_last_error().decode()
    # dfft_rconv1d itself still stops at 8192
    assert lib.dfft_rconv1d(vp(X), vp(Y), vp(HP), 1, 16384, 3, 4, F64, CPLX, None) == L.EUNSUPPORTED
    assert lib.dfft_rconv1d_length(8193) == 0


def test_valid_calls_reach_the_device_query():
    from distributedfft_amd import _lib as L
    lib = _lib()
    if lib.dfft_device_count() > 0:
        return
    for m in LC.LENGTHS + [10240, 1 << 23]:
        for n in (m, m // 2 + 1, 5, 1):
            for dtype in (F64, F32):
                for kind in (CPLX, REAL):
                    assert _call(n=n, m=m, dtype=dtype, kind=kind, hp=1 << 44, out=1 << 42)[0] == L.ENOGPU, (m, n)
                    assert _call(inp=X, out=X, n=n, m=m, dtype=dtype, kind=kind, hp=1 << 44)[0] == L.ENOGPU    # exactly in place
    data = 9000 * 3 * 4 * 8
    hb = 3 * 8193 * 16
    assert _call(out=X + data)[0] == L.ENOGPU                       # ranges that merely touch do not overlap
    assert _call(hp=Y + data)[0] == L.ENOGPU
    assert _call(hp=Y - hb)[0] == L.ENOGPU
    assert _call(n=1, channels=(1 << 16) - 1, batch=1 << 15, hp=1 << 44, out=1 << 42)[0] == L.ENOGPU
    vp = C.c_void_p
    assert lib.dfft_rconv1d_long_filter(vp(X), vp(X + hb), 16384, 3, F64, CPLX, None) == L.ENOGPU
    assert lib.dfft_rconv1d_long_filter(vp(X), vp(X + hb // 4), 16384, 3, F32, REAL, None) == L.ENOGPU


# ---- route and scratch ------------------------------------------------------------------------------------------------------------------
def test_route_and_scratch_rules(monkeypatch):
    """Scratch of the three-launch route: chunk rows x m/2 complex, chunk = min(rows, max(256 MiB, one row's) / one row's) -- one chunk
    for small calls, several with a ragged last one; the figure does not depend on the filter kind (it is not an argument)."""
    lib = _lib()
    monkeypatch.delenv("DFFT_RCONV_LONG_FUSED", raising=False)

    def lease(m, rows, dtype):
        rb = (m // 2) * (16 if dtype == F64 else 8)
        return min(rows, max(256 << 20, rb) // rb) * rb

    for m in LC.LENGTHS + [10240, 1 << 21, 1 << 23]:
        n1, n2 = _split(m)
        for dtype in (F64, F32):
            assert lib.dfft_rconv1d_long_fused_applies(m, dtype) == int((n1, dtype) not in ROUTED and (n2, dtype) not in ROUTED)
            for channels, batch in ((1, 1), (3, 5), (16, 768), (3, 1 << 20)):
                got = lib.dfft_rconv1d_long_scratch_bytes(m // 2 + 1, m, channels, batch, dtype)
                assert got == lease(m, channels * batch, dtype), (m, dtype, channels, batch, got)
    # one chunk; several chunks with a ragged last one (2055 rows of 128 KiB: 2048 + 7)
    assert lib.dfft_rconv1d_long_scratch_bytes(8193, 16384, 3, 5, F64) == 15 * 8192 * 16
    assert lib.dfft_rconv1d_long_scratch_bytes(8193, 16384, 3, 685, F64) == 2048 * 8192 * 16 == 256 << 20
    assert 2055 % 2048 == 7
    assert lib.dfft_rconv1d_long_scratch_bytes(1, 1 << 23, 1, 9, F64) == 4 * (1 << 22) * 16
    # not a call the entry point would accept: no route, no lease
    assert lib.dfft_rconv1d_long_fused_applies(8192, F64) == 0
    assert lib.dfft_rconv1d_long_fused_applies(16384, 5) == 0
    assert lib.dfft_rconv1d_long_scratch_bytes(1, 8192, 1, 1, F64) == 0
    assert lib.dfft_rconv1d_long_scratch_bytes(16385, 16384, 1, 1, F64) == 0
    assert lib.dfft_rconv1d_long_scratch_bytes(1, 16384, 1 << 16, 1 << 15, F64) == 0
    assert lib.dfft_rconv1d_long_scratch_bytes(1, 16384, 1, 1, 3) == 0
    monkeypatch.setenv("DFFT_RCONV_LONG_FUSED", "0")
    assert lib.dfft_rconv1d_long_fused_applies(16384, F64) == 0
    monkeypatch.setenv("DFFT_RCONV_LONG_FUSED", "1")
    assert lib.dfft_rconv1d_long_fused_applies(16384, F64) == 1


# ---- build ------------------------------------------------------------------------------------------------------------------------------
def test_build_units():
    from distributedfft_amd import build
    from distributedfft_amd.build import NUM_INST_GROUPS
    names = [u[1].name for u in build.units()]
    assert [f"dfft_lconv_{g}.o" for g in range(NUM_INST_GROUPS + 1)] == [n for n in names if n.startswith("dfft_lconv_")]
    # every factor length has a tuned plan
    plans = {int(n) for n in re.findall(r"^\s*X\((\d+),", (CSRC / "dfft_plans.h").read_text(), re.M)}
    assert set(LC.FACTORS) <= plans


# ---- resource inventory -----------------------------------------------------------------------------------------------------------------
def test_inventory_belongs_to_the_sources_and_no_fused_kernel_spills():
    """profiles/2026-10-20_rconv1d_long/kernel_resources.txt (tools/fused_resources.py lconv) must carry the sha256 of the sources in the tree
    and list every instantiation the library routes fused -- factor length x fp64 / fp32 x (pass A, pass C: two-real / per-real accesses;
    Mid: complex / real filter), less the (N, type) lconv_fused_ok sends to the composed route, which it names -- with zero scratch."""
    text = FI.current_text("lconv")
    m = re.search(r"^# composed-route \(N, type\): (.*)$", text, re.M)
    assert m, "the inventory names the (N, type) lconv_fused_ok sends to the composed route"
    routed = {(int(n), F64 if t == "f64" else F32) for n, t in re.findall(r"\((\d+), (f64|f32)\)", m.group(1))}
    assert routed == ROUTED and len(routed) <= 6, "a few instantiations, not a way round the rule"
    variants = {"lconv_a": ("vec", "real"), "lconv_c": ("vec", "real"), "lconv_mid": ("complex", "real")}
    want = {(k, n, t, v) for k, vs in variants.items() for v in vs for n in LC.FACTORS for t in ("f64", "f32")
            if (n, F64 if t == "f64" else F32) not in routed and not (k == "lconv_mid" and n == 64)}   # 64 is never the longer factor
    fused = [ln for ln in text.splitlines() if ln.startswith(("lconv_a_kernel ", "lconv_c_kernel ", "lconv_mid_kernel "))]
    seen = set()
    for ln in fused:
        g = re.match(r"(lconv_a|lconv_c|lconv_mid)_kernel (f64|f32) N=(\d+) E=\d+ variant=(vec|real|complex) ", ln)
        assert g, ln
        seen.add((g.group(1), int(g.group(3)), g.group(2), g.group(4)))
    assert seen == want and len(fused) == len(want) == 6 * (len(LC.FACTORS) * 2 - len(routed)) - 4
    # the filter and multiply kernels of the unit, and the pad and truncate kernels of the common unit
    helpers = [ln for ln in text.splitlines() if ln.startswith(("lconv_filter_", "lconv_mul_"))] + FI.common_lines("pad_rows_", "trunc_rows_")
    assert len(helpers) == 11
    for ln in fused + helpers:
        assert re.search(r"scratch=(\d+)", ln).group(1) == "0", ln
    # the routed lengths are lengths the source names, and the library routes every split with one of them
    src = (CSRC / "dfft_lconv.hip").read_text()
    body = re.search(r"constexpr bool lconv_fused_ok\(int N, bool f64\) \{(.*?)\n\}", src, re.S).group(1)
    lib = _lib()
    for n, t in routed:
        assert re.search(rf"\b{n}\b", body), n
        assert lib.dfft_rconv1d_long_fused_applies(2 * n * 2048, t) == 0
        assert lib.dfft_rconv1d_long_fused_applies(2 * 64 * n, t) == 0
