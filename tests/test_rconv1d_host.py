"""Batched 1-D real FFT convolution (dfft_rconv1d), host side (no GPU): the four symbols, the refusals that are decided before the device
is queried, dfft_rconv1d_length, the route and scratch rules, a numpy model of the kernel's pairwise split / multiply / merge, the
cross-compilation of the dispatcher unit, the committed resource inventory of the fused kernels, and the CPU yardstick that the GPU
bound of tests/test_gpu_rconv1d.py is held against."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import accuracy_ref as A
import fused_inventory as FI
import rconv1d_cases as RC

try:
    import scipy.fft as sf
except ImportError:   # pragma: no cover
    sf = None

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "distributedfft_amd" / "csrc"
INVENTORY = ROOT / "profiles" / "2026-10-19_rconv1d" / "kernel_resources.txt"
SYMBOLS = ("dfft_rconv1d", "dfft_rconv1d_fused_applies", "dfft_rconv1d_scratch_bytes", "dfft_rconv1d_length")
X, Y, HP = 0x10000000, 0x20000000, 0x30000000
F64, F32, CPLX, REAL = 0, 1, 0, 1
# (M, dtype) that tools/fused_resources.py rconv found spilling: the composed route (rconv_fused_ok of dfft_rconv.hip)
ROUTED = {(3125, F64), (3125, F32), (1536, F64)}


def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


def _tuned():
    return sorted(RC.plan_points())


def _call(inp=X, out=Y, h=HP, n=64, m=128, channels=3, batch=4, dtype=F64, kind=CPLX):
    lib = _lib()
    vp = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    rc = lib.dfft_rconv1d(vp(inp), vp(out), vp(h), n, m, channels, batch, dtype, kind, None)
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
    assert L.SIGNATURES["dfft_rconv1d"][1] == [C.c_void_p] * 3 + [C.c_longlong] * 4 + [C.c_int, C.c_int, C.c_void_p]
    assert L.SIGNATURES["dfft_rconv1d_length"] == (C.c_longlong, [C.c_longlong])
    assert L.SIGNATURES["dfft_rconv1d_scratch_bytes"][0] == C.c_ulonglong
    assert "overlap-save" in header and "DFFT_RCONV_FUSED" in header


def test_refusals_are_decided_before_the_device_is_queried():
    from distributedfft_amd import _lib as L
    for dtype in (F64, F32):
        for kind in (CPLX, REAL):
            kw = dict(dtype=dtype, kind=kind)
            assert _call(inp=0, **kw)[0] == L.EINVAL                      # NULL pointers
            assert _call(out=0, **kw)[0] == L.EINVAL
            assert _call(h=0, **kw)[0] == L.EINVAL
            for bad in (0, -3):                                           # sizes below 1
                assert _call(n=bad, **kw)[0] == L.EINVAL
                assert _call(m=bad, **kw)[0] == L.EINVAL
                assert _call(channels=bad, **kw)[0] == L.EINVAL
                assert _call(batch=bad, **kw)[0] == L.EINVAL
            assert _call(n=130, m=128, **kw)[0] == L.EINVAL               # m < n
            assert _call(n=200, m=194, **kw)[0] == L.EINVAL               # ... before m is judged
            rs = 8 if dtype == F64 else 4
            data = 64 * 3 * 4 * rs
            assert _call(out=X + rs, **kw)[0] == L.EINVAL                 # in and out overlap partly, both orders
            assert _call(inp=X + rs, out=X, **kw)[0] == L.EINVAL
            assert _call(out=X + data - rs, **kw)[0] == L.EINVAL
            hb = 3 * 65 * (rs if kind == REAL else 2 * rs)
            assert _call(h=Y, **kw)[0] == L.EINVAL                        # h overlaps out
            assert _call(h=Y + data - rs, **kw)[0] == L.EINVAL
            assert _call(h=Y - hb + rs, **kw)[0] == L.EINVAL
            for m in (9, 194, 22, 2, 8194, 16384, 2 * 4099, 1 << 30):    # odd, Bluestein half, 11 | m/2, m/2 = 1, above 8192
                rc, msg = _call(n=1, m=m, **kw)
                assert rc == L.EUNSUPPORTED and f"m = {m}" in msg, (m, rc, msg)
                assert _lib().dfft_real_form(m) != 1
    for dtype in (-1, 2, 7):
        assert _call(dtype=dtype)[0] == L.EINVAL
    for kind in (-1, 2):
        assert _call(kind=kind)[0] == L.EINVAL
    # 2^31 rows or more
    assert _call(n=1, m=4, channels=1 << 16, batch=1 << 15)[0] == L.EUNSUPPORTED
    assert _call(n=1, m=4, channels=1 << 40, batch=1 << 40)[0] == L.EUNSUPPORTED


def test_valid_calls_reach_the_device_query():
    from distributedfft_amd import _lib as L
    if _lib().dfft_device_count() > 0:
        return
    for M in RC.HALVES + [3125, 1536]:
        for n in RC.n_values(2 * M):
            for dtype in (F64, F32):
                for kind in (CPLX, REAL):
                    assert _call(n=n, m=2 * M, dtype=dtype, kind=kind, h=1 << 44)[0] == L.ENOGPU, (M, n)
                    assert _call(inp=X, out=X, n=n, m=2 * M, dtype=dtype, kind=kind, h=1 << 44)[0] == L.ENOGPU    # exactly in place
    # ranges that merely touch do not overlap: 4 x 3 rows of 64 doubles = 6144 bytes; 3 x 65 complex doubles = 3120 bytes
    assert _call(out=X + 6144)[0] == L.ENOGPU
    assert _call(h=Y + 6144)[0] == L.ENOGPU
    assert _call(h=Y - 3120)[0] == L.ENOGPU
    assert _call(n=1, m=4, channels=(1 << 16) - 1, batch=1 << 15, h=1 << 44, out=1 << 42)[0] == L.ENOGPU


def test_rconv1d_length():
    lib = _lib()
    accepted = [m for m in range(1, 8193) if lib.dfft_real_form(m) == 1]
    assert accepted[0] == 4 and accepted[-1] == 8192
    want, it = {}, iter(accepted)
    cur = next(it)
    for a in range(1, 8193):
        while cur < a:
            cur = next(it)
        want[a] = cur
    for a in range(1, 8193):
        got = lib.dfft_rconv1d_length(a)
        assert got == want[a], (a, got, want[a])      # accepted, >= a, and no accepted m in between
    for a in (8193, 8194, 10000, 1 << 20, 1 << 40):
        assert lib.dfft_rconv1d_length(a) == 0
    for a in (0, -5):
        assert lib.dfft_rconv1d_length(a) == 4
    from distributedfft_amd import api
    assert api.rconv1d_length(4096 + 7 - 1) == lib.dfft_rconv1d_length(4102) == 4116


def test_route_and_scratch_rules(monkeypatch):
    """Fused: m/2 tuned and not in the routed list, whatever n, the filter kind and vec; 0 under DFFT_RCONV_FUSED=0 (read per call).
    Scratch: 0 for the fused route, else chunk rows x (m reals + (m/2 + 1) complex), chunk = min(rows, max(256 MiB, one row's) / one row's)."""
    lib = _lib()
    monkeypatch.delenv("DFFT_RCONV_FUSED", raising=False)
    tuned = set(_tuned())

    def lease(m, rows, dtype):
        cs = 16 if dtype == F64 else 8
        rb = m * cs // 2 + (m // 2 + 1) * cs
        return min(rows, max(256 << 20, rb) // rb) * rb

    halves = sorted(tuned | {36, 6, 18, 3600, 2000, 4000})
    for M in halves:
        m = 2 * M
        assert lib.dfft_real_form(m) == 1, m
        for dtype in (F64, F32):
            fused = M in tuned and (M, dtype) not in ROUTED
            for kind in (CPLX, REAL):
                for vec in (0, 1):
                    for n in (1, M, m):
                        assert lib.dfft_rconv1d_fused_applies(n, m, dtype, kind, vec) == int(fused), (M, dtype, kind, vec, n)
            for channels, batch in ((1, 1), (3, 5), (16, 768), (3, 1 << 20)):
                got = lib.dfft_rconv1d_scratch_bytes(M, m, channels, batch, dtype)
                assert got == (0 if fused else lease(m, channels * batch, dtype)), (M, dtype, channels, batch, got)
    # not a call the entry point would accept: no route, no lease
    assert lib.dfft_rconv1d_fused_applies(130, 128, F64, CPLX, 1) == 0
    assert lib.dfft_rconv1d_fused_applies(64, 128, 5, CPLX, 1) == 0
    assert lib.dfft_rconv1d_fused_applies(64, 128, F64, 3, 1) == 0
    assert lib.dfft_rconv1d_fused_applies(1, 22, F64, CPLX, 0) == 0
    assert lib.dfft_rconv1d_scratch_bytes(1, 22, 1, 1, F64) == 0
    assert lib.dfft_rconv1d_scratch_bytes(130, 128, 1, 1, F64) == 0
    assert lib.dfft_rconv1d_scratch_bytes(1, 4, 1 << 16, 1 << 15, F64) == 0
    # more than one chunk: 8192-point rows of 64 KiB + 64 KiB + 16 bytes
    assert lib.dfft_rconv1d_scratch_bytes(4096, 8192, 1, 100000, F64) == 0
    monkeypatch.setenv("DFFT_RCONV_FUSED", "0")
    assert lib.dfft_rconv1d_fused_applies(64, 128, F64, CPLX, 1) == 0
    assert lib.dfft_rconv1d_scratch_bytes(4096, 8192, 1, 100000, F64) == lease(8192, 100000, F64) == 2047 * (65536 + 65552)
    assert lib.dfft_rconv1d_scratch_bytes(64, 128, 3, 5, F32) == 15 * (128 * 4 + 65 * 8)
    monkeypatch.setenv("DFFT_RCONV_FUSED", "1")
    assert lib.dfft_rconv1d_fused_applies(64, 128, F64, CPLX, 1) == 1


# ---- numpy model of the kernel ----------------------------------------------------------------------------------------------------------
def kernel_model(x, H, m):
    """One row as rconv_rows_kernel computes it: the thread that holds Z[k] reads Z[(M - k) mod M], forms X[k] and X[M-k], multiplies
    them by H[k] / m and H[M-k] / m (imaginary parts of the products dropped at k = 0) and merges them into Z'[k]; the inverse runs as
    conj . forward . conj."""
    M, n = m // 2, x.shape[-1]
    xp = np.zeros(m)
    xp[:n] = x
    Z = np.fft.fft(xp[0::2] + 1j * xp[1::2])
    W = np.exp(-2j * np.pi * np.arange(M) / m)
    sc = 0.5 / m
    Zp = np.empty(M, dtype=complex)
    for k in range(M):                      # one iteration = one (thread, point)
        zk, zm, w = Z[k], Z[(M - k) % M], W[k]
        xe = zk + np.conj(zm)               # 2 Xe[k]
        xo = -1j * (zk - np.conj(zm))       # 2 Xo[k]
        t = xo * w
        ya = (xe + t) * (H[k] * sc)
        yb = np.conj(xe - t) * (H[M - k] * sc)
        if k == 0:
            ya, yb = ya.real + 0j, yb.real + 0j
        Zp[k] = np.conj((ya + np.conj(yb)) + 1j * (ya - np.conj(yb)) * np.conj(w))
    z = np.conj(np.fft.fft(Zp))
    y = np.empty(m)
    y[0::2], y[1::2] = z.real, z.imag
    return y[:n]


@pytest.mark.parametrize("kind", RC.KINDS)
@pytest.mark.parametrize("M", [2, 3, 4, 5, 8, 9, 16, 25, 48, 125, 128])
def test_kernel_model_matches_numpy(M, kind):
    """Checks the identity on a numpy restatement of the kernel -- even and odd M, k = 0 and the self-paired k = M/2 included, real and
    complex H.  Not library code: tests/test_gpu_rconv1d.py runs the kernels."""
    m = 2 * M
    rng = np.random.default_rng(M * 3 + (kind == "complex"))
    H = RC.make_filter(1, m, kind, M)[0]
    for n in RC.n_values(m) + [m - 1, 3]:
        if not 1 <= n <= m:
            continue
        x = rng.standard_normal(n)
        want = np.fft.irfft(np.fft.rfft(x, m) * H, m)[:n]
        got = kernel_model(x, H, m)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (M, n, kind)
    # H == 1: the identity
    x = rng.standard_normal(m)
    assert np.abs(kernel_model(x, np.ones(M + 1), m) - x).max() <= 1e-12 * np.abs(x).max()


def test_reference_is_numpy_irfft_of_rfft():
    for M, n, channels, kind in ((8, 15, 3, "complex"), (25, 25, 1, "real"), (36, 72, 3, "complex")):
        x, H, ref = RC.case(M, n, channels, 2, kind)
        want = np.fft.irfft(np.fft.rfft(x, 2 * M, axis=1) * H[np.arange(x.shape[0]) % channels], 2 * M, axis=1)[:, :n]
        assert np.abs(ref.astype(np.float64) - want).max() <= 1e-13 * np.abs(want).max()
    # taps: rfft of the zero-padded taps as H gives numpy.convolve
    rng = np.random.default_rng(3)
    x, k = rng.standard_normal((1, 100)), rng.standard_normal(7)
    H = np.fft.rfft(k, 108)[None, :]
    assert np.abs(RC.reference(x, H, 108)[0].astype(np.float64) - np.convolve(x[0], k)[:100]).max() < 1e-12


# ---- build ------------------------------------------------------------------------------------------------------------------------------
def test_dispatcher_unit_cross_compiles(tmp_path):
    """The dispatcher unit of dfft_rconv.hip (composed-route kernels and host code) builds for gfx950; build() compiles every group."""
    from distributedfft_amd.build import NUM_INST_GROUPS
    obj = tmp_path / "dfft_rconv_dispatch.o"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}", f"-I{CSRC}",
                        f"-DDFFT_INST_GROUP={NUM_INST_GROUPS}", "-c", str(CSRC / "dfft_rconv.hip"), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert obj.stat().st_size > 0
    from distributedfft_amd import build
    names = [u[1].name for u in build.units()]
    assert [f"dfft_rconv_{g}.o" for g in range(NUM_INST_GROUPS + 1)] == [n for n in names if n.startswith("dfft_rconv_")]


# ---- resource inventory -----------------------------------------------------------------------------------------------------------------
def test_inventory_belongs_to_the_sources_and_no_fused_kernel_spills():
    """profiles/2026-10-19_rconv1d/kernel_resources.txt (tools/fused_resources.py rconv) must carry the sha256 of the sources in the tree and
    list every fused instantiation -- tuned M x fp64 / fp32 x complex / real filter x two-real / per-real accesses, less the ones
    rconv_fused_ok sends to the composed route, which it names -- with zero scratch."""
    text = FI.current_text("rconv")
    fused = [ln for ln in text.splitlines() if ln.startswith("rconv_rows_kernel ")]
    m = re.search(r"^# composed-route \(M, type, filter, form\): (.*)$", text, re.M)
    assert m, "the inventory names the instantiations rconv_fused_ok sends to the composed route"
    routed = {(int(n), t, f, a) for n, t, f, a in re.findall(r"\((\d+), (f64|f32), (complex|real), (vec|real)\)", m.group(1))}
    assert {(n, F64 if t == "f64" else F32) for n, t, _, _ in routed} == ROUTED
    assert len(routed) == 4 * len(ROUTED) <= 16, "a few instantiations, not a way round the rule"
    want = {(n, t, f, a) for n in _tuned() for t in ("f64", "f32") for f in ("complex", "real") for a in ("vec", "real")} - routed
    seen = set()
    for ln in fused:
        g = re.match(r"rconv_rows_kernel (f64|f32) M=(\d+) E=\d+ filter=(complex|real) form=(vec|real) ", ln)
        assert g, ln
        seen.add((int(g.group(2)), g.group(1), g.group(3), g.group(4)))
    assert seen == want
    assert len(fused) == len(want)
    # the multiply kernel of the unit, and the pad and truncate kernels of the common unit
    helpers = [ln for ln in text.splitlines() if ln.startswith("rconv_mul_")] + FI.common_lines("pad_rows_", "trunc_rows_")
    assert len(helpers) == 8
    for ln in fused + helpers:
        assert re.search(r"scratch=(\d+)", ln).group(1) == "0", ln
    # the routed lengths are lengths the source names, and the library routes them
    src = (CSRC / "dfft_rconv.hip").read_text()
    body = re.search(r"constexpr bool rconv_fused_ok\(int M, bool f64\) \{(.*?)\n\}", src, re.S).group(1)
    lib = _lib()
    for n, t, _, _ in routed:
        assert re.search(rf"\b{n}\b", body), n
        assert lib.dfft_rconv1d_fused_applies(1, 2 * n, F64 if t == "f64" else F32, CPLX, 1) == 0


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------------
_MEASURED = {}


def _yardstick():
    """The same-precision CPU FFT pipeline (scipy.fft, as tests/test_accuracy_host.py; numpy for fp64 where scipy is missing) on exactly
    the cases of tests/test_gpu_rconv1d.py: worst nu per precision."""
    if _MEASURED:
        return _MEASURED
    precs = A.PRECS if sf is not None else ("f64",)
    mod = sf if sf is not None else np.fft
    for M, n, channels, batch, kind in RC.all_cases():
        x, H, ref = RC.case(M, n, channels, batch, kind)
        m = 2 * M
        for prec in precs:
            Hp = H.astype(A.RDT[prec] if kind == "real" else A.CDT[prec])[np.arange(x.shape[0]) % channels]
            got = mod.irfft(mod.rfft(x.astype(A.RDT[prec]), m, axis=1) * Hp, m, axis=1)[:, :n]
            assert got.dtype == A.RDT[prec] or sf is None
            v = RC.nu_rows(got, ref, m, prec)
            if v > _MEASURED.get(prec, (-1.0, ""))[0]:
                _MEASURED[prec] = (v, f"M={M} n={n} channels={channels} {kind}")
    return _MEASURED


@pytest.mark.parametrize("prec", A.PRECS)
def test_gpu_bound_is_at_most_eight_times_the_cpu_yardstick(prec):
    if prec == "f32" and sf is None:
        pytest.skip("the fp32 yardstick needs scipy.fft: numpy computes float32 transforms in double")
    from test_gpu_rconv1d import BOUND
    value, what = _yardstick()[prec]
    print(f"yardstick rconv1d {prec}: {value:.3f}  ({what})")
    assert 0 < BOUND[prec] <= 8 * value, (prec, BOUND[prec], value, what)
