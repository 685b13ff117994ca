"""Batched 1-D real cross-spectrum (dfft_rxspec1d), host side (no GPU): the four symbols, the refusals that are decided before the device
is queried, the slice rule against a brute-force restatement, the route and scratch rules, a numpy model of the kernel's arithmetic
(pairing from Z, DC and Nyquist bins, per-slice accumulation, in-order reduction), the gradient formulas of api.rconv1d / api.fftconv1d
against torch's CPU autograd, the cross-compilation of the dispatcher unit, the committed resource inventory of the fused kernels, and
the CPU yardstick that the GPU bound of tests/test_gpu_rxspec1d.py is held against."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import accuracy_ref as A
import fused_inventory as FI
import rconv1d_cases as RC
import rxspec1d_cases as XC

try:
    import scipy.fft as sf
except ImportError:   # pragma: no cover
    sf = None

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "distributedfft_amd" / "csrc"
INVENTORY = ROOT / "profiles" / "2026-10-20_rxspec1d" / "kernel_resources.txt"
SYMBOLS = ("dfft_rxspec1d", "dfft_rxspec1d_fused_applies", "dfft_rxspec1d_scratch_bytes", "dfft_rxspec1d_slices")
X, G, OUT = 0x10000000, 0x20000000, 0x30000000
F64, F32 = 0, 1
CODE = {"f64": F64, "f32": F32}


def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


def _call(x=X, g=G, out=OUT, n=64, m=128, channels=3, batch=4, dtype=F64):
    lib = _lib()
    vp = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    rc = lib.dfft_rxspec1d(vp(x), vp(g), vp(out), n, m, channels, batch, dtype, None)
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
    assert L.SIGNATURES["dfft_rxspec1d"] == (C.c_int, [C.c_void_p] * 3 + [C.c_longlong] * 4 + [C.c_int, C.c_void_p])
    assert L.SIGNATURES["dfft_rxspec1d_fused_applies"] == (C.c_int, [C.c_longlong, C.c_longlong, C.c_int, C.c_int])
    assert L.SIGNATURES["dfft_rxspec1d_scratch_bytes"] == (C.c_ulonglong, [C.c_longlong] * 4 + [C.c_int])
    assert L.SIGNATURES["dfft_rxspec1d_slices"] == (C.c_longlong, [C.c_longlong] * 3 + [C.c_int])
    assert "DFFT_RXSPEC_FUSED" in header


def test_refusals_are_decided_before_the_device_is_queried():
    from distributedfft_amd import _lib as L
    for dtype in (F64, F32):
        kw = dict(dtype=dtype)
        assert _call(x=0, **kw)[0] == L.EINVAL                        # NULL pointers
        assert _call(g=0, **kw)[0] == L.EINVAL
        assert _call(out=0, **kw)[0] == L.EINVAL
        for bad in (0, -3):                                           # sizes below 1
            assert _call(n=bad, **kw)[0] == L.EINVAL
            assert _call(m=bad, **kw)[0] == L.EINVAL
            assert _call(channels=bad, **kw)[0] == L.EINVAL
            assert _call(batch=bad, **kw)[0] == L.EINVAL
        assert _call(n=130, m=128, **kw)[0] == L.EINVAL               # m < n
        assert _call(n=200, m=194, **kw)[0] == L.EINVAL               # ... before m is judged
        rs = 8 if dtype == F64 else 4
        data, ob = 64 * 3 * 4 * rs, 3 * 65 * 2 * rs
        assert _call(out=X, **kw)[0] == L.EINVAL                      # out overlaps x, either end
        assert _call(out=X + data - rs, **kw)[0] == L.EINVAL
        assert _call(out=X - ob + rs, **kw)[0] == L.EINVAL
        assert _call(out=G, **kw)[0] == L.EINVAL                      # out overlaps g
        assert _call(out=G + data - rs, **kw)[0] == L.EINVAL
        assert _call(out=G - ob + rs, **kw)[0] == L.EINVAL
        assert _call(g=X, out=X + rs, **kw)[0] == L.EINVAL            # ... also for the auto-spectrum
        for m in (9, 194, 22, 2, 8194, 16384, 2 * 4099, 1 << 30):    # odd, Bluestein half, 11 | m/2, m/2 = 1, above 8192
            rc, msg = _call(n=1, m=m, **kw)
            assert rc == L.EUNSUPPORTED and f"m = {m}" in msg, (m, rc, msg)
            assert _lib().dfft_real_form(m) != 1
    for dtype in (-1, 2, 7):
        assert _call(dtype=dtype)[0] == L.EINVAL
    assert _call(n=1, m=4, channels=1 << 16, batch=1 << 15)[0] == L.EUNSUPPORTED   # 2^31 rows or more
    assert _call(n=1, m=4, channels=1 << 40, batch=1 << 40)[0] == L.EUNSUPPORTED


def test_valid_calls_reach_the_device_query():
    from distributedfft_amd import _lib as L
    if _lib().dfft_device_count() > 0:
        return
    for M in XC.HALVES + [3125, 1536, 1280]:
        for n in XC.n_values(2 * M):
            for dtype in (F64, F32):
                assert _call(n=n, m=2 * M, dtype=dtype, out=1 << 44)[0] == L.ENOGPU, (M, n)
                assert _call(g=X, n=n, m=2 * M, dtype=dtype, out=1 << 44)[0] == L.ENOGPU     # g is x: the auto-spectrum
    # ranges that merely touch do not overlap: 4 x 3 rows of 64 doubles = 6144 bytes; 3 x 65 complex doubles = 3120 bytes
    assert _call(out=X + 6144)[0] == L.ENOGPU
    assert _call(out=G - 3120)[0] == L.ENOGPU
    assert _call(g=X + 8, out=OUT)[0] == L.ENOGPU                    # x and g may overlap: neither is written
    assert _call(n=1, m=4, channels=(1 << 16) - 1, batch=1 << 15, out=1 << 44)[0] == L.ENOGPU


# ---- slices, route, scratch -------------------------------------------------------------------------------------------------------------
def test_slices_match_the_rule_and_cover_the_batch_once():
    """slices = max(1, min(target / channels, batch / 8)), target = 512 * min(G, 8) with G the thread groups per workgroup of the
    m/2-point kernel (1 for an untuned m/2) -- whatever the precision and the environment; the ranges are contiguous and cover the batch."""
    lib = _lib()
    for M in sorted(set(RC.plan_points()) | {36, 6, 18, 3600}):
        G = RC.rows_per_group(M)
        target = 512 * min(G, 8)
        for channels in (1, 2, 3, 16, 511, 512, 513, 4096, 5000):
            for batch in (1, 7, 8, 15, 16, 17, 100, 4096, 32768, 32775, 40000, 1 << 20):
                if channels * batch >= 1 << 31:      # a call that is refused
                    assert lib.dfft_rxspec1d_slices(2 * M, channels, batch, F64) == 0
                    continue
                want = 1
                for s in range(1, target + 1):       # brute force: the most slices with s * channels <= target and 8 s <= batch
                    if s * channels > target or XC.MIN_ROWS * s > batch:
                        break
                    want = s
                for dtype in (F64, F32):
                    got = lib.dfft_rxspec1d_slices(2 * M, channels, batch, dtype)
                    assert got == want == XC.slices_rule(M, channels, batch), (M, channels, batch, got, want)
                ranges = XC.slice_ranges(batch, want)
                assert ranges[0][0] == 0 and sum(r for _, r in ranges) == batch
                assert all(a + r == b for (a, r), (b, _) in zip(ranges, ranges[1:]))
                assert max(r for _, r in ranges) - min(r for _, r in ranges) <= 1 and (want == 1 or ranges[-1][1] >= XC.MIN_ROWS)
    for args in ((22, 1, 1, F64), (9, 1, 1, F64), (8194, 1, 1, F64), (128, 0, 1, F64), (128, 1, 0, F64), (128, 1, 1, 5), (4, 1 << 16, 1 << 15, F64)):
        assert lib.dfft_rxspec1d_slices(*args) == 0, args
    # the batches of the sweep do what they are chosen for
    for M in sorted(set(XC.HALVES) | set(RC.plan_points())):
        for channels in XC.CHANNELS + (2,):
            one, many = XC.batches(M, channels)
            s = XC.slices_rule(M, channels, many)
            assert one == 1 and XC.slices_rule(M, channels, 1) == 1 and s >= 2 and many % s and many < 64
            G = RC.rows_per_group(M)
            assert G == 1 or (channels * s) % G or channels % G == 0, (M, channels)
            assert M not in XC.HALVES or channels == 2 or G == 1 or (channels * s) % G, "the sweep's own cases do leave a ragged workgroup"
    M, n, channels, batch = XC.BEYOND_TARGET
    s = XC.slices_rule(M, channels, batch)
    assert s == 512 * 8 // channels < batch // XC.MIN_ROWS and batch % s and batch // s >= 16


def test_route_and_scratch_rules(monkeypatch):
    """Fused: m/2 tuned and not in the routed list, whatever n and vec; 0 under DFFT_RXSPEC_FUSED=0 (read per call).  Scratch: the
    partial sums of the slices (0 for one slice) on the fused route, else chunk rows x (m reals + 2 (m/2 + 1) complex)."""
    lib = _lib()
    monkeypatch.delenv("DFFT_RXSPEC_FUSED", raising=False)
    tuned = set(RC.plan_points())

    def lease(m, rows, dtype):
        cs = 16 if dtype == F64 else 8
        rb = m * cs // 2 + 2 * (m // 2 + 1) * cs
        return min(rows, max(256 << 20, rb) // rb) * rb

    for M in sorted(tuned | {36, 6, 18, 3600}):
        m = 2 * M
        for prec, dtype in CODE.items():
            fused = XC.fused(M, prec)
            assert fused == (M in tuned and (M, prec) not in XC.ROUTED)
            for vec in (0, 1):
                for n in (1, M, m):
                    assert lib.dfft_rxspec1d_fused_applies(n, m, dtype, vec) == int(fused), (M, prec, vec, n)
            for channels, batch in ((1, 1), (3, 5), (3, 19), (16, 4096)):
                got = lib.dfft_rxspec1d_scratch_bytes(M, m, channels, batch, dtype)
                s = XC.slices_rule(M, channels, batch)
                want = (s * channels * (M + 1) * (16 if dtype == F64 else 8) if s > 1 else 0) if fused else lease(m, channels * batch, dtype)
                assert got == want, (M, prec, channels, batch, got, want)
    assert lib.dfft_rxspec1d_fused_applies(130, 128, F64, 1) == 0
    assert lib.dfft_rxspec1d_fused_applies(64, 128, 5, 1) == 0
    assert lib.dfft_rxspec1d_fused_applies(1, 22, F64, 0) == 0
    assert lib.dfft_rxspec1d_scratch_bytes(1, 22, 1, 1, F64) == 0
    assert lib.dfft_rxspec1d_scratch_bytes(130, 128, 1, 1, F64) == 0
    assert lib.dfft_rxspec1d_scratch_bytes(1, 4, 1 << 16, 1 << 15, F64) == 0
    monkeypatch.setenv("DFFT_RXSPEC_FUSED", "0")
    assert lib.dfft_rxspec1d_fused_applies(64, 128, F64, 1) == 0
    assert lib.dfft_rxspec1d_scratch_bytes(64, 128, 3, 5, F32) == 15 * (128 * 4 + 2 * 65 * 8)
    assert lib.dfft_rxspec1d_slices(128, 3, 19, F64) == 2            # the slice count does not depend on the route
    monkeypatch.setenv("DFFT_RXSPEC_FUSED", "1")
    assert lib.dfft_rxspec1d_fused_applies(64, 128, F64, 1) == 1


# ---- numpy model of the kernel ----------------------------------------------------------------------------------------------------------
def _bins_model(row, m):
    """2 X[k], k = 0 ... M, of one row as rxspec_rows_kernel forms them: the thread that holds Z[k] reads Z[(M - k) mod M]; bin M comes
    from Z[0] alone."""
    M, n = m // 2, row.shape[-1]
    xp = np.zeros(m)
    xp[:n] = row
    Z = np.fft.fft(xp[0::2] + 1j * xp[1::2])
    W = np.exp(-2j * np.pi * np.arange(M) / m)
    out = np.empty(M + 1, dtype=complex)
    for k in range(M):
        zk, zm = Z[k], Z[(M - k) % M]
        xe = zk + np.conj(zm)
        xo = -1j * (zk - np.conj(zm))
        out[k] = xe + xo * W[k]
        if k == 0:
            out[M] = xe.real - xo.real
    return out


def kernel_model(x, g, m, channels, slices):
    """The whole call: per (slice, channel) item the products of the rows of the slice in row order, times 1/4, imaginary parts of bins 0
    and M zero; then the slices in order."""
    batch = x.shape[0] // channels
    M = m // 2
    partial = np.zeros((slices, channels, M + 1), dtype=complex)
    for s, (b0, count) in enumerate(XC.slice_ranges(batch, slices)):
        for c in range(channels):
            acc = np.zeros(M + 1, dtype=complex)
            for b in range(b0, b0 + count):
                acc += np.conj(_bins_model(x[b * channels + c], m)) * _bins_model(g[b * channels + c], m)
            acc *= 0.25
            acc[0], acc[M] = acc[0].real, acc[M].real
            partial[s, c] = acc
    out = partial[0].copy()
    for s in range(1, slices):
        out += partial[s]
    return out


@pytest.mark.parametrize("M", [2, 3, 4, 5, 8, 9, 16, 25, 48, 125])
def test_kernel_model_matches_the_longdouble_reference(M):
    """Even and odd M, k = 0, the self-paired k = M/2 and the Nyquist bin, one and several slices with a ragged last one.  Not library
    code: tests/test_gpu_rxspec1d.py runs the kernels."""
    m = 2 * M
    for channels, batch, slices in ((1, 1, 1), (3, 19, 2), (2, 11, 3)):
        for n in XC.n_values(m) + [m - 1, 3]:
            if not 1 <= n <= m:
                continue
            x = A.rand_real((batch * channels, n), 500 + M + n)
            g = A.rand_real((batch * channels, n), 900 + M + n)
            ref = XC.reference(x, g, m, channels)
            got = kernel_model(x, g, m, channels, slices)
            # The sum over the batch cancels (worst for n = 1, where every bin is the one number sum_b x[b] g[b]), and the rounding error
            # of a sum scales with the sum of the moduli of its terms: the model is held to nu <= 8 relative to that sum, line by line.
            moduli = (np.abs(np.fft.rfft(x, m, axis=1)) * np.abs(np.fft.rfft(g, m, axis=1))).reshape(batch, channels, M + 1).sum(0)
            err = np.sqrt((np.abs(got - ref).astype(np.float64) ** 2).sum(1)) / np.sqrt((moduli ** 2).sum(1))
            assert err.max() <= 8 * A.EPS["f64"] * np.sqrt(np.log2(m)), (M, n, channels, batch, err.max() / A.EPS["f64"])
            assert np.all(got[:, 0].imag == 0) and np.all(got[:, M].imag == 0)
            auto = kernel_model(x, x, m, channels, slices)
            assert XC.nu_lines(auto, XC.reference(x, x, m, channels), m, "f64") <= 8.0 and np.all(auto.real >= 0)   # (no cancellation)


def test_reference_is_numpy_rfft_and_no_line_is_zero():
    for M, n, channels, batch in ((8, 15, 3, 5), (25, 25, 1, 3), (36, 72, 3, 2)):
        x, g, ref, auto = XC.case(M, n, channels, batch)
        X_ = np.fft.rfft(x, 2 * M, axis=1).reshape(batch, channels, M + 1)
        G_ = np.fft.rfft(g, 2 * M, axis=1).reshape(batch, channels, M + 1)
        want = (np.conj(X_) * G_).sum(0)
        assert np.abs(ref.astype(np.complex128) - want).max() <= 1e-12 * np.abs(want).max()
        assert np.abs(auto.astype(np.complex128) - (np.abs(X_) ** 2).sum(0)).max() <= 1e-12 * np.abs(want).max()
    for M, n, channels, batch in XC.all_cases():
        if M <= 64 or n == 1:
            x, g, ref, auto = XC.case(M, n, channels, batch)
            for r in (ref, auto):
                assert np.all(np.sum(r.real ** 2 + r.imag ** 2, axis=1) > 0), (M, n, channels, batch)


# ---- the gradient formulas --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,n", [(8, 7), (25, 24), (36, 72)])
def test_gradient_formulas_match_torch_cpu_autograd(M, n):
    """grad_x = rconv1d(g, conj H), grad_H = w / m * S (its real part for a real H), grad_k = irfft(S)[:taps] with S the cross-spectrum of
    x and g -- against torch's autograd of irfft(rfft(x, m) * H, m)[..., :n] in float64, all on the CPU."""
    import torch
    m, channels, batch, taps = 2 * M, 3, 4, 5
    gen = torch.Generator().manual_seed(M)
    x = torch.randn(batch, channels, n, dtype=torch.float64, generator=gen)
    g = torch.randn(batch, channels, n, dtype=torch.float64, generator=gen)
    S = torch.from_numpy(XC.reference(x.reshape(-1, n).numpy(), g.reshape(-1, n).numpy(), m, channels).astype(np.complex128))
    w = torch.full((M + 1,), 2.0 / m, dtype=torch.float64)
    w[0] = w[-1] = 1.0 / m

    def conv(x, H):
        return torch.fft.irfft(torch.fft.rfft(x, m) * H, m)[..., :n]

    for real in (False, True):
        H = torch.randn(channels, M + 1, dtype=torch.float64 if real else torch.complex128, generator=gen)
        xa, Ha = x.clone().requires_grad_(True), H.clone().requires_grad_(True)
        conv(xa, Ha).backward(g)
        assert (xa.grad - conv(g, H.conj())).abs().max() <= 1e-13 * xa.grad.abs().max()
        want = (S.real if real else S) * w
        assert (Ha.grad - want).abs().max() <= 1e-13 * want.abs().max(), ("grad_H", real)
    k = torch.randn(channels, taps, dtype=torch.float64, generator=gen, requires_grad=True)
    if n + taps - 1 <= m:
        xa = x.clone().requires_grad_(True)
        kp = torch.nn.functional.pad(k, (0, m - taps))
        conv(xa, torch.fft.rfft(kp)).backward(g)
        want = torch.fft.irfft(S, m)[:, :taps]
        assert (k.grad - want).abs().max() <= 1e-13 * want.abs().max()


# ---- build ------------------------------------------------------------------------------------------------------------------------------
def test_dispatcher_unit_cross_compiles(tmp_path):
    """The dispatcher unit of dfft_xspec.hip (reduction, composed-route kernels and host code) builds for gfx950; build() compiles every
    group."""
    from distributedfft_amd.build import NUM_INST_GROUPS
    obj = tmp_path / "dfft_xspec_dispatch.o"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}", f"-I{CSRC}",
                        f"-DDFFT_INST_GROUP={NUM_INST_GROUPS}", "-c", str(CSRC / "dfft_xspec.hip"), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert obj.stat().st_size > 0
    from distributedfft_amd import build
    names = [u[1].name for u in build.units()]
    assert [f"dfft_xspec_{g}.o" for g in range(NUM_INST_GROUPS + 1)] == [n for n in names if n.startswith("dfft_xspec_") and n != "dfft_xspec_api.o"]
    assert "dfft_xspec_api.o" in names


# ---- resource inventory -----------------------------------------------------------------------------------------------------------------
def test_inventory_belongs_to_the_sources_and_no_fused_kernel_spills():
    """profiles/2026-10-20_rxspec1d/kernel_resources.txt (tools/fused_resources.py rxspec) must carry the sha256 of the sources in the tree and
    list every fused instantiation -- tuned M x fp64 / fp32 x two-real / per-real accesses, less the ones rxspec_fused_ok sends to the
    composed route, which it names -- with zero scratch; dfft_rxspec1d_fused_applies agrees with it."""
    text = FI.current_text("rxspec")
    fused = [ln for ln in text.splitlines() if ln.startswith("rxspec_rows_kernel ")]
    m = re.search(r"^# composed-route \(M, type, form\): (.*)$", text, re.M)
    assert m, "the inventory names the instantiations rxspec_fused_ok sends to the composed route"
    routed = {(int(n), t, a) for n, t, a in re.findall(r"\((\d+), (f64|f32), (vec|real)\)", m.group(1))}
    assert {(n, t) for n, t, _ in routed} == XC.ROUTED
    assert len(routed) == 2 * len(XC.ROUTED) <= 20, "a few instantiations, not a way round the rule"
    tuned = sorted(RC.plan_points())
    want = {(n, t, a) for n in tuned for t in ("f64", "f32") for a in ("vec", "real")} - routed
    seen = set()
    for ln in fused:
        g = re.match(r"rxspec_rows_kernel (f64|f32) M=(\d+) E=\d+ form=(vec|real) ", ln)
        assert g, ln
        seen.add((int(g.group(2)), g.group(1), g.group(3)))
    assert seen == want and len(fused) == len(want)
    # the accumulating kernel of the unit, and the reduction and pad kernels of the common unit
    helpers = [ln for ln in text.splitlines() if ln.startswith("rxspec_mac_")] + FI.common_lines("slice_reduce_", "pad_rows_")
    assert len(helpers) == 6
    for ln in fused + helpers:
        assert re.search(r"scratch=(\d+)", ln).group(1) == "0", ln
    src = (CSRC / "dfft_xspec.hip").read_text()
    body = re.search(r"constexpr bool rxspec_fused_ok\(int M, bool f64\) \{(.*?)\n\}", src, re.S).group(1)
    lib = _lib()
    for n, t, _ in routed:
        assert re.search(rf"\b{n}\b", body), n
    for n in tuned:
        for t in ("f64", "f32"):
            assert lib.dfft_rxspec1d_fused_applies(1, 2 * n, CODE[t], 1) == int((n, t, "vec") in seen), (n, t)


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------------
_MEASURED = {}


def _yardstick():
    """The same-precision CPU pipeline (scipy.fft's rfft in that precision, numpy's for fp64 where scipy is missing; multiply; sum over the
    batch) on exactly the cases of tests/test_gpu_rxspec1d.py: worst nu per precision."""
    if _MEASURED:
        return _MEASURED
    precs = A.PRECS if sf is not None else ("f64",)
    mod = sf if sf is not None else np.fft
    for M, n, channels, batch in XC.all_cases():
        x, g, ref, _ = XC.case(M, n, channels, batch)
        m = 2 * M
        for prec in precs:
            Xs = mod.rfft(x.astype(A.RDT[prec]), m, axis=1)
            Gs = mod.rfft(g.astype(A.RDT[prec]), m, axis=1)
            assert Xs.dtype == A.CDT[prec]
            got = (np.conj(Xs) * Gs).reshape(batch, channels, M + 1).sum(axis=0, dtype=A.CDT[prec])
            v = XC.nu_lines(got, ref, m, prec)
            if v > _MEASURED.get(prec, (-1.0, ""))[0]:
                _MEASURED[prec] = (v, f"M={M} n={n} channels={channels} batch={batch}")
    return _MEASURED


@pytest.mark.parametrize("prec", A.PRECS)
def test_gpu_bound_is_at_most_eight_times_the_cpu_yardstick(prec):
    if prec == "f32" and sf is None:
        pytest.skip("the fp32 yardstick needs scipy.fft: numpy computes float32 transforms in double")
    from test_gpu_rxspec1d import BOUND
    value, what = _yardstick()[prec]
    print(f"yardstick rxspec1d {prec}: {value:.3f}  ({what})")
    assert 0 < BOUND[prec] <= 8 * value, (prec, BOUND[prec], value, what)
