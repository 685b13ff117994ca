"""Long batched 1-D real cross-spectrum (dfft_rxspec1d_long), host side (no GPU): the symbols, a numpy restatement of the kernels held
against numpy.fft, the gradient formulas of rconv1d_long / fftconv1d_long against torch's CPU autograd, the chunk / slice rule through
the library, the refusals that are decided before the device is queried, the build units, the committed resource inventory of the
kernels, and the CPU yardstick that the bound of tests/test_gpu_rxspec1d_long.py is made from."""
import ctypes as C
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import accuracy_ref as A
import fused_inventory as FI
import rconv1d_long_cases as LC
import rxspec1d_long_cases as LX

try:
    import scipy.fft as sf
except ImportError:   # pragma: no cover
    sf = None

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "distributedfft_amd" / "csrc"
INVENTORY = ROOT / "profiles" / "2026-10-20_rxspec1d_long" / "kernel_resources.txt"
SYMBOLS = ("dfft_rxspec1d_long", "dfft_rxspec1d_long_fused_applies", "dfft_rxspec1d_long_scratch_bytes", "dfft_rxspec1d_long_slices")
X, G, OUT = 0x10000000, 0x20000000, 0x30000000
F64, F32 = 0, 1
CODE = {"f64": F64, "f32": F32}


def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


def _call(x=X, g=G, out=OUT, n=9000, m=16384, channels=3, batch=4, dtype=F64, order=0):
    lib = _lib()
    vp = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    rc = lib.dfft_rxspec1d_long(vp(x), vp(g), vp(out), n, m, channels, batch, dtype, order, None)
    return rc, lib.dfft_last_error().decode()


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
    assert L.SIGNATURES["dfft_rxspec1d_long"][1] == [C.c_void_p] * 3 + [C.c_longlong] * 4 + [C.c_int, C.c_int, C.c_void_p]
    assert L.SIGNATURES["dfft_rxspec1d_long_scratch_bytes"][0] == C.c_ulonglong
    assert L.SIGNATURES["dfft_rxspec1d_long_slices"] == (C.c_longlong, [C.c_longlong] * 3 + [C.c_int])
    assert "DFFT_RXSPEC_LONG_FUSED" in header
    assert callable(api.rxspec1d_long)
    # the rule is stated in the header with the constants the helper restates
    for word in ("256 MiB", f"{LX.TARGET_ITEMS} / (channels * ceil(N1 / 2))", f"steps / {LX.MIN_STEPS}"):
        assert word in header, word


# ---- numpy model of the kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2", [(4, 8), (3, 8), (5, 5), (8, 4), (2, 3)])
def test_kernel_model_matches_numpy(n1, n2):
    """Pass A + the accumulating Mid step + the store in both orders, thread for thread, against numpy.fft: the [k1][k2] layout, the
    partner map, rows 0 and N1/2, the factored pairing twiddle, bins 0 and M from Z[0] alone, the slices; odd N1, a self-paired row
    N1/2, N1 > N2 and odd M included.  Not library code: tests/test_gpu_rxspec1d_long.py runs the kernels."""
    M = n1 * n2
    m = 2 * M
    rng = np.random.default_rng(100 * n1 + n2)
    for n in (m, m // 2, m // 2 + 1, 5, 1):
        for channels, batch, slices, row0 in ((1, 1, 1, 0), (3, 5, 2, 0), (2, 3, 3, 0), (3, 4, 1, 2)):
            rows = batch * channels
            x, g = rng.standard_normal((rows, n)), rng.standard_normal((rows, n))
            chan = (row0 + np.arange(rows)) % channels
            P = np.conj(np.fft.rfft(x, m, axis=1)) * np.fft.rfft(g, m, axis=1)
            Pa = np.abs(np.fft.rfft(x, m, axis=1)) ** 2
            want = np.stack([P[chan == c].sum(axis=0) for c in range(channels)])
            wanta = np.stack([Pa[chan == c].sum(axis=0) for c in range(channels)])
            for order in (0, 1):
                got = LX.kernel_model(x, g, n1, n2, channels, slices, order, row0)
                ref = LC.permute_filter(want, n1, n2) if order else want
                assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (n1, n2, n, channels, batch, order)
                assert np.all(got[:, 0].imag == 0) and np.all(got[:, M].imag == 0)
                a = LX.kernel_model(x, x, n1, n2, channels, slices, order, row0)
                refa = LC.permute_filter(wanta, n1, n2) if order else wanta
                assert np.all(a.imag == 0) and np.all(a.real >= 0), "the auto-spectrum has exact-zero imaginary parts"
                assert np.abs(a - refa).max() <= 1e-12 * np.abs(refa).max(), (n1, n2, n, channels, batch, order, "auto")
    H = LC.make_filter(2, m, "complex", M)
    assert np.array_equal(LX.unpermute(LC.permute_filter(H, n1, n2), n1, n2), H)


# ---- the gradient formulas --------------------------------------------------------------------------------------------------------------
def test_gradient_formulas_match_torch_cpu_autograd():
    """grad_x = rconv1d_long(g, conj Hp), grad_Hp = w / m * S in the filter's order (its real part for a real Hp), grad_k =
    irfft(S)[:taps] / m ... with S the cross-spectrum of x and g -- against torch's autograd of irfft(rfft(x, m) * H, m)[..., :n] in
    float64 at a long length, m = 10240 = 2 * 64 * 80, all on the CPU.  The permuted filter enters the autograd graph through the index
    map of rconv1d_long_filter, so the claim that conjugation and the bin weights commute with the permutation is checked too."""
    import torch
    m, channels, batch, n, taps = 10240, 2, 3, 6000, 4000
    M = m // 2
    n1, n2 = LX.SPLITS[m]
    gen = torch.Generator().manual_seed(m)
    x = torch.randn(batch, channels, n, dtype=torch.float64, generator=gen)
    g = torch.randn(batch, channels, n, dtype=torch.float64, generator=gen)
    S = LX.reference(x.reshape(-1, n).numpy(), g.reshape(-1, n).numpy(), m, channels).astype(np.complex128)
    Sp = torch.from_numpy(LC.permute_filter(S, n1, n2))
    S = torch.from_numpy(S)
    w = torch.full((M + 1,), 2.0 / m, dtype=torch.float64)
    w[0] = w[-1] = 1.0 / m
    # H[k] = Hp[pos[k]]: pos[k1 + N1 k2] = k1 N2 + k2, pos[M] = M
    pos = torch.from_numpy(LX.unpermute(np.arange(M + 1)[None, :], n1, n2)[0].copy())

    def conv(x, H):
        return torch.fft.irfft(torch.fft.rfft(x, m) * H, m)[..., :n]

    for real in (False, True):
        H = torch.randn(channels, M + 1, dtype=torch.float64 if real else torch.complex128, generator=gen)
        Hp = torch.from_numpy(LC.permute_filter(H.numpy(), n1, n2))
        assert torch.equal(Hp[:, pos], H)
        xa, Hpa = x.clone().requires_grad_(True), Hp.clone().requires_grad_(True)
        conv(xa, Hpa[:, pos]).backward(g)
        gx = conv(g, Hp.conj()[:, pos])                       # rconv1d_long(g, conj Hp)
        assert (xa.grad - gx).abs().max() <= 1e-12 * xa.grad.abs().max()
        want = (Sp.real if real else Sp) * w                  # w is its own permutation: bins 0 and M stay where they are
        assert (Hpa.grad - want).abs().max() <= 1e-12 * want.abs().max(), ("grad_Hp", real)
    k = torch.randn(channels, taps, dtype=torch.float64, generator=gen, requires_grad=True)
    assert n + taps - 1 <= m
    xa = x.clone().requires_grad_(True)
    conv(xa, torch.fft.rfft(torch.nn.functional.pad(k, (0, m - taps)))).backward(g)
    want = torch.fft.irfft(S, m)[:, :taps]                    # torch's irfft carries the 1 / m
    assert (k.grad - want).abs().max() <= 1e-12 * want.abs().max()
    # ... and the longdouble formulas the GPU tests use say the same
    Hc = torch.randn(channels, M + 1, dtype=torch.complex128, generator=gen)
    xa = x.clone().requires_grad_(True)
    conv(xa, Hc).backward(g)
    gx = LX.ld_conv(g.reshape(-1, n).numpy(), np.conj(Hc.numpy()), m, n).astype(np.float64).reshape(batch, channels, n)
    assert np.abs(xa.grad.numpy() - gx).max() <= 1e-12 * np.abs(gx).max()
    assert np.abs(LX.bin_weights(m).astype(np.float64) - w.numpy()).max() == 0


# ---- the chunk / slice rule -------------------------------------------------------------------------------------------------------------
def test_chunk_and_slice_rule_through_the_library(monkeypatch):
    """dfft_rxspec1d_long_slices and ..._scratch_bytes equal the helper's restatement of the rule of include/dfft.h over a grid of
    (m, channels, batch), whatever the environment; the step ranges are contiguous and cover the steps once."""
    lib = _lib()
    for env in (None, "0"):
        if env is None:
            monkeypatch.delenv("DFFT_RXSPEC_LONG_FUSED", raising=False)
        else:
            monkeypatch.setenv("DFFT_RXSPEC_LONG_FUSED", env)
        for m in LX.LENGTHS + [1 << 21, 1 << 23, 2 * 81 * 2048]:
            for prec in A.PRECS:
                for channels, batch in ((1, 1), (1, 15), (1, 16), (1, 17), (3, 5), (3, 100), (2, 4096), (16, 768), (64, 64), (3, 1 << 20), (5000, 3)):
                    what = (m, prec, channels, batch)
                    assert lib.dfft_rxspec1d_long_slices(m, channels, batch, CODE[prec]) == LX.call_slices(m, channels, batch, prec), what
                    assert lib.dfft_rxspec1d_long_scratch_bytes(m // 2 + 1, m, channels, batch, CODE[prec]) == LX.scratch_bytes(m, channels, batch, prec), what
                    rows = batch * channels
                    ch = LX.chunks(m, prec, rows)
                    assert ch[0][0] == 0 and ch[-1][0] + ch[-1][1] == rows and len({k for _, k in ch[:-1]}) <= 1 and ch[-1][1] <= ch[0][1]
                    assert ch[0][1] * 2 * (m // 2) * LX.ESIZE[prec] <= max(LX.SCRATCH_CAP, 2 * (m // 2) * LX.ESIZE[prec])
                    for k in {ch[0][1], ch[-1][1]}:      # the whole chunks are all alike, the last one may be ragged
                        steps, s = -(-k // channels), LX.slices_rule(m, channels, k)
                        rg = LX.step_ranges(steps, s)
                        assert 1 <= s <= steps and rg[0][0] == 0 and sum(c for _, c in rg) == steps
                        assert all(a + c == b for (a, c), (b, _) in zip(rg, rg[1:])) and max(c for _, c in rg) - min(c for _, c in rg) <= 1
    # one slice while the batch is short, the item target caps the count, the smallest ragged cut
    assert LX.call_slices(10240, 1, 15, "f64") == 1 and LX.call_slices(10240, 1, 16, "f64") == 2 and LX.ragged_batch(10240) == 17
    assert LX.call_slices(10240, 1, 1 << 20, "f32") == LX.slices_rule(10240, 1, LX.chunk_rows(10240, "f32", 1 << 20)) == 2048 // 32
    assert LX.call_slices(16384, 64, 4096, "f64") == 1          # 64 * 32 items with one slice already
    # several chunks: 256 MiB / (2 * 5120 * 16 B) = 1638 rows of m = 10240 in fp64
    assert LX.chunk_rows(10240, "f64", 10 ** 6) == 1638 and LX.chunk_rows(10240, "f32", 10 ** 6) == 3276
    assert LX.chunk_rows(1 << 23, "f64", 9) == 2 and LX.chunk_rows(1 << 23, "f64", 1) == 1
    # not a call the entry point would accept: no slices, no lease
    for bad in ((8192, 1, 1, F64), (16386, 1, 1, F64), (16384, 0, 1, F64), (16384, 1, 0, F64), (16384, 1 << 16, 1 << 15, F64), (16384, 1, 1, 3)):
        assert lib.dfft_rxspec1d_long_slices(*bad) == 0, bad
        assert lib.dfft_rxspec1d_long_scratch_bytes(1, *bad) == 0, bad
    assert lib.dfft_rxspec1d_long_scratch_bytes(16385, 16384, 1, 1, F64) == 0


def test_route_rule(monkeypatch):
    lib = _lib()
    monkeypatch.delenv("DFFT_RXSPEC_LONG_FUSED", raising=False)
    for m in LX.LENGTHS + [LX.mid_length(N) for N in LX.FACTORS if N > 64]:
        for prec in A.PRECS:
            assert lib.dfft_rxspec1d_long_fused_applies(m, CODE[prec]) == int(LX.fused(m, prec)), (m, prec)
    assert lib.dfft_rxspec1d_long_fused_applies(8192, F64) == 0 and lib.dfft_rxspec1d_long_fused_applies(16384, 5) == 0
    monkeypatch.setenv("DFFT_RXSPEC_LONG_FUSED", "0")
    assert lib.dfft_rxspec1d_long_fused_applies(16384, F64) == 0
    monkeypatch.setenv("DFFT_RXSPEC_LONG_FUSED", "1")
    assert lib.dfft_rxspec1d_long_fused_applies(16384, F64) == 1


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_are_decided_before_the_device_is_queried():
    from distributedfft_amd import _lib as L
    lib = _lib()
    accepted = {2 * a * b for a in LX.FACTORS for b in LX.FACTORS if 8192 < 2 * a * b <= 1 << 23}
    for dtype in (F64, F32):
        for order in (0, 1):
            kw = dict(dtype=dtype, order=order)
            assert _call(x=0, **kw)[0] == L.EINVAL                        # NULL pointers
            assert _call(g=0, **kw)[0] == L.EINVAL
            assert _call(out=0, **kw)[0] == L.EINVAL
            for bad in (0, -3):                                           # sizes below 1
                assert _call(n=bad, **kw)[0] == L.EINVAL
                assert _call(m=bad, **kw)[0] == L.EINVAL
                assert _call(channels=bad, **kw)[0] == L.EINVAL
                assert _call(batch=bad, **kw)[0] == L.EINVAL
            assert _call(n=16385, m=16384, **kw)[0] == L.EINVAL           # m < n
            assert _call(n=20000, m=16386, **kw)[0] == L.EINVAL           # ... before m is judged
            rs = 8 if dtype == F64 else 4
            data, ob = 9000 * 3 * 4 * rs, 3 * 8193 * 2 * rs
            for fld in ("x", "g"):                                        # out overlaps x or g: inside, at the end, from in front
                base = X if fld == "x" else G
                for bad in (base, base + data - rs, base - ob + rs):
                    rc, msg = _call(out=bad, **kw)
                    assert rc == L.EINVAL and "overlaps" in msg, (fld, bad, rc, msg)
            assert _call(x=X, g=X, out=X + rs, **kw)[0] == L.EINVAL       # the auto-spectrum too
            for m in (8192, 128, 4096, 16385, 16386, 2 * 64 * 63, 2 * 343 * 64, 2 * 49 * 256, (1 << 23) + 2, 1 << 30):
                rc, msg = _call(n=1, m=m, **kw)
                assert rc == L.EUNSUPPORTED and f"m = {m}" in msg, (m, rc, msg)
    # every m that dfft_rconv1d_long_split rejects, over a stretch of the range
    for m in range(8190, 21000):
        ok = lib.dfft_rconv1d_long_split(m, None, None) == 1
        assert ok == (m in accepted)
        if not ok:
            assert _call(n=1, m=m)[0] == L.EUNSUPPORTED, m
    for dtype in (-1, 2, 7):
        assert _call(dtype=dtype)[0] == L.EINVAL
    for order in (-1, 2):
        assert _call(order=order)[0] == L.EINVAL
    # 2^31 rows or more
    assert _call(n=1, channels=1 << 16, batch=1 << 15)[0] == L.EUNSUPPORTED
    assert _call(n=1, channels=1 << 40, batch=1 << 40)[0] == L.EUNSUPPORTED
    assert _call(n=1, channels=1, batch=1 << 31)[0] == L.EUNSUPPORTED
    # dfft_rxspec1d itself still stops at 8192
    vp = C.c_void_p
    assert lib.dfft_rxspec1d(vp(X), vp(G), vp(OUT), 1, 16384, 3, 4, F64, None) == L.EUNSUPPORTED


def test_valid_calls_reach_the_device_query():
    from distributedfft_amd import _lib as L
    if _lib().dfft_device_count() > 0:
        return
    for m in LX.LENGTHS + [1 << 23]:
        for n in (m, m // 2 + 1, 5, 1):
            for dtype in (F64, F32):
                for order in (0, 1):
                    assert _call(n=n, m=m, dtype=dtype, order=order, g=1 << 42, out=1 << 44)[0] == L.ENOGPU, (m, n)
                    assert _call(x=X, g=X, n=n, m=m, dtype=dtype, order=order, out=1 << 44)[0] == L.ENOGPU    # the auto-spectrum
    data, ob = 9000 * 3 * 4 * 8, 3 * 8193 * 16
    assert _call(out=X + data)[0] == L.ENOGPU                       # ranges that merely touch do not overlap
    assert _call(out=G - ob)[0] == L.ENOGPU
    assert _call(n=1, channels=(1 << 16) - 1, batch=1 << 15, g=1 << 42, out=1 << 44)[0] == L.ENOGPU


# ---- build ------------------------------------------------------------------------------------------------------------------------------
def test_dispatcher_unit_cross_compiles_and_build_units(tmp_path):
    """The dispatcher unit of dfft_lxspec.hip (reduction, composed-route kernels, tables and host code) builds for gfx950; build()
    compiles every group under names that the unit lists of the convolution and the short cross-spectrum do not pick up."""
    from distributedfft_amd import build
    from distributedfft_amd.build import NUM_INST_GROUPS
    obj = tmp_path / "dfft_lxspec_dispatch.o"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}", f"-I{CSRC}",
                        f"-DDFFT_INST_GROUP={NUM_INST_GROUPS}", "-c", str(CSRC / "dfft_lxspec.hip"), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert obj.stat().st_size > 0
    names = [u[1].name for u in build.units()]
    assert [f"dfft_lxspec_{g}.o" for g in range(NUM_INST_GROUPS + 1)] == [n for n in names if n.startswith("dfft_lxspec_")]


# ---- resource inventory -----------------------------------------------------------------------------------------------------------------
def test_inventory_belongs_to_the_sources_and_no_fused_kernel_spills():
    """profiles/2026-10-20_rxspec1d_long/kernel_resources.txt (tools/fused_resources.py lxspec) must carry the sha256 of the sources in the
    tree and list every fused instantiation -- the accumulating Mid kernel of the 17 factor lengths above 64 x fp64 / fp32, less the
    (N2, type) lxspec_fused_ok sends to the composed route, which it names; pass A of the 18 factor lengths x fp64 / fp32 x two-real /
    per-real accesses -- with zero scratch; dfft_rxspec1d_long_fused_applies agrees with it."""
    text = FI.current_text("lxspec")
    m = re.search(r"^# composed-route \(N2, type\): (.*)$", text, re.M)
    assert m, "the inventory names the (N2, type) lxspec_fused_ok sends to the composed route"
    routed = set(re.findall(r"\((\d+), (f64|f32)\)", m.group(1)))
    routed = {(int(n), t) for n, t in routed}
    assert routed == LX.ROUTED and len(routed) <= 6, "a few instantiations, not a way round the rule"
    above = [n for n in LX.FACTORS if n > 64]
    assert len(above) == 17 and len(LX.FACTORS) == 18
    want_mid = {(n, t) for n in above for t in A.PRECS} - routed
    want_a = {(n, t, v) for n in LX.FACTORS for t in A.PRECS for v in ("vec", "real")}
    mid = [ln for ln in text.splitlines() if ln.startswith("lxspec_mid_kernel ")]
    pa = [ln for ln in text.splitlines() if ln.startswith("lxspec_a_kernel ")]
    seen_mid, seen_a = set(), set()
    for ln in mid:
        g = re.match(r"lxspec_mid_kernel (f64|f32) N=(\d+) E=\d+ variant=any ", ln)
        assert g, ln
        seen_mid.add((int(g.group(2)), g.group(1)))
    for ln in pa:
        g = re.match(r"lxspec_a_kernel (f64|f32) N=(\d+) E=\d+ variant=(vec|real) ", ln)
        assert g, ln
        seen_a.add((int(g.group(2)), g.group(1), g.group(3)))
    assert seen_mid == want_mid and len(mid) == len(want_mid) == 17 * 2 - len(routed)
    assert seen_a == want_a and len(pa) == len(want_a)
    # the reduction and accumulating kernels of the unit, and the pad kernel of the common unit
    helpers = [ln for ln in text.splitlines() if ln.startswith(("lxspec_reduce_", "lxspec_mac_"))] + FI.common_lines("pad_rows_")
    assert len(helpers) == 6
    for ln in mid + pa + helpers:
        assert re.search(r"scratch=(\d+)", ln).group(1) == "0", ln
    # the routed lengths are lengths the source names, and the library routes every split with one of them as the longer factor
    src = (CSRC / "dfft_lxspec.hip").read_text()
    body = re.search(r"constexpr bool lxspec_fused_ok\(int N, bool f64\) \{(.*?)\n\}", src, re.S).group(1)
    for n, _ in routed:
        assert re.search(rf"\b{n}\b", body), n
    lib = _lib()
    for n in above:
        for t in A.PRECS:
            assert lib.dfft_rxspec1d_long_fused_applies(LX.mid_length(n), CODE[t]) == int((n, t) in seen_mid), (n, t)
            assert lib.dfft_rxspec1d_long_fused_applies(2 * n * n, CODE[t]) == int((n, t) in seen_mid), (n, t)


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------------
_MEASURED = {}


def round_up_two_digits(v):
    """v rounded up to two significant digits"""
    e = math.floor(math.log10(v)) - 1
    return round(math.ceil(v / 10 ** e - 1e-9) * 10 ** e, 10)


def _yardstick():
    """The same-precision CPU pipeline (scipy.fft's rfft in that precision, numpy's for fp64 where scipy is missing; multiply; sum over the
    batch) on exactly the cases of tests/test_gpu_rxspec1d_long.py: worst nu per (precision, class of case)."""
    if _MEASURED:
        return _MEASURED
    precs = A.PRECS if sf is not None else ("f64",)
    mod = sf if sf is not None else np.fft
    cases = [(c, LX.case(*c)[:3], A.PRECS) for c in LX.all_cases()] + [(c, LX.chunk_case(*c), ("f64",)) for c in LX.CHUNK_CASES]
    for (m, n, channels, batch), (x, g, ref), case_precs in cases:
        for prec in precs:
            if prec not in case_precs:
                continue
            Xs = mod.rfft(x.astype(A.RDT[prec]), m, axis=1)
            Gs = mod.rfft(g.astype(A.RDT[prec]), m, axis=1)
            assert Xs.dtype == A.CDT[prec]
            got = (np.conj(Xs) * Gs).reshape(batch, channels, m // 2 + 1).sum(axis=0, dtype=A.CDT[prec])
            v, key = LX.nu_lines(got, ref, m, prec), (prec, LX.klass(n, batch))
            if v > _MEASURED.get(key, (-1.0, ""))[0]:
                _MEASURED[key] = (v, f"m={m} n={n} channels={channels} batch={batch}")
    return _MEASURED


@pytest.mark.parametrize("prec", A.PRECS)
def test_bound_is_twice_the_larger_of_the_cpu_yardstick_and_the_composed_route(prec):
    """Per class of case: BOUND = 2 x max(the recorded CPU-pipeline worst, the recorded composed-route worst), rounded up to two digits;
    the CPU pipeline, measured again here on exactly the GPU test's cases, stays under it."""
    for k in LX.BOUND[prec]:
        cpu, comp = LX.MEASURED["cpu"][prec][k], LX.MEASURED["composed"][prec][k]
        assert LX.BOUND[prec][k] == round_up_two_digits(2 * max(cpu, comp)), (prec, k, LX.BOUND[prec][k], cpu, comp)
    if prec == "f32" and sf is None:
        return   # the fp32 yardstick needs scipy.fft: numpy computes float32 transforms in double
    for k in LX.BOUND[prec]:
        value, what = _yardstick()[(prec, k)]
        print(f"yardstick rxspec1d_long {prec} {k}: {value:.3f}  ({what})")
        assert 0 < value <= LX.BOUND[prec][k], (prec, k, value, what)


def test_round_up():
    assert round_up_two_digits(1.138) == 1.2 and round_up_two_digits(8.472) == 8.5 and round_up_two_digits(55.508) == 56.0
    assert round_up_two_digits(0.5) == 0.5 and round_up_two_digits(1.2) == 1.2 and round_up_two_digits(0.1234) == 0.13
