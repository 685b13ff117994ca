"""Real-to-real transforms (DCT / DST, types II and III), host side (no GPU): a numpy model of the two-for-one identities of
csrc/dfft_r2r.hip against the direct O(n^2) sums, the mirror reference the GPU tests use for long n, the argument checks of
dfft_r2r1d_strided that run before the device is queried, the cross-compilation of the dispatcher unit, and the committed resource
inventory of the fused kernels."""
import ctypes as C
import hashlib
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "distributedfft_amd" / "csrc"
INVENTORY = ROOT / "profiles" / "r15" / "kernel_resources.txt"
A, B = 0x10000000, 0x20000000
KINDS = {"dct2": 0, "dct3": 1, "dst2": 2, "dst3": 3}


# ---- references (float64, along axis 1 of [b][n][s]) ------------------------------------------------------------------------------------
def direct(x, kind):
    """The defining sums (scipy.fft norm=None / FFTW REDFT10, REDFT01, RODFT10, RODFT01), as one n x n matrix product."""
    n = x.shape[1]
    i = np.arange(n)
    if kind == "dct2":
        m = 2 * np.cos(np.pi * np.outer(i, 2 * i + 1) / (2 * n))          # [k][j]
    elif kind == "dct3":
        m = 2 * np.cos(np.pi * np.outer(2 * i + 1, i) / (2 * n))          # [j][k]
        m[:, 0] = 1.0
    elif kind == "dst2":
        m = 2 * np.sin(np.pi * np.outer(i + 1, 2 * i + 1) / (2 * n))      # [k][j]
    elif kind == "dst3":
        m = 2 * np.sin(np.pi * np.outer(2 * i + 1, i + 1) / (2 * n))      # [j][k]
        m[:, n - 1] = (-1.0) ** i
    else:
        raise ValueError(kind)
    return np.matmul(m, x.astype(np.float64))   # [n][n] x [b][n][s]


def mirror(x, kind):
    """O(n log n) reference for long n.  DCT-II: rfft of the 4n odd-index embedding (u[2j+1] = u[4n-2j-1] = x[j]); DCT-III: its
    transpose (the odd bins of the 4n-point transform of 2x, x[0] halved); the DST kinds through the sign / reversal identities."""
    x = x.astype(np.float64)
    b, n, s = x.shape
    sign = ((-1.0) ** np.arange(n))[None, :, None]
    if kind == "dct2":
        u = np.zeros((b, 4 * n, s))
        u[:, 1:2 * n:2, :] = x
        u[:, 4 * n - 1:2 * n:-2, :] = x
        return np.fft.rfft(u, axis=1)[:, :n, :].real
    if kind == "dct3":
        v = np.zeros((b, 4 * n, s))
        v[:, :n, :] = 2 * x
        v[:, 0, :] = x[:, 0, :]
        return np.fft.fft(v, axis=1)[:, 1:2 * n:2, :].real
    if kind == "dst2":
        return mirror(x * sign, "dct2")[:, ::-1, :]
    if kind == "dst3":
        return sign * mirror(x[:, ::-1, :], "dct3")
    raise ValueError(kind)


def reference(x, kind):
    """What the GPU tests compare against: the direct sums up to n = 1024, the mirror reference above."""
    return direct(x, kind) if x.shape[1] <= 1024 else mirror(x, kind)


# ---- numpy model of the two-for-one method ----------------------------------------------------------------------------------------------
def _perm(n):
    """row of the caller's axis that position m of the permuted sequence holds: v[m] = x[2m] (m < ceil(n/2)), v[n-1-m] = x[2m+1]"""
    m = np.arange(n)
    return np.where(m < (n + 1) // 2, 2 * m, 2 * (n - 1 - m) + 1)


def _pairs_model(xa, xb, kind):
    """One n-point complex transform for the two real sequences xa, xb [..., n]: the identities of dfft_r2r.hip, index maps included."""
    n = xa.shape[-1]
    k = np.arange(n)
    w = np.exp(-1j * np.pi * k / (2 * n))
    p = _perm(n)
    dst = kind in ("dst2", "dst3")
    neg = np.where(dst & (k >= (n + 1) // 2), -1.0, 1.0)
    if kind in ("dct2", "dst2"):
        z = (xa[..., p] + 1j * xb[..., p]) * neg                     # DST: x (-1)^j, and perm(m) is odd exactly for m >= ceil(n/2)
        Z = np.fft.fft(z, axis=-1)
        Zt = np.conj(Z[..., (-k) % n])
        ya, yb = (w * (Z + Zt)).real, (w * (Z - Zt)).imag
        if dst:
            ya, yb = ya[..., ::-1], yb[..., ::-1]                    # stored at row n-1-k
        return ya, yb
    if dst:
        xa, xb = xa[..., ::-1], xb[..., ::-1]                        # loaded from row n-1-k

    def P(X):
        Xm = np.concatenate([np.zeros(X.shape[:-1] + (1,)), X[..., :0:-1]], axis=-1)   # X[n-k], X[n] := 0
        return np.conj(w) * (X - 1j * Xm)
    z = np.fft.ifft(P(xa) + 1j * P(xb), axis=-1) * n
    ya, yb = np.empty_like(xa), np.empty_like(xb)
    ya[..., p] = z.real * neg
    yb[..., p] = z.imag * neg
    return ya, yb


def pair_model(x, kind):
    """[b][n][s] -> [b][n][s]: adjacent columns paired for s > 1, adjacent rows for s = 1; an odd last one paired with zeros."""
    b, n, s = x.shape
    if s == 1:
        r = np.concatenate([x[:, :, 0], np.zeros((b % 2, n))], axis=0)
        ya, yb = _pairs_model(r[0::2], r[1::2], kind)
        out = np.empty_like(r)
        out[0::2], out[1::2] = ya, yb
        return out[:b, :, None]
    xa = np.concatenate([x, np.zeros((b, n, s % 2))], axis=2)
    ya, yb = _pairs_model(np.moveaxis(xa[:, :, 0::2], 1, -1), np.moveaxis(xa[:, :, 1::2], 1, -1), kind)
    out = np.empty_like(xa)
    out[:, :, 0::2], out[:, :, 1::2] = np.moveaxis(ya, -1, 1), np.moveaxis(yb, -1, 1)
    return out[:, :, :s]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n", [1, 2, 3, 8, 15, 16, 125])
def test_pair_model_and_mirror_match_the_direct_sums(n, kind):
    """Checks the derivation of the identities and of the two references on numpy restatements -- not library code, so it cannot catch
    a kernel bug: tests/test_gpu_r2r.py runs the kernels against these references."""
    rng = np.random.default_rng(n * 7 + KINDS[kind])
    for b, s in ((3, 1), (4, 1), (2, 2), (2, 3), (1, 7), (2, 8)):   # odd and even row / column counts
        x = rng.standard_normal((b, n, s))
        ref = direct(x, kind)
        tol = 1e-12 * max(1.0, np.abs(ref).max()) * n
        assert np.abs(pair_model(x, kind) - ref).max() < tol, (b, s)
        assert np.abs(mirror(x, kind) - ref).max() < tol, (b, s)
        # against scipy's conventions where scipy is present
        try:
            import scipy.fft as sf
        except ImportError:
            continue
        f = {"dct2": lambda v: sf.dct(v, 2, axis=1), "dct3": lambda v: sf.dct(v, 3, axis=1),
             "dst2": lambda v: sf.dst(v, 2, axis=1), "dst3": lambda v: sf.dst(v, 3, axis=1)}[kind]
        assert np.abs(f(x) - ref).max() < tol


@pytest.mark.parametrize("n", [1, 2, 3, 8, 15, 16, 125])
def test_type_three_of_type_two_is_2n_x(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal((2, n, 3))
    for two, three in (("dct2", "dct3"), ("dst2", "dst3")):
        assert np.abs(direct(direct(x, two), three) - 2 * n * x).max() < 1e-11 * n * n


# ---- the C entry point ------------------------------------------------------------------------------------------------------------------
def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


def _r2r(inp, out, n, s, batch, dtype=0, kind=0):
    lib = _lib()
    rc = lib.dfft_r2r1d_strided(C.c_void_p(inp) if inp else None, C.c_void_p(out) if out else None, n, s, batch, dtype, kind, None)
    return rc, lib.dfft_last_error().decode()


def test_argument_errors():
    from distributedfft_amd import _lib as L
    for kind in range(4):
        assert _r2r(0, B, 16, 4, 2, kind=kind)[0] == L.EINVAL                  # NULL pointers
        assert _r2r(A, 0, 16, 4, 2, kind=kind)[0] == L.EINVAL
        for bad in (0, -3):
            assert _r2r(A, B, bad, 4, 2, kind=kind)[0] == L.EINVAL             # n, s, batch below 1
            assert _r2r(A, B, 16, bad, 2, kind=kind)[0] == L.EINVAL
            assert _r2r(A, B, 16, 4, bad, kind=kind)[0] == L.EINVAL
        assert _r2r(A, B, 16, 4, 2, dtype=7, kind=kind)[0] == L.EINVAL
        assert _r2r(A, B, 16, 4, 2, dtype=-1, kind=kind)[0] == L.EINVAL
        rc, msg = _r2r(A, B, 2 ** 23 + 1, 4, 2, kind=kind)                     # a length of kind 0
        assert rc == L.EINVAL and str(2 ** 23 + 1) in msg
        assert _lib().dfft_length_kind(2 ** 23 + 1) == 0
        assert _r2r(A, A + 64, 16, 4, 2, kind=kind)[0] == L.EINVAL             # partial overlap, both orders
        assert _r2r(A + 64, A, 16, 4, 2, kind=kind)[0] == L.EINVAL
        assert _r2r(A, A + 16 * 4 * 2 * 8 - 8, 16, 4, 2, kind=kind)[0] == L.EINVAL
    for kind in (-1, 4, 17):
        assert _r2r(A, B, 16, 4, 2, kind=kind)[0] == L.EINVAL


def test_reaches_the_device_query_for_every_form():
    """Fused columns, fused rows, run-time-scheduled, four-step and Bluestein lengths, exact aliasing included: on a machine without a
    GPU the call gets as far as the device query."""
    from distributedfft_amd import _lib as L
    if _lib().dfft_device_count() > 0:
        return
    far = 1 << 44
    for n in (16, 512, 125, 15, 375, 16384, 1, 97, 1009):
        for s in (1, 2, 3, 1000):
            for kind in range(4):
                for dtype in (L.F64, L.F32):
                    assert _r2r(A, far, n, s, 4, dtype=dtype, kind=kind)[0] == L.ENOGPU, (n, s, kind)
                    assert _r2r(A, A, n, s, 4, dtype=dtype, kind=kind)[0] == L.ENOGPU, (n, s, kind)   # exactly in place
    # ranges that merely touch do not overlap: 2 items of 16 x 4 doubles = 1024 bytes
    assert _r2r(A, A + 1024, 16, 4, 2)[0] == L.ENOGPU
    assert _r2r(A + 1024, A, 16, 4, 2)[0] == L.ENOGPU


def test_python_constants_match_the_header():
    from distributedfft_amd import _lib as L
    text = (ROOT / "include" / "dfft.h").read_text()
    for name, val in (("DCT2", L.R2R_DCT2), ("DCT3", L.R2R_DCT3), ("DST2", L.R2R_DST2), ("DST3", L.R2R_DST3)):
        assert re.search(rf"#define DFFT_R2R_{name} {val}\b", text)
        assert KINDS[name.lower()] == val
    assert "dfft_r2r1d_strided" in L.SIGNATURES


def test_dispatcher_unit_cross_compiles(tmp_path):
    """The dispatcher unit of dfft_r2r.hip (composed-route kernels, table cache and host code) builds for gfx950; build() compiles every
    group."""
    from distributedfft_amd.build import NUM_INST_GROUPS
    obj = tmp_path / "dfft_r2r_dispatch.o"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}", f"-I{CSRC}",
                        f"-DDFFT_INST_GROUP={NUM_INST_GROUPS}", "-c", str(CSRC / "dfft_r2r.hip"), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert obj.stat().st_size > 0
    from distributedfft_amd import build
    assert "dfft_r2r.hip" in Path(build.__file__).read_text()


# ---- resource inventory -----------------------------------------------------------------------------------------------------------------
def test_inventory_belongs_to_the_sources_and_no_fused_kernel_spills():
    """profiles/r15/kernel_resources.txt (tools/r2r_resources.py) must carry the sha256 of the sources in the tree and list every fused
    instantiation -- type II / III x fp64 / fp32 x (columns per-real, columns two-element, rows) of every tuned length, less the few
    that r2r_fused_ok sends to the composed route -- with zero scratch."""
    text = INVENTORY.read_text()
    h = hashlib.sha256()
    for name in ("dfft_r2r.hip", "dfft_r2r.h"):
        h.update((CSRC / name).read_bytes())
    m = re.match(r"# sources sha256 ([0-9a-f]{64}) ", text)
    assert m and m.group(1) == h.hexdigest(), "regenerate with: python tools/r2r_resources.py profiles/r15/kernel_resources.txt"
    fused = [ln for ln in text.splitlines() if re.match(r"r2r[23]_kernel ", ln)]
    tuned = {int(n) for n in re.findall(r"^\s*X\((\d+),", (CSRC / "dfft_plans.h").read_text(), re.M)} | {768}
    m = re.search(r"^# composed-route \(n, type, kernel, form\): (.*)$", text, re.M)
    assert m, "the inventory names the instantiations r2r_fused_ok sends to the composed route"
    routed = {(int(n), t, k, f) for n, t, k, f in re.findall(r"\((\d+), (f64|f32), (r2r[23]), (\w+)\)", m.group(1))}
    want = {(n, t, k, f) for n in tuned for t in ("f64", "f32") for k in ("r2r2", "r2r3") for f in ("cols", "cols_vec", "rows")} - routed
    assert len(routed) <= 16, "a few instantiations, not a way round the rule"
    seen = set()
    for ln in fused:
        g = re.match(r"(r2r[23])_kernel (f64|f32) N=(\d+) E=\d+ form=(\w+) ", ln)
        assert g, ln
        seen.add((int(g.group(3)), g.group(2), g.group(1), g.group(4)))
    assert seen == want
    assert len(fused) == len(want)
    for ln in fused + [ln for ln in text.splitlines() if ln.startswith(("r2r_pre_", "r2r_post_"))]:
        assert re.search(r"scratch=(\d+)", ln).group(1) == "0", ln
    # the routed instantiations are lengths the source names
    src = (CSRC / "dfft_r2r.hip").read_text()
    body = re.search(r"constexpr bool r2r_fused_ok\(int n, bool f64, bool three, int form\) \{(.*?)\n\}", src, re.S).group(1)
    for n, _, _, _ in routed:
        assert re.search(rf"\b{n}\b", body), n
