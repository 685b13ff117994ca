"""Real transforms along a strided axis and batched 2-D real transforms, host side (no GPU): the new translation units cross-compile, the
argument checks of dfft_rfft1d_strided / dfft_rfft2d_batch that run before the device is queried, a numpy model of the column pairing
of csrc/dfft_real_cols.hip (split, merge, odd s, any input backward), and the committed resource inventory of its kernels."""
import ctypes as C
import hashlib
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "distributedfft_amd" / "csrc"
INVENTORY = ROOT / "profiles" / "r11" / "kernel_resources.txt"
A, B = 0x10000000, 0x20000000


def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


def test_dispatcher_unit_cross_compiles(tmp_path):
    """The dispatcher unit of dfft_real_cols.hip (multi-pass kernels and host code) builds for gfx950; build() compiles every group."""
    from distributedfft_amd.build import NUM_INST_GROUPS
    obj = tmp_path / "dfft_real_cols_dispatch.o"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}", f"-I{CSRC}",
                        f"-DDFFT_INST_GROUP={NUM_INST_GROUPS}", "-c", str(CSRC / "dfft_real_cols.hip"), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert obj.stat().st_size > 0
    from distributedfft_amd import build
    assert "dfft_real_cols.hip" in Path(build.__file__).read_text()


def _strided(inp, out, n, s, batch, dtype=0, direction=1):
    lib = _lib()
    rc = lib.dfft_rfft1d_strided(C.c_void_p(inp) if inp else None, C.c_void_p(out) if out else None, n, s, batch, dtype, direction, None)
    return rc, lib.dfft_last_error().decode()


def _rfft2(inp, out, n1, n2, batch, dtype=0, direction=1):
    lib = _lib()
    rc = lib.dfft_rfft2d_batch(C.c_void_p(inp) if inp else None, C.c_void_p(out) if out else None, n1, n2, batch, dtype, direction, None)
    return rc, lib.dfft_last_error().decode()


def test_strided_argument_errors():
    from distributedfft_amd import _lib as L
    for d in (1, -1):
        assert _strided(0, B, 16, 4, 2, direction=d)[0] == L.EINVAL
        assert _strided(A, 0, 16, 4, 2, direction=d)[0] == L.EINVAL
        assert _strided(A, B, 16, 0, 2, direction=d)[0] == L.EINVAL             # s < 1
        assert _strided(A, B, 16, -3, 2, direction=d)[0] == L.EINVAL
        assert _strided(A, B, 16, 4, -1, direction=d)[0] == L.EINVAL
        assert _strided(A, B, 16, 4, 2, dtype=7, direction=d)[0] == L.EINVAL
        assert _strided(A, A, 16, 4, 2, direction=d)[0] == L.EINVAL             # out == in
        assert _strided(A, A + 64, 16, 4, 2, direction=d)[0] == L.EINVAL        # overlapping ranges
        assert _strided(A + 64, A, 16, 4, 2, direction=d)[0] == L.EINVAL
        rc, msg = _strided(A, B, 2 ** 23 + 1, 4, 2, direction=d)
        assert rc == L.EUNSUPPORTED and str(2 ** 23 + 1) in msg
        assert _strided(A, B, 0, 4, 2, direction=d)[0] == L.EUNSUPPORTED
    assert _strided(A, B, 16, 4, 2, direction=0)[0] == L.EINVAL


def test_strided_reaches_the_device_query_for_every_form():
    from distributedfft_amd import _lib as L
    if _lib().dfft_device_count() > 0:
        return
    far = 1 << 44
    for n in (16, 512, 125, 15, 375, 15625, 16384, 1, 97, 4099):
        for s in (1, 2, 3, 1000):
            for d in (1, -1):
                assert _strided(A, far, n, s, 4, direction=d)[0] == L.ENOGPU, (n, s, d)
    # ranges that merely touch do not overlap: 2 items of 16 x 4 reals (fp64) = 1024 bytes
    assert _strided(A, A + 1024, 16, 4, 2)[0] == L.ENOGPU
    assert _strided(A, A + 1024, 16, 4, 0)[0] == L.ENOGPU


def test_rfft2d_argument_errors():
    from distributedfft_amd import _lib as L
    for d in (1, -1):
        assert _rfft2(0, B, 64, 64, 2, direction=d)[0] == L.EINVAL
        assert _rfft2(A, 0, 64, 64, 2, direction=d)[0] == L.EINVAL
        assert _rfft2(A, B, 0, 64, 2, direction=d)[0] == L.EINVAL
        assert _rfft2(A, B, 64, 0, 2, direction=d)[0] == L.EINVAL
        assert _rfft2(A, B, 64, 64, -1, direction=d)[0] == L.EINVAL
        assert _rfft2(A, B, 64, 64, 2, dtype=5, direction=d)[0] == L.EINVAL
        assert _rfft2(A, A + 128, 64, 64, 2, direction=d)[0] == L.EINVAL       # overlapping ranges
        rc, msg = _rfft2(A, B, 64, 2 ** 23 + 1, 2, direction=d)
        assert rc == L.EUNSUPPORTED and "n2" in msg                              # real_form(n2) == 0
        rc, msg = _rfft2(A, B, 2 ** 23 + 1, 64, 2, direction=d)
        assert rc == L.EUNSUPPORTED and "n1" in msg                              # length_kind(n1) == 0
    assert _rfft2(A, B, 64, 64, 2, direction=2)[0] == L.EINVAL
    if _lib().dfft_device_count() > 0:
        return
    for n1, n2 in ((64, 64), (125, 243), (97, 1009), (1, 16), (16, 1), (16384, 30)):
        for d in (1, -1):
            assert _rfft2(A, 1 << 44, n1, n2, 3, direction=d)[0] == L.ENOGPU, (n1, n2, d)


# ---- numpy model of the column pairing ------------------------------------------------------------------------------------------------
def _pair_cols_rfft(x):
    """[b][n][s] -> [b][n//2 + 1][s] through one complex transform down each pair of columns (an odd last column paired with zeros)."""
    b, n, s = x.shape
    xa = np.concatenate([x, np.zeros((b, n, s % 2))], axis=2)
    z = xa[:, :, 0::2] + 1j * xa[:, :, 1::2]
    Z = np.fft.fft(z, axis=1)
    m = np.arange(n // 2 + 1)
    Zk, Zm = Z[:, m, :], np.conj(Z[:, (-m) % n, :])
    out = np.empty((b, n // 2 + 1, xa.shape[2]), complex)
    out[:, :, 0::2] = (Zk + Zm) / 2
    out[:, :, 1::2] = (Zk - Zm) / 2j
    return out[:, :, :s]


def _pair_cols_irfft(X, n):
    """n * irfft along axis 1 of [b][n//2 + 1][s] for any input, through the merged complex columns and one inverse transform per pair."""
    b, nh, s = X.shape
    Xa = np.concatenate([X, np.zeros((b, nh, s % 2), complex)], axis=2).copy()
    Xa[:, 0, :] = Xa[:, 0, :].real
    if n % 2 == 0:
        Xa[:, n // 2, :] = Xa[:, n // 2, :].real
    a, bb = Xa[:, :, 0::2], Xa[:, :, 1::2]
    k = np.arange(n)
    lo = 2 * k <= n
    m = np.where(lo, k, n - k)
    Am, Bm = a[:, m, :], bb[:, m, :]
    Z = np.where(lo[None, :, None], Am + 1j * Bm, np.conj(Am) + 1j * np.conj(Bm))
    z = np.fft.ifft(Z, axis=1) * n
    out = np.empty((b, n, Xa.shape[2]))
    out[:, :, 0::2] = z.real
    out[:, :, 1::2] = z.imag
    return out[:, :, :s]


@pytest.mark.parametrize("n", [1, 2, 3, 8, 15, 16, 97, 125])
@pytest.mark.parametrize("s", [1, 2, 3, 7, 8])
def test_column_pair_model_matches_numpy(n, s):
    """Checks the derivation of the pairing formulas (split, merge, the zero partner of an odd last column, numpy's rule for the imaginary
    DC / Nyquist parts) on a numpy restatement -- not library code, so it cannot catch a kernel bug: tests/test_gpu_real_strided.py runs the
    kernels against numpy."""
    rng = np.random.default_rng(n * 31 + s)
    x = rng.standard_normal((3, n, s))
    assert np.abs(_pair_cols_rfft(x) - np.fft.rfft(x, axis=1)).max() < 1e-12 * max(1.0, np.abs(x).sum())
    X = rng.standard_normal((3, n // 2 + 1, s)) + 1j * rng.standard_normal((3, n // 2 + 1, s))  # any input, imaginary DC / Nyquist too
    ref = n * np.fft.irfft(X, n, axis=1)
    assert np.abs(_pair_cols_irfft(X, n) - ref).max() < 1e-12 * max(1.0, np.abs(ref).max())


# ---- resource inventory ---------------------------------------------------------------------------------------------------------------
def test_inventory_belongs_to_the_sources_and_no_fused_kernel_spills():
    """profiles/r11/kernel_resources.txt (tools/real_cols_resources.py) must carry the sha256 of the sources in the tree and list every
    fused column-pair kernel of every tuned length with zero scratch."""
    text = INVENTORY.read_text()
    h = hashlib.sha256()
    for name in ("dfft_real_cols.hip", "dfft_real_cols.h"):
        h.update((CSRC / name).read_bytes())
    m = re.match(r"# sources sha256 ([0-9a-f]{64}) ", text)
    assert m and m.group(1) == h.hexdigest(), "regenerate with: python tools/real_cols_resources.py profiles/r11/kernel_resources.txt"
    fused = [ln for ln in text.splitlines() if re.match(r"(r2c|c2r)_pair_cols_kernel ", ln)]
    tuned = {int(n) for n in re.findall(r"^\s*X\((\d+),", (CSRC / "dfft_plans.h").read_text(), re.M)} | {768}
    seen = {int(re.search(r"N=(\d+)", ln).group(1)) for ln in fused}
    assert seen == tuned
    assert len(fused) == len(tuned) * 2 * 2 * 2  # R2C / C2R x fp64 / fp32 x complex / per-real access
    for ln in fused + [ln for ln in text.splitlines() if ln.startswith(("r2c_cols_", "c2r_cols_"))]:
        assert re.search(r"scratch=(\d+)", ln).group(1) == "0", ln
