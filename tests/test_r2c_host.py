"""Real-to-complex / complex-to-real slab plans, host side (no GPU): the buffer counts, the argument checks that run before the device is
queried, and the kernel sources the r2c kernels include but must not change."""
import ctypes as C
import hashlib
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "distributedfft_amd" / "csrc"


def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


def _slab(n, P, g):
    blk = -(-n // P)
    return (blk if g < P - 1 else n - (P - 1) * blk), blk


@pytest.mark.parametrize("N,P", [((25, 10, 16), 4), ((24, 10, 12), 4), ((48, 100, 12), 1), ((14, 49, 16), 2), ((512, 512, 512), 1),
                                 ((512, 512, 512), 8), ((1024, 768, 512), 3), ((7, 5, 4802), 3)])
def test_r2c_counts_match_the_layout(N, P):
    from distributedfft_amd import api
    n0, n1, n2 = N
    nh = n2 // 2 + 1
    for g in range(P):
        xs, _ = _slab(n0, P, g)
        ys, yblk = _slab(n1, P, g)
        ylast, _ = _slab(n1, P, P - 1)
        real, cplx = api.r2c_counts(n0, n1, n2, P, g)
        assert real == xs * n1 * n2
        send = (P - 1) * xs * yblk * nh + xs * ylast * nh if P > 1 else 0
        assert cplx == max(ys * nh * n0, send)
        # the complex side of a C2C plan of the same shape holds N2 instead of N2/2 + 1 bins per row
        assert cplx <= api.get_max_data_count(n0, n1, n2, P, g == P - 1)


def test_r2c_counts_rejects_bad_arguments():
    lib = _lib()
    r, c = C.c_longlong(), C.c_longlong()
    assert lib.dfft_r2c_counts(0, 4, 4, 1, 0, C.byref(r), C.byref(c)) == -1
    assert lib.dfft_r2c_counts(4, 4, 4, 2, 2, C.byref(r), C.byref(c)) == -1
    assert lib.dfft_r2c_counts(2, 4, 4, 4, 0, C.byref(r), C.byref(c)) == -1  # the last device would own no plane


def _create(n0, n1, n2, flags=0, in_ptr=0x1000, out_ptr=0x2000, dtype=0, direction=1, P=1, g=0):
    lib = _lib()
    h = C.c_void_p()
    rc = lib.dfft_plan_create_r2c(C.byref(h), n0, n1, n2, dtype, direction, C.c_void_p(in_ptr), C.c_void_p(out_ptr) if out_ptr else None,
                                  None, g, P, flags)
    return rc, lib.dfft_last_error().decode()


@pytest.mark.parametrize("direction", [1, -1])
def test_r2c_plan_argument_errors(direction):
    """Checked before the device query: these codes are the same with and without a GPU."""
    from distributedfft_amd import _lib as L
    d = dict(direction=direction)
    rc, msg = _create(16, 16, 15, **d)
    assert rc == L.EUNSUPPORTED and "N2 = 15" in msg                    # odd N2
    rc, msg = _create(16, 16, 22, **d)
    assert rc == L.EUNSUPPORTED and "N2 = 22" in msg                    # N2/2 = 11 is no supported length
    rc, msg = _create(16, 16, 2 * 8192, **d)
    assert rc == L.EUNSUPPORTED                                         # N2/2 beyond 4096
    rc, msg = _create(8192, 16, 16, **d)
    assert rc == L.EUNSUPPORTED and "8192" in msg                       # long N0
    rc, msg = _create(16, 8192, 16, **d)
    assert rc == L.EUNSUPPORTED and "8192" in msg                       # long N1
    assert _create(16, 16, 16, out_ptr=0, **d)[0] == L.EINVAL           # out == NULL
    assert _create(16, 16, 16, out_ptr=0x1000, **d)[0] == L.EINVAL      # out == in
    for f in (L.PLAN_OVERLAP, L.PLAN_NATURAL, L.PLAN_UNFUSED, L.PLAN_OVERLAP | L.PLAN_INPUT_FROM_IN):
        assert _create(16, 16, 16, flags=f, **d)[0] == L.EUNSUPPORTED, f
    assert _create(16, 16, 16, dtype=7, **d)[0] == L.EINVAL
    assert _create(16, 16, 16, P=2, g=0, **d)[0] == L.EINVAL            # P > 1 without a communicator


def test_r2c_plan_accepts_supported_sizes_up_to_the_device_query():
    """Supported shapes pass every argument check: without a GPU the first error is the device query's.  (On a machine with a GPU the
    plan would be created -- on the dummy pointers of this test -- so there the check is the counts' alone; tests/test_gpu_r2c.py
    creates real plans of these shapes.)"""
    from distributedfft_amd import _lib as L
    from distributedfft_amd import api
    shapes = ((16, 16, 16), (25, 10, 16), (14, 49, 4802), (12, 12, 8192), (8, 8, 40), (8, 8, 7200))
    for N in shapes:
        assert api.r2c_counts(*N, 1, 0)[0] == N[0] * N[1] * N[2]
    if _lib().dfft_device_count() > 0:
        return
    for N in shapes:
        for flags in (L.PLAN_DEFAULT, L.PLAN_INPUT_FROM_IN):
            assert _create(*N, flags=flags)[0] == L.ENOGPU, N


def test_pinned_kernel_sources_unchanged():
    """The r2c kernels include the C2C kernel sources and must not change them: every file tools/kernel_resources.py pins still hashes to
    the first line of profiles/r06/kernel_resources.txt (which is what keeps every C2C kernel byte-identical)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    pinned = {"dfft_fft_impl.h", "dfft_butterfly.h", "dfft_plans.h", "dfft_fft_inst.hip", "dfft_zy.hip", "dfft_zy.h", "dfft_kernels.h"}
    assert pinned <= set(kr.KERNEL_SOURCES)
    line = (ROOT / "profiles" / "r06" / "kernel_resources.txt").read_text().splitlines()[0]
    assert re.match(r"# kernel sources sha256 ([0-9a-f]{64})", line).group(1) == kr.sources_sha256()
    h = hashlib.sha256()
    for name in kr.KERNEL_SOURCES:
        h.update(name.encode())
        h.update((CSRC / name).read_bytes())
    assert h.hexdigest() == kr.sources_sha256()
