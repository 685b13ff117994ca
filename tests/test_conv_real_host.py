"""Host-side checks of the real-field spectral-filter plans (dfft_plan_create_conv_real, api.PlanConvReal): symbols, filter counts, the
refusals decided before the device is queried, PlanConvReal's argument checks, the width rule and the documented layout of the filter copy
 and the resource inventory of csrc/dfft_conv_real.hip.  No GPU needed."""
import ctypes as C
import hashlib
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "distributedfft_amd" / "csrc"
INVENTORY = ROOT / "profiles" / "r13" / "kernel_resources.txt"
SYMBOLS = ("dfft_plan_create_conv_real", "dfft_conv_real_filter_count")
A = 0x10000000


def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


def _create(n0, n1, n2, dtype=0, inp=A, out=0, P=1, g=0, flags=0, plan=True):
    lib = _lib()
    h = C.c_void_p()
    rc = lib.dfft_plan_create_conv_real(C.byref(h) if plan else None, n0, n1, n2, dtype, inp or None, out or None, None, g, P, flags)
    return rc, lib.dfft_last_error().decode()


def test_header_library_and_signatures_agree_on_the_conv_real_symbols():
    from distributedfft_amd import _lib as L
    from distributedfft_amd import api
    header = (ROOT / "include" / "dfft.h").read_text()
    lib = _lib()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES, name
        assert getattr(lib, name) is not None
    assert L.SIGNATURES["dfft_plan_create_conv_real"] == L.SIGNATURES["dfft_plan_create_conv"]
    assert L.SIGNATURES["dfft_conv_real_filter_count"] == L.SIGNATURES["dfft_conv_filter_count"]
    assert issubclass(api.PlanConvReal, api.PlanConv) and callable(api.conv_real_filter_count)


def test_filter_count_is_local_n1_times_nh_times_n0():
    from distributedfft_amd import api
    cases = [((10, 10, 8), 4), ((25, 10, 16), 4), ((24, 10, 12), 3), ((64, 64, 64), 2), ((128, 128, 32), 8), ((64, 20, 40), 2), ((8, 8, 8), 1)]
    for N, P in cases:
        total = 0
        for g in range(P):
            _, _, ln1, _ = api.local_size(*N, P, g)
            cnt = api.conv_real_filter_count(*N, P, g)
            assert cnt == ln1 * (N[2] // 2 + 1) * N[0], (N, P, g)
            # the layout is the forward R2C plan's: its complex count holds the result [ln1][Nh][N0]
            assert api.r2c_counts(*N, P, g)[1] >= cnt
            total += cnt
        assert total == N[0] * N[1] * (N[2] // 2 + 1), (N, P)
    lib = _lib()
    assert lib.dfft_conv_real_filter_count(8, 8, 8, 2, 2) == -1 and lib.dfft_conv_real_filter_count(0, 8, 8, 1, 0) == -1
    assert lib.dfft_conv_real_filter_count(8, 8, 0, 1, 0) == -1 and lib.dfft_conv_real_filter_count(8, 8, 8, 0, 0) == -1
    assert lib.dfft_conv_real_filter_count(8, 8, 8, 2, -1) == -1
    with pytest.raises(ValueError):
        api.conv_real_filter_count(8, 8, 8, 2, 5)


def test_refusals_are_decided_before_the_device_is_queried():
    from distributedfft_amd import _lib as L
    lib = _lib()
    for flag in (L.PLAN_UNFUSED, L.PLAN_INPUT_FROM_IN, L.PLAN_OVERLAP, L.PLAN_NATURAL, L.PLAN_ANY_LENGTH, L.PLAN_OVERLAP | L.PLAN_INPUT_FROM_IN):
        rc, msg = _create(64, 64, 64, flags=flag)
        assert rc == L.EUNSUPPORTED and "DFFT_PLAN_DEFAULT" in msg, (flag, rc, msg)
    for bad in (8192, 97, 1 << 30):  # four-step, Bluestein, no form at all
        for axis in range(2):
            n = [64, 64, 64]
            n[axis] = bad
            rc, msg = _create(*n)
            assert rc == L.EUNSUPPORTED and str(bad) in msg, (n, rc, msg)
    # the real axis: dfft_real_form 1 only -- odd (form 2), 2 (form 2), Bluestein / four-step halves and lengths (form 3), nothing (form 0)
    for n2, form in ((9, 2), (2, 2), (35, 2), (194, 3), (16384, 3), (1, 3), (97, 3), (1 << 30, 0)):
        assert lib.dfft_real_form(n2) == form, (n2, lib.dfft_real_form(n2))
        rc, msg = _create(64, 64, n2)
        assert rc == L.EUNSUPPORTED and str(n2) in msg, (n2, rc, msg)
    assert _create(64, 64, 64, inp=0)[0] == L.EINVAL          # NULL in
    assert _create(64, 64, 64, plan=False)[0] == L.EINVAL     # NULL plan
    assert _create(64, 64, 64, dtype=5)[0] == L.EINVAL        # bad dtype
    assert _create(0, 64, 64)[0] == L.EINVAL
    assert _create(64, 0, 64)[0] == L.EINVAL
    assert _create(64, 64, 0)[0] == L.EINVAL
    assert _create(64, 64, 64, P=2, g=2)[0] == L.EINVAL
    assert _create(64, 64, 64, P=0, g=0)[0] == L.EINVAL
    assert _create(64, 64, 64, P=2, g=0)[0] == L.EINVAL       # P > 1 without a communicator
    # EINVAL wins over EUNSUPPORTED, as in dfft_plan_create_conv
    assert _create(64, 64, 9, inp=0)[0] == L.EINVAL


def test_accepted_shapes_reach_the_device_query():
    from distributedfft_amd import _lib as L
    lib = _lib()
    if lib.dfft_device_count() > 0:
        return
    shapes = [(64, 64, 64), (128, 16, 32), (1024, 6, 32), (2048, 4, 16), (1000, 8, 16), (343, 8, 8), (20, 36, 40), (128, 8, 4), (128, 8, 30),
              (64, 12, 10), (4096, 2, 4), (8, 8, 8192), (512, 512, 512)]
    for N in shapes:
        assert lib.dfft_real_form(N[2]) == 1
        for dtype in (L.F64, L.F32):
            for out in (0, A, 0x20000000):  # in place (NULL / in) and out of place
                rc, msg = _create(*N, dtype=dtype, out=out)
                assert rc == L.ENOGPU, (N, dtype, out, rc, msg)


def _bare_plan(dtype, count, filter_count):
    """A PlanConvReal object without a library handle: what set_filter / set_kernel check before they call the library."""
    import torch
    from distributedfft_amd import api
    p = object.__new__(api.PlanConvReal)
    p.handle = None  # any call into the library would fail on it
    p.dtype, p.max_count, p.filter_count, p.device = dtype, count, filter_count, torch.device("cuda:0")
    return p


def test_set_filter_and_set_kernel_argument_errors_raise_in_python():
    import torch
    from distributedfft_amd import _lib as L
    from distributedfft_amd import api
    p = _bare_plan(L.F64, 8 * 8 * 8, 8 * 8 * 5)
    with pytest.raises(ValueError, match="320 elements expected"):
        p.set_filter(torch.zeros(512, dtype=torch.complex128))  # the C2C count is not the real plan's
    with pytest.raises(TypeError, match="PlanConvReal.set_filter.*precision"):
        p.set_filter(torch.zeros(320, dtype=torch.complex64))
    with pytest.raises(TypeError, match="precision"):
        p.set_filter(torch.zeros(320, dtype=torch.float32))
    with pytest.raises(ValueError, match="contiguous"):
        p.set_filter(torch.zeros(8, 8, 10, dtype=torch.complex128)[:, :, ::2])
    with pytest.raises(ValueError, match="device"):
        p.set_filter(torch.zeros(320, dtype=torch.float64))  # right in every other respect, but a host tensor
    with pytest.raises(TypeError):
        p.set_filter(np.zeros(320))
    with pytest.raises(TypeError, match="precision"):
        p.set_kernel(torch.zeros(512, dtype=torch.complex128))  # kernels of a real-field plan are real
    with pytest.raises(ValueError, match="device"):
        p.set_kernel(torch.zeros(512, dtype=torch.float64))
    q = _bare_plan(L.F32, 512, 320)
    with pytest.raises(TypeError, match="precision"):
        q.set_kernel(torch.zeros(512, dtype=torch.float64))
    with pytest.raises(ValueError, match="elements expected"):
        q.set_kernel(torch.zeros(511, dtype=torch.float32))
    # the constructor refuses complex and host buffers before the library is asked
    with pytest.raises(L.DfftError) as e:
        api.PlanConvReal(8, 8, 8, torch.zeros(512, dtype=torch.float64), None, None, 0, 1)
    assert e.value.code == L.ENOGPU


# ---- the width of the private spectrum and the filter copy's layout -----------------------------------------------------
def _width(nh, prec):
    """Nc is the smallest multiple of g >= Nh for the largest power of two g, 2 < g <= one 128-byte line of elements (8 fp64,
    16 fp32), whose padding is at most Nh / 32 columns; an even Nc when no such g exists."""
    g = 8 if prec == "f64" else 16
    while g > 2:
        w = -(-nh // g) * g
        if (w - nh) * 32 <= nh:
            return w
        g //= 2
    return -(-nh // 2) * 2


def test_width_rule_examples_and_properties():
    assert (_width(257, "f64"), _width(257, "f32")) == (264, 264)   # +2.7 %: whole lines in fp64, half lines in fp32
    assert (_width(129, "f64"), _width(129, "f32")) == (132, 132)
    assert (_width(33, "f64"), _width(17, "f32"), _width(5, "f64"), _width(3, "f32"), _width(6, "f64")) == (34, 18, 6, 4, 6)
    assert (_width(16, "f64"), _width(16, "f32"), _width(513, "f32"), _width(4097, "f64")) == (16, 16, 528, 4104)
    for prec in ("f64", "f32"):
        for nh in range(1, 4098):
            w = _width(nh, prec)
            assert w % 2 == 0 and nh <= w <= nh + max(1, nh // 32), (nh, prec, w)


def _copy_offsets(n0, rows, nh, plane, pitch):
    """caller element (r * Nh + kz) * N0 + kx goes to kx * plane + r * pitch + kz."""
    r, kz, kx = np.meshgrid(np.arange(rows), np.arange(nh), np.arange(n0), indexing="ij")
    return (kx * plane + r * pitch + kz).reshape(-1)


@pytest.mark.parametrize("n0,rows,n2,prec,P1", [
    (8, 4, 16, "f64", True),     # Nh = 9 -> Nc = 10, the intermediate's rows padded to 16
    (8, 4, 16, "f32", False),    # received slab [N0][y_local][Nc]
    (16, 3, 512, "f64", False),  # Nh = 257 -> 264
    (16, 3, 512, "f32", True),   # Nh = 257 -> 264, pitch 272
    (5, 3, 8, "f64", True),      # Nh = 5 -> 6
    (5, 2, 30, "f32", False),    # Nh = 16: no padding at all
])
def test_filter_copy_layout_is_a_bijection_onto_the_documented_offsets(n0, rows, n2, prec, P1):
    nh = n2 // 2 + 1
    nc = _width(nh, prec)
    line = 8 if prec == "f64" else 16
    pitch = -(-nc // line) * line if P1 else nc   # P = 1: the intermediate's line-padded rows; P > 1: the received slab's rows
    plane = rows * pitch
    off = _copy_offsets(n0, rows, nh, plane, pitch)
    assert off.size == n0 * rows * nh and np.unique(off).size == off.size          # injective
    assert off.min() == 0 and off.max() < n0 * plane                               # inside the slab
    # exactly the first Nh columns of every row of every plane ...
    want = (np.arange(n0)[:, None, None] * plane + np.arange(rows)[None, :, None] * pitch + np.arange(nh)[None, None, :]).reshape(-1)
    assert np.array_equal(np.sort(off), np.sort(want))
    # ... and never the padding: the pad columns Nh .. Nc - 1 the X stage reads, or the row padding Nc .. pitch - 1
    pad = (np.arange(n0)[:, None, None] * plane + np.arange(rows)[None, :, None] * pitch + np.arange(nh, pitch)[None, None, :]).reshape(-1)
    assert np.intersect1d(off, pad).size == 0 and off.size + pad.size == n0 * plane
    # the copy read back through the slab's own map is H[kx, r, kz]
    h = np.arange(rows * nh * n0, dtype=np.float64)  # caller layout [r][kz][kx]
    copy = np.zeros(n0 * plane)
    copy[off] = h
    for kx, r, kz in [(0, 0, 0), (n0 - 1, rows - 1, nh - 1), (n0 // 2, rows // 2, nh // 3)]:
        assert copy[kx * plane + r * pitch + kz] == h[(r * nh + kz) * n0 + kx]
    assert not copy[pad].any()


# ---- resource inventory -----------------------------------------------------------------------------------------------------------------
def test_inventory_belongs_to_the_sources_and_nothing_spills():
    """profiles/r13/kernel_resources.txt (tools/conv_real_resources.py) carries the sha256 of the sources in the tree, lists the re-layout
    kernel for both precisions and both filter kinds and shows scratch=0 everywhere."""
    text = INVENTORY.read_text()
    h = hashlib.sha256()
    for name in ("dfft_conv_real.hip", "dfft_conv_real.h"):
        h.update((CSRC / name).read_bytes())
    m = re.match(r"# sources sha256 ([0-9a-f]{64}) ", text)
    assert m and m.group(1) == h.hexdigest(), "regenerate with: python tools/conv_real_resources.py profiles/r13/kernel_resources.txt"
    kernels = [ln for ln in text.splitlines() if ln and not ln.startswith("#")]
    kinds = {re.match(r"xconv_real_relayout_kernel (\S+) ", ln).group(1) for ln in kernels}
    assert kinds == {"f64-complex", "f64-real", "f32-complex", "f32-real"}, kinds
    for ln in kernels:
        assert re.search(r"scratch=(\d+)", ln).group(1) == "0", ln
    # every __global__ function of the unit is in the inventory
    src = (CSRC / "dfft_conv_real.hip").read_text()
    assert set(re.findall(r"(\w+_kernel)\s*\(", "".join(re.findall(r"__global__[^{;]*", src)))) == {"xconv_real_relayout_kernel"}


def test_build_compiles_the_conv_real_unit():
    from distributedfft_amd import build
    assert "dfft_conv_real.hip" in Path(build.__file__).read_text()
