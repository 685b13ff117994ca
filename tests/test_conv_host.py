"""Host-side checks of the spectral-filter plans (dfft_plan_create_conv, api.PlanConv): symbols, filter counts, the refusals decided before
the device is queried, PlanConv's argument checks, the documented layout of the filter copy and the resource inventory
of csrc/dfft_conv.hip.  No GPU needed."""
import ast
import ctypes as C
import hashlib
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "distributedfft_amd" / "csrc"
INVENTORY = ROOT / "profiles" / "r12" / "kernel_resources.txt"
SYMBOLS = ("dfft_plan_create_conv", "dfft_conv_filter_count", "dfft_conv_set_filter", "dfft_conv_set_kernel")
A = 0x10000000


def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


def _create(n0, n1, n2, dtype=0, inp=A, out=0, P=1, g=0, flags=0, plan=True):
    lib = _lib()
    h = C.c_void_p()
    rc = lib.dfft_plan_create_conv(C.byref(h) if plan else None, n0, n1, n2, dtype, inp or None, out or None, None, g, P, flags)
    return rc, lib.dfft_last_error().decode()


def test_header_library_and_signatures_agree_on_the_conv_symbols():
    from distributedfft_amd import _lib as L
    header = (ROOT / "include" / "dfft.h").read_text()
    lib = _lib()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES, name
        assert getattr(lib, name) is not None
    assert re.search(r"#define DFFT_FILTER_COMPLEX 0\b", header) and re.search(r"#define DFFT_FILTER_REAL 1\b", header)
    assert (L.FILTER_COMPLEX, L.FILTER_REAL) == (0, 1)


def _parity_shapes():
    """SHAPES of tests/test_gpu_parity.py, read from its source (importing a GPU test module here would pull in its fixtures)."""
    tree = ast.parse((ROOT / "tests" / "test_gpu_parity.py").read_text())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "SHAPES" for t in node.targets):
            return ast.literal_eval(node.value)
    raise AssertionError("SHAPES not found")


def test_filter_count_is_local_n1_times_n2_times_n0():
    from distributedfft_amd import api
    cases = [(N, P) for N, P in _parity_shapes() if P > 1]
    assert ((10, 10, 8), 4) in cases and ((25, 10, 16), 4) in cases  # uneven splits included
    for N, P in cases:
        total = 0
        for g in range(P):
            _, _, ln1, _ = api.local_size(*N, P, g)
            cnt = api.conv_filter_count(*N, P, g)
            assert cnt == ln1 * N[2] * N[0], (N, P, g)
            total += cnt
        assert total == N[0] * N[1] * N[2], (N, P)
    assert _lib().dfft_conv_filter_count(8, 8, 8, 2, 2) == -1 and _lib().dfft_conv_filter_count(0, 8, 8, 1, 0) == -1
    with pytest.raises(ValueError):
        api.conv_filter_count(8, 8, 8, 2, 5)


def test_refusals_are_decided_before_the_device_is_queried():
    from distributedfft_amd import _lib as L
    lib = _lib()
    for flag in (L.PLAN_UNFUSED, L.PLAN_INPUT_FROM_IN, L.PLAN_OVERLAP, L.PLAN_NATURAL, L.PLAN_ANY_LENGTH):
        rc, msg = _create(64, 64, 64, flags=flag)
        assert rc == L.EUNSUPPORTED and "DFFT_PLAN_DEFAULT" in msg, (flag, rc, msg)
    assert lib.dfft_length_kind(8192) == 2 and lib.dfft_length_kind(97) == 3 and lib.dfft_length_kind(1 << 30) == 0
    for bad in (8192, 97, 1 << 30):  # four-step, Bluestein, no form at all
        for axis in range(3):
            n = [64, 64, 64]
            n[axis] = bad
            rc, msg = _create(*n)
            assert rc == L.EUNSUPPORTED and str(bad) in msg, (n, rc, msg)
    assert _create(64, 64, 64, inp=0)[0] == L.EINVAL          # NULL in
    assert _create(64, 64, 64, plan=False)[0] == L.EINVAL     # NULL plan
    assert _create(64, 64, 64, dtype=5)[0] == L.EINVAL        # bad dtype
    assert _create(0, 64, 64)[0] == L.EINVAL
    assert _create(64, 64, 64, P=2, g=2)[0] == L.EINVAL
    assert _create(64, 64, 64, P=2, g=0)[0] == L.EINVAL       # P > 1 without a communicator
    # not conv plans: the filter entry points refuse them
    assert lib.dfft_conv_set_filter(None, C.c_void_p(A), 0) == L.EINVAL
    assert lib.dfft_conv_set_kernel(None, C.c_void_p(A)) == L.EINVAL


def test_accepted_shapes_reach_the_device_query():
    from distributedfft_amd import _lib as L
    if _lib().dfft_device_count() > 0:
        return
    for N in [(64, 64, 64), (128, 16, 32), (1024, 6, 32), (2048, 4, 16), (1000, 8, 16), (343, 8, 8), (20, 36, 40), (512, 8, 9), (4096, 2, 2)]:
        for dtype in (L.F64, L.F32):
            for out in (0, A, 0x20000000):  # in place (NULL / in) and out of place
                rc, msg = _create(*N, dtype=dtype, out=out)
                assert rc == L.ENOGPU, (N, dtype, out, rc, msg)


def _bare_plan(dtype, count, filter_count):
    """A PlanConv object without a library handle: what set_filter / set_kernel check before they call the library."""
    import torch
    from distributedfft_amd import api
    p = object.__new__(api.PlanConv)
    p.handle = None  # any call into the library would fail on it
    p.dtype, p.max_count, p.filter_count, p.device = dtype, count, filter_count, torch.device("cuda:0")
    return p


def test_set_filter_argument_errors_raise_in_python():
    import torch
    from distributedfft_amd import _lib as L
    p = _bare_plan(L.F64, 8 * 8 * 8, 8 * 8 * 8)
    with pytest.raises(ValueError, match="elements expected"):
        p.set_filter(torch.zeros(100, dtype=torch.complex128))
    with pytest.raises(TypeError, match="precision"):
        p.set_filter(torch.zeros(512, dtype=torch.complex64))
    with pytest.raises(TypeError, match="precision"):
        p.set_filter(torch.zeros(512, dtype=torch.float32))
    with pytest.raises(TypeError, match="precision"):
        p.set_filter(torch.zeros(512, dtype=torch.int64))
    with pytest.raises(ValueError, match="contiguous"):
        p.set_filter(torch.zeros(8, 8, 16, dtype=torch.complex128)[:, :, ::2])
    with pytest.raises(ValueError, match="device"):
        p.set_filter(torch.zeros(512, dtype=torch.float64))  # right in every other respect, but a host tensor
    with pytest.raises(TypeError):
        p.set_filter(np.zeros(512))
    with pytest.raises(TypeError, match="precision"):
        p.set_kernel(torch.zeros(512, dtype=torch.float64))  # kernels are complex
    q = _bare_plan(L.F32, 512, 512)
    with pytest.raises(TypeError, match="precision"):
        q.set_filter(torch.zeros(512, dtype=torch.float64))
    with pytest.raises(ValueError, match="elements expected"):
        q.set_kernel(torch.zeros(511, dtype=torch.complex64))


# ---- the filter copy's layout --------------------------------------------------------------------------------------
def _copy_offsets(n0, rows, n2, plane, pitch, rot):
    """caller element (r * N2 + z) * N0 + kx goes to kx * plane + r * pitch + (rot ? (z + rot * kx) mod N2 : z)."""
    r, z, kx = np.meshgrid(np.arange(rows), np.arange(n2), np.arange(n0), indexing="ij")
    col = (z + rot * kx) % n2 if rot else z
    return (kx * plane + r * pitch + col).reshape(-1)


@pytest.mark.parametrize("n0,rows,n2,plane,pitch,rot", [
    (8, 4, 16, 4 * 16, 16, 0),                 # natural layout (P = 1 without the padded buffer; P > 1 plain rows: rows = y_local)
    (8, 4, 16, 4 * 16 + 3 * 8, 16, 0),         # padded hand-over buffer: three 128-byte lines (8 fp64 elements each) per plane
    (16, 2, 32, 2 * 32, 32, 24),               # rotated rows, 3 lines of fp64 per plane
    (16, 3, 32, 3 * 32, 32, 32),               # a rotation of a whole row is the identity
    (5, 3, 7, 3 * 7, 7, 0),                    # ragged everything
])
def test_filter_copy_layout_is_a_bijection_onto_the_documented_offsets(n0, rows, n2, plane, pitch, rot):
    off = _copy_offsets(n0, rows, n2, plane, pitch, rot)
    assert off.size == n0 * rows * n2 and np.unique(off).size == off.size          # injective
    assert off.min() == 0 and off.max() < n0 * plane                               # inside the slab
    # exactly the elements of the slab that are not padding: plane x, row r, N2 columns
    want = (np.arange(n0)[:, None, None] * plane + np.arange(rows)[None, :, None] * pitch + np.arange(n2)[None, None, :]).reshape(-1)
    assert np.array_equal(np.sort(off), np.sort(want))
    # the copy read back through the slab's own map is H[kx, r, z]: what the X stage multiplies plane kx, row r, column z by
    h = np.arange(rows * n2 * n0, dtype=np.float64)  # caller layout [r][z][kx]
    copy = np.full(n0 * plane, -1.0)
    copy[off] = h
    for kx, r, z in [(0, 0, 0), (n0 - 1, rows - 1, n2 - 1), (n0 // 2, rows // 2, n2 // 3)]:
        col = (z + rot * kx) % n2 if rot else z
        assert copy[kx * plane + r * pitch + col] == h[(r * n2 + z) * n0 + kx]


# ---- resource inventory -----------------------------------------------------------------------------------------------------------------
def test_inventory_belongs_to_the_sources_and_nothing_spills():
    """profiles/r12/kernel_resources.txt (tools/conv_resources.py) carries the sha256 of the sources in the tree, lists a fused kernel for
    every required (length x dtype x filter kind x map) and shows scratch=0 everywhere."""
    text = INVENTORY.read_text()
    h = hashlib.sha256()
    for name in ("dfft_conv.hip", "dfft_conv.h", "dfft_conv_impl.h"):
        h.update((CSRC / name).read_bytes())
    m = re.match(r"# sources sha256 ([0-9a-f]{64}) ", text)
    assert m and m.group(1) == h.hexdigest(), "regenerate with: python tools/conv_resources.py profiles/r12/kernel_resources.txt"
    kernels = [ln for ln in text.splitlines() if ln and not ln.startswith("#")]
    fused = {tuple(re.match(r"xconv_cols_kernel (\S+) N=(\d+) E=\d+ filter=(\S+) map=(\S+) ", ln).groups()) for ln in kernels if ln.startswith("xconv_cols_kernel ")}
    for n in (128, 256, 384, 512, 768, 1024):
        for t in ("f64", "f32pair"):
            for f in ("complex", "real"):
                for mp in ("plain", "rotated"):
                    assert (t, str(n), f, mp) in fused, (t, n, f, mp)
    assert any(ln.startswith("xconv_mul_kernel") for ln in kernels) and any(ln.startswith("xconv_relayout_kernel") for ln in kernels)
    for ln in kernels:
        assert re.search(r"scratch=(\d+)", ln).group(1) == "0", ln


def test_build_compiles_the_conv_units():
    from distributedfft_amd import build
    assert "dfft_conv.hip" in Path(build.__file__).read_text()
