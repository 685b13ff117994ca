"""Host-side checks of the multi-output real-field spectral-filter plans (dfft_plan_create_conv_real_multi, dfft_conv_set_factors,
api.PlanConvRealMulti): symbols, the refusals decided before the device is queried, a numpy model of the factor tables' addressing
 and the resource inventory of csrc/dfft_conv_multi.hip.  No GPU needed."""
import ctypes as C
import hashlib
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "distributedfft_amd" / "csrc"
INVENTORY = ROOT / "profiles" / "r14" / "kernel_resources.txt"
SYMBOLS = ("dfft_plan_create_conv_real_multi", "dfft_conv_set_factors")
FUSED_LENGTHS = (64, 128, 256, 384, 512, 768, 1024)
A = 0x10000000
STEP = 0x01000000


def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


def _create(n0, n1, n2, dtype=0, inp=A, outs=(A + STEP, A + 2 * STEP), nout=None, P=1, g=0, flags=0, plan=True, null_outs=False):
    lib = _lib()
    h = C.c_void_p()
    arr = (C.c_void_p * max(1, len(outs)))(*[o or None for o in outs])
    rc = lib.dfft_plan_create_conv_real_multi(C.byref(h) if plan else None, n0, n1, n2, dtype, inp or None, None if null_outs else arr,
                                              len(outs) if nout is None else nout, None, g, P, flags)
    return rc, lib.dfft_last_error().decode()


def test_header_library_and_signatures_agree_on_the_multi_symbols():
    from distributedfft_amd import _lib as L
    from distributedfft_amd import api
    header = (ROOT / "include" / "dfft.h").read_text()
    lib = _lib()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES, name
        assert getattr(lib, name) is not None
    m = re.search(r"#define\s+DFFT_CONV_MAX_OUTPUTS\s+(\d+)", header)
    assert m and int(m.group(1)) == L.CONV_MAX_OUTPUTS == 8
    internal = (CSRC / "dfft_conv_multi.h").read_text()
    assert re.search(r"CONV_MAX_OUTPUTS\s*=\s*8\b", internal)
    res, args = L.SIGNATURES["dfft_plan_create_conv_real_multi"]
    # the single-output signature with (void* const* outs, int noutputs) in the place of `out`
    one = L.SIGNATURES["dfft_plan_create_conv_real"][1]
    assert res is C.c_int and len(args) == len(one) + 1 and args[:6] == one[:6] and args[8:] == one[7:]
    assert args[6] == C.POINTER(C.c_void_p) and args[7] is C.c_int
    assert L.SIGNATURES["dfft_conv_set_factors"] == (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p])
    assert issubclass(api.PlanConvRealMulti, api.PlanConvReal) and callable(api.PlanConvRealMulti.set_factors)


def test_refusals_are_decided_before_the_device_is_queried():
    from distributedfft_amd import _lib as L
    lib = _lib()
    # the output list
    assert _create(64, 64, 64, outs=(), nout=0)[0] == L.EINVAL
    assert _create(64, 64, 64, outs=tuple(A + (k + 1) * STEP for k in range(9)))[0] == L.EINVAL
    assert _create(64, 64, 64, outs=(A + STEP,), nout=-1)[0] == L.EINVAL
    assert _create(64, 64, 64, null_outs=True)[0] == L.EINVAL
    rc, msg = _create(64, 64, 64, outs=(A + STEP, 0, A + 2 * STEP))
    assert rc == L.EINVAL and "outs[1]" in msg, (rc, msg)                          # a NULL out
    rc, msg = _create(64, 64, 64, outs=(A + STEP, A + 2 * STEP, A + STEP))
    assert rc == L.EINVAL and "same buffer" in msg, (rc, msg)                      # two equal outs
    # everything dfft_plan_create_conv_real refuses, with its codes
    for flag in (L.PLAN_UNFUSED, L.PLAN_INPUT_FROM_IN, L.PLAN_OVERLAP, L.PLAN_NATURAL, L.PLAN_ANY_LENGTH, L.PLAN_OVERLAP | L.PLAN_INPUT_FROM_IN):
        rc, msg = _create(64, 64, 64, flags=flag)
        assert rc == L.EUNSUPPORTED and "DFFT_PLAN_DEFAULT" in msg, (flag, rc, msg)
    for bad in (8192, 97, 1 << 30):  # four-step, Bluestein, no form at all
        for axis in range(2):
            n = [64, 64, 64]
            n[axis] = bad
            rc, msg = _create(*n)
            assert rc == L.EUNSUPPORTED and str(bad) in msg, (n, rc, msg)
    for n2, form in ((9, 2), (2, 2), (35, 2), (194, 3), (16384, 3), (1, 3), (97, 3), (1 << 30, 0)):
        assert lib.dfft_real_form(n2) == form
        rc, msg = _create(64, 64, n2)
        assert rc == L.EUNSUPPORTED and str(n2) in msg, (n2, rc, msg)
    rc, msg = _create(4096, 4096, 512)                                              # the 2^31 bound
    assert rc == L.EUNSUPPORTED and "2^31" in msg, (rc, msg)
    assert _create(64, 64, 64, inp=0)[0] == L.EINVAL
    assert _create(64, 64, 64, plan=False)[0] == L.EINVAL
    assert _create(64, 64, 64, dtype=5)[0] == L.EINVAL
    assert _create(0, 64, 64)[0] == L.EINVAL
    assert _create(64, 0, 64)[0] == L.EINVAL
    assert _create(64, 64, 0)[0] == L.EINVAL
    assert _create(64, 64, 64, P=2, g=2)[0] == L.EINVAL
    assert _create(64, 64, 64, P=0, g=0)[0] == L.EINVAL
    assert _create(64, 64, 64, P=2, g=0)[0] == L.EINVAL       # P > 1 without a communicator
    assert _create(64, 64, 9, inp=0)[0] == L.EINVAL           # EINVAL wins over EUNSUPPORTED
    assert _create(64, 64, 9, outs=(A + STEP, A + STEP))[0] == L.EINVAL
    # set_factors without a plan
    assert lib.dfft_conv_set_factors(None, 0, None, None, None) == L.EINVAL


def test_accepted_shapes_reach_the_device_query():
    from distributedfft_amd import _lib as L
    lib = _lib()
    if lib.dfft_device_count() > 0:
        return
    shapes = [(64, 64, 64), (128, 16, 32), (1024, 6, 32), (2048, 4, 16), (1000, 8, 16), (343, 8, 8), (20, 36, 40), (128, 8, 4), (128, 8, 30),
              (64, 12, 10), (512, 512, 512)]
    for N in shapes:
        for dtype in (L.F64, L.F32):
            for outs in ((A + STEP,), (A,), (A, A + STEP, A + 2 * STEP), tuple(A + (k + 1) * STEP for k in range(8))):  # outs[0] may be `in`
                rc, msg = _create(*N, dtype=dtype, outs=outs)
                assert rc == L.ENOGPU, (N, dtype, outs, rc, msg)


def test_python_argument_checks_come_before_the_library():
    import torch
    from distributedfft_amd import _lib as L
    from distributedfft_amd import api
    x = torch.zeros(512, dtype=torch.float64)
    with pytest.raises(L.DfftError) as e:
        api.PlanConvRealMulti(8, 8, 8, x, [torch.zeros(512, dtype=torch.float64)], None, 0, 1)
    assert e.value.code == L.ENOGPU
    p = object.__new__(api.PlanConvRealMulti)
    p.handle = None
    p.dtype, p.N, p.noutputs, p.device = L.F64, (8, 6, 8), 2, torch.device("cuda:0")
    with pytest.raises(ValueError, match="output 2 of 2"):
        p.set_factors(2)
    with pytest.raises(ValueError, match="8 elements expected"):
        p.set_factors(0, ax=torch.zeros(6, dtype=torch.complex128))
    with pytest.raises(ValueError, match="6 elements expected"):
        p.set_factors(0, ay=torch.zeros(8, dtype=torch.complex128))
    with pytest.raises(ValueError, match="5 elements expected"):
        p.set_factors(0, az=torch.zeros(8, dtype=torch.complex128))
    with pytest.raises(TypeError, match="precision"):
        p.set_factors(0, az=torch.zeros(5, dtype=torch.complex64))
    with pytest.raises(ValueError, match="device"):
        p.set_factors(1, ay=torch.zeros(6, dtype=torch.complex128))  # right in every other respect, but a host tensor


# ---- the factor tables -----------------------------------------------------------------------------------------------
def _slab(n, P, g):
    blk = -(-n // P)
    return g * blk, (blk if g < P - 1 else n - (P - 1) * blk)


def _width(nh, prec):
    g = 8 if prec == "f64" else 16
    while g > 2:
        w = -(-nh // g) * g
        if (w - nh) * 32 <= nh:
            return w
        g //= 2
    return -(-nh // 2) * 2


def _tables(N, P, g, prec, K, factors):
    """one block per plan -- `ones` elements of 1, then per output a (N0 rounded up to even) | b (this device's rows y0 ..
    y0 + y_local of the caller's global vector, rounded up to even) | c (Nc wide, zeros behind N2/2 + 1).  Returns the block and per
    output the three offsets the X stage reads from (0: the ones)."""
    n0, n1, n2 = N
    nh = n2 // 2 + 1
    nc = _width(nh, prec)
    y0, ys = _slab(n1, P, g)
    fa, fb = -(-n0 // 2) * 2, -(-ys // 2) * 2
    ones = max(fa, fb, nc)
    per = fa + fb + nc
    block = np.zeros(ones + K * per, dtype=np.complex128)
    block[:ones] = 1
    offs = []
    for k, (ax, ay, az) in enumerate(factors):
        ta = ones + k * per
        tb, tc = ta + fa, ta + fa + fb
        if ax is not None:
            block[ta:ta + n0] = ax
        if ay is not None:
            block[tb:tb + ys] = ay[y0:y0 + ys]
        if az is not None:
            block[tc:tc + nc] = 0
            block[tc:tc + nh] = az
        offs.append((ta if ax is not None else 0, tb if ay is not None else 0, tc if az is not None else 0))
    return block, offs, (ys, nc, nh, y0)


@pytest.mark.parametrize("N,P,prec", [((8, 10, 16), 4, "f64"), ((8, 10, 16), 3, "f32"), ((25, 10, 16), 4, "f64"), ((24, 10, 12), 3, "f32"),
                                      ((16, 3, 512), 1, "f64")])
def test_factor_tables_slice_ay_at_y0_and_pad_az_to_the_width(N, P, prec):
    n0, n1, n2 = N
    r = np.random.default_rng(3)
    K = 3
    factors = [(r.standard_normal(n0) + 1j, r.standard_normal(n1) + 2j, r.standard_normal(n2 // 2 + 1) + 3j), (None, np.arange(n1) + 0j, None),
               (None, None, None)]
    seen = np.zeros(n1, dtype=int)
    for g in range(P):
        block, offs, (ys, nc, nh, y0) = _tables(N, P, g, prec, K, factors)
        assert y0 == g * -(-n1 // P) and nc % 2 == 0 and nc >= nh
        for k, (oa, ob, oc) in enumerate(offs):
            ax, ay, az = factors[k]
            # every table starts on a 16-byte boundary in both precisions (fp32 elements are 8 bytes: even offsets)
            assert oa % 2 == 0 and ob % 2 == 0 and oc % 2 == 0
            # what the X stage reads for plane x, local row r and column z is the caller's a[x], b[y0 + r], c[z] -- and 0 in the pad columns
            assert np.array_equal(block[oa:oa + n0], ax if ax is not None else np.ones(n0))
            assert np.array_equal(block[ob:ob + ys], ay[y0:y0 + ys] if ay is not None else np.ones(ys))
            if az is not None:
                assert np.array_equal(block[oc:oc + nh], az) and not block[oc + nh:oc + nc].any()
            else:
                assert np.array_equal(block[oc:oc + nc], np.ones(nc))
        # the arange factor of output 1 names the global rows this device read
        ob = offs[1][1]
        rows = block[ob:ob + ys].real.astype(int)
        assert np.array_equal(rows, np.arange(y0, y0 + ys))
        seen[rows] += 1
        # tables of different outputs do not overlap: writing output 0's tables leaves the others' as they were
        other, _, _ = _tables(N, P, g, prec, K, [(None, None, None)] + factors[1:])
        per = (len(block) - max(-(-n0 // 2) * 2, -(-ys // 2) * 2, nc)) // K
        assert np.array_equal(block[-2 * per:], other[-2 * per:])
    assert (seen == 1).all(), "every global row is read by exactly one device"
    # the uneven splits the issue names: N1 = 10 over P = 4 is 3 + 3 + 3 + 1, over P = 3 it is 4 + 4 + 2
    assert [_slab(10, 4, g) for g in range(4)] == [(0, 3), (3, 3), (6, 3), (9, 1)]
    assert [_slab(10, 3, g) for g in range(3)] == [(0, 4), (4, 4), (8, 2)]


def test_the_library_source_addresses_the_tables_as_the_model_does():
    src = (CSRC / "dfft_plan_conv.cpp").read_text()
    body = src[src.index("int dfft_conv_set_factors("):]
    body = body[:body.index("\n}\n")]
    assert "plan->sy.start(plan->me)" in body and "plan->ys" in body          # ay from y0, y_local elements
    assert re.search(r"hipMemsetAsync\(tc, 0, \(size_t\)c->L\.ncols \* cs", body)  # az: the whole Nc-wide table cleared first
    assert re.search(r"hipMemcpyAsync\(tc, az, \(size_t\)c->nh \* cs", body)       # then N2/2 + 1 elements copied


# ---- resource inventory -----------------------------------------------------------------------------------------------------------------
def test_inventory_belongs_to_the_sources_and_nothing_spills():
    """profiles/r14/kernel_resources.txt (tools/conv_multi_resources.py) carries the sha256 of the sources in the tree, lists the fused
    kernel of every fused length in both precisions and for both filter kinds and the factor multiply, and shows scratch=0 everywhere."""
    text = INVENTORY.read_text()
    h = hashlib.sha256()
    for name in ("dfft_conv_multi.hip", "dfft_conv_multi.h", "dfft_conv_impl.h"):
        h.update((CSRC / name).read_bytes())
    m = re.match(r"# sources sha256 ([0-9a-f]{64}) ", text)
    assert m and m.group(1) == h.hexdigest(), "regenerate with: python tools/conv_multi_resources.py profiles/r14/kernel_resources.txt"
    kernels = [ln for ln in text.splitlines() if ln and not ln.startswith("#")]
    fused = set()
    for ln in kernels:
        f = re.match(r"xconv_multi_cols_kernel (f64|f32pair) N=(\d+) E=\d+ filter=(complex|real) ", ln)
        if f:
            fused.add((f.group(1), int(f.group(2)), f.group(3)))
    # the lengths that claim xconv=fused: the one conv_fused_n of dfft_conv_impl.h, which both kernel units take -- no list of their own
    shared = (CSRC / "dfft_conv_impl.h").read_text()
    claimed = tuple(int(v) for v in re.findall(r"n == (\d+)", re.search(r"constexpr bool conv_fused_n\(int n\) \{([^}]*)\}", shared).group(1)))
    assert claimed == FUSED_LENGTHS
    for name in ("dfft_conv_multi.h", "dfft_conv_multi.hip", "dfft_conv.hip"):
        own = (CSRC / name).read_text()
        assert not re.search(r"\bn == \d+", own) and not re.search(r"constexpr bool \w*fused_n\b", own), name
        assert name.endswith(".h") or '#include "dfft_conv_impl.h"' in own, name
    assert fused == {(t, n, k) for t in ("f64", "f32pair") for n in FUSED_LENGTHS for k in ("complex", "real")}, fused
    assert {ln.split()[1] for ln in kernels if ln.startswith("xconv_factor_mul_kernel ")} == {"f64", "f32x2"}
    for ln in kernels:
        assert re.search(r"scratch=(\d+)", ln).group(1) == "0", ln
    # every __global__ function of the unit is in the inventory
    src = (CSRC / "dfft_conv_multi.hip").read_text()
    names = set(re.findall(r"(\w+_kernel)\s*\(", "".join(re.findall(r"__global__[^{;]*", src))))
    assert names == {"xconv_multi_cols_kernel", "xconv_factor_mul_kernel"}
    assert names == {ln.split()[0] for ln in kernels}


def test_build_compiles_the_conv_multi_unit():
    from distributedfft_amd import build
    text = Path(build.__file__).read_text()
    assert "dfft_conv_multi.hip" in text and "dfft_conv_multi_{g}.o" in text


def test_the_single_output_sources_are_untouched():
    """The conv sources the multi-output kernel shares its traits with (dfft_conv_impl.h among them) are the ones pinned by sha256 into
    profiles/r12 and r13: a change to the shared header shows up in the single-output inventory too."""
    for inv, names in ((ROOT / "profiles" / "r12" / "kernel_resources.txt", ("dfft_conv.hip", "dfft_conv.h", "dfft_conv_impl.h")),
                       (ROOT / "profiles" / "r13" / "kernel_resources.txt", ("dfft_conv_real.hip", "dfft_conv_real.h"))):
        h = hashlib.sha256()
        for name in names:
            h.update((CSRC / name).read_bytes())
        assert re.match(r"# sources sha256 ([0-9a-f]{64}) ", inv.read_text()).group(1) == h.hexdigest()
