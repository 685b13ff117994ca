"""-m gpu: the plan-less entry points at extents whose element or byte offsets pass 2^31 and 2^32 (tests/large_extent.py: tiled inputs,
every line checked on the device, the K base lines against longdouble references under the existing BOUND of the route's family).

One case per 32-bit guard of the plan-less routes that a call of at most 80 GiB can reach, one side just under the switch and one at or
over it where both fit ("32-bit guards of the plan-less routes", lists every guard with the case that brackets it).  The larger
tensor of a pair runs in place.  A case whose peak (buffers + the library's scratch + 1 GiB) exceeds the free HBM skips; on a 288 GB
MI355X none does.  The case tables are module constants so that tests/test_large_extent_host.py can hold the wrap assertion for every shape
and the route predicates for every switch without a GPU.  The 1-D real convolution and STFT entry points run in the sibling module
tests/test_gpu_large_extent_rows.py, whose tensors all_shapes() covers."""
import pytest

import accuracy_ref as A
import large_extent as LE

pytestmark = pytest.mark.gpu
FWD, BWD = +1, -1
F64, F32 = 0, 1
CODE = {"f64": F64, "f32": F32}

# ---- the case tables -----------------------------------------------------------------------------------------------------------------------
# dfft_fft1d_cols: (id, n, width, batch, prec, in place).  A pass of n' points over w kernel units needs (n' - 1) * w + 63 < 2^32
# (include/dfft.h): a-under / b-under sit 1 052 608 and 4 units under that for the one pass of a tuned n; e2-under sits 8 128 units under
# it for pass A (64 points over 128 * width) of the four-step 8192 = 64 * 128, with a scratch as large as the data -- on a tensor that
# starts 8 bytes past a 16-byte boundary (OFFSET), since pass A of an aligned one runs on column pairs, whose switch is at twice the width.  COLS_REFUSED are the
# column extents just over the rule: nothing runs, tests/test_large_extent_host.py asserts the refusals.  c carries the extent in the
# batch (64-bit tile bases) past 2^31 and 2^32 elements.
COLS = [
    ("a-under-n4096-odd-width", 4096, 1048575, 1, "f32", True),
    ("b-under-n64", 64, 68174083, 1, "f32", True),
    ("c-f32-over-2^31-out-of-place", 256, 24, 349526, "f32", False),
    ("c-f32-over-2^32-in-place", 256, 24, 699051, "f32", True),
    ("c-f64-over-2^31-in-place", 256, 24, 349526, "f64", True),
    ("e2-under-four-step-pass-A", 8192, 532609, 1, "f32", True),
]
OFFSET = {"e2-under-four-step-pass-A"}
COLS_REFUSED = [(4096, 1048833, "f32"), (64, 68174085, "f32"), (8192, 532611, "f32")]   # (8192: on such an offset tensor)
# dfft_fft1d_rows: (id, n, batch, prec) in place.  d: tile index times line length; e: four-step, scratch as large as the data
ROWS = [
    ("d-f32", 256, (1 << 24) + 3, "f32"),
    ("d-f64", 256, (1 << 23) + 3, "f64"),
    ("e-four-step", 8192, (1 << 19) + 1, "f32"),
]
# dfft_fft1d_any: (id, n, s, batch, prec, one launch?) in place.  f: multi-pass rows in scratch chunks, batch * n just over 2^32;
# g: the one-launch -> multi-pass switch of the columns at n * s = 2^31
ANY = [
    ("f-multi-pass-rows", 4099, 1, 1047809, "f32", False),
    ("g-over-n*s-2^31", 2039, 1053226, 1, "f32", False),
    ("g-under-n*s-2^31", 2039, 1053204, 1, "f32", True),
]
# past n * s = 2^31 the M-point passes (M = 4096) serve fp32 with even s only (column pairs on the scratch): an odd s and fp64 are refused
# (tests/test_large_extent_host.py); the even-s limit, 4095 * s / 2 + 63 < 2^32, needs 34 GB of data and 69 GB of scratch
ANY_REFUSED = [(2039, 1053227, "f32"), (2039, 1053226, "f64")]
# real transforms: (id, n, s, batch, prec, one launch? (None: rows)); forward and backward each.  h: 2^32 reals; i: the fused -> multi-pass
# switch of the strided real columns at n * s = 2^31; j: many small items, just over 2^31 reals
REAL = [
    ("h-rows", 1024, 1, (1 << 22) + 1, "f32", None),
    ("i-at-n*s-2^31", 512, 4194304, 1, "f32", False),
    ("i-under-n*s-2^31", 512, 4194302, 1, "f32", True),
    ("j-small-items", 125, 7, 2454268, "f32", True),
]
# dfft_r2r1d_strided: (id, n, s, batch, prec, kinds, placements, one launch?).  k: the fused -> composed switch at n * s = 2^31; l: rows
R2R = [
    ("k-at-n*s-2^31", 512, 4194304, 1, "f32", ("dct2", "dst3"), (True, False), False),
    ("k-under-n*s-2^31", 512, 4194302, 1, "f32", ("dct2", "dst3"), (True, False), True),
    ("k-odd-over-n*s-2^31", 512, 4194305, 1, "f32", ("dct2", "dst3"), (True, False), False),
    ("l-rows", 512, 1, (1 << 23) + 1, "f32", ("dct3", "dst2"), (True,), True),
]
# dfft_fft2d_batch in place: (id, n1, n2, batch, prec); both batches are past ZY_MAX_PLANES = 4096 (and fp32 has no one-launch stage):
# two launches per cache chunk, the first row of a chunk's row launch at x0 * n1
FFT2D = [
    ("m-f32", 256, 256, (1 << 16) + 1, "f32"),
    ("m-f64", 256, 256, (1 << 15) + 1, "f64"),
]
# dfft_rfft2d_batch, forward and backward: (id, n1, n2, batch, prec)
# "odd": an odd n2 (real form 2: the rows lease scratch) over two plane groups of 8192 planes -- forward takes and returns the lease once
# per group around the rows (the columns lease their own), backward holds one lease across both groups
RFFT2D = [("n", 512, 512, (1 << 14) + 1, "f32"), ("odd", 64, 63, 8192 + 61, "f64")]


def all_shapes():
    """(what, batch, m, s, elem_bytes) of every tensor of every case: what the wrap assertion has to hold for"""
    c = {"f64": 16, "f32": 8}
    out = []
    for cid, n, w, b, p, _ in COLS:
        out.append((cid, b, n, w, c[p]))
    for cid, n, b, p in ROWS:
        out.append((cid, b, n, 1, c[p]))
    for cid, n, s, b, p, _ in ANY:
        out.append((cid, b, n, s, c[p]))
    for cid, n, s, b, p, _ in REAL:
        out += [(cid + " reals", b, n, s, c[p] // 2), (cid + " bins", b, n // 2 + 1, s, c[p])]
    for cid, n, s, b, p, *_ in R2R:
        out.append((cid, b, n, s, c[p] // 2))
    for cid, n1, n2, b, p in FFT2D:
        out.append((cid, b, n1 * n2, 1, c[p]))
    for cid, n1, n2, b, p in RFFT2D:
        out += [(cid + " reals", b, n1 * n2, 1, c[p] // 2), (cid + " bins", b, n1 * (n2 // 2 + 1), 1, c[p])]
    import test_gpu_large_extent_rows as rows_module   # the 1-D real convolution and STFT entry points: the sibling module's tensors
    return out + rows_module.shapes()


# ---- running a case --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def _worst_per_family():
    """After the module's last case: the worst line difference per family and precision, the figures of DESIGN.md section 7k."""
    yield
    for (family, prec), (value, what) in sorted(LE.WORST_LINES.items()):
        print(f"large-extent worst {family} {prec}: {value:.3f} eps sqrt(log2 n) (limit {2 * A.BOUND[family][prec]})  {what}")


def _run(gpu, what, family, prec, n_eff, base_in, ref, batch, s, call, inplace, scratch=0, offset=False):
    """The skip is decided here, before anything is allocated or run: the case's peak against the free HBM."""
    import torch
    torch.cuda.empty_cache()  # blocks cached by earlier tests do not count as free otherwise
    free, _ = torch.cuda.mem_get_info()
    K, peak, _, _ = LE.case_plan(prec, base_in, ref, batch, s, inplace, scratch)
    if peak > free:
        pytest.skip(f"needs {peak / 2**30:.0f} GiB of HBM, {free / 2**30:.0f} free")
    LE.run_case(gpu, what, family, prec, n_eff, base_in, ref, batch, s, call, inplace, K=K, scratch=scratch, offset=offset)


def _k(shapes):
    return LE.pick_k(shapes)


def _family(n):
    from test_gpu_parity import TUNED
    return "tuned" if n in TUNED else "generic"


def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


# ---- columns ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,n,width,batch,prec,inplace", COLS, ids=[c[0] for c in COLS])
def test_cols(gpu, cid, n, width, batch, prec, inplace):
    from distributedfft_amd import api
    off = cid in OFFSET
    assert _lib().dfft_cols_extent_supported(n, width, CODE[prec], 0 if off else 1) == 1
    K = _k([(batch, n, width, LE.CBYTES[prec])])
    x, ref = LE.complex_base(n, K, FWD)
    four = api.length_kind(n) == 2
    _run(gpu, f"cols {cid}", "four-step" if four else _family(n), prec, n, x, ref, batch, width, lambda t, o: api.fft1d_cols(t, FWD, out=o),
         inplace, scratch=batch * n * width * LE.CBYTES[prec] if four else 0, offset=off)


# ---- rows ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,n,batch,prec", ROWS, ids=[c[0] for c in ROWS])
def test_rows(gpu, cid, n, batch, prec):
    from distributedfft_amd import api
    K = _k([(batch, n, 1, LE.CBYTES[prec])])
    x, ref = LE.complex_base(n, K, BWD)
    four = api.length_kind(n) == 2
    _run(gpu, f"rows {cid}", "four-step" if four else _family(n), prec, n, x, ref, batch, 1,
         lambda t, o: api.fft1d_rows(t.view(batch, n), BWD, out=o.view(batch, n)), True,
         scratch=batch * n * LE.CBYTES[prec] if four else 0)


# ---- any length ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,n,s,batch,prec,fused", ANY, ids=[c[0] for c in ANY])
def test_any(gpu, cid, n, s, batch, prec, fused):
    from distributedfft_amd import api
    lib = _lib()
    assert api.length_kind(n) == 3 and bool(lib.dfft_bluestein_fused_applies(n, s)) == fused   # the route the case is there for
    assert lib.dfft_fft1d_any_extent_supported(n, s, CODE[prec], 1, 1) == 1
    scratch = int(lib.dfft_fft1d_any_scratch_bytes(n, s, batch, CODE[prec]))
    assert (scratch == 0) == fused
    K = _k([(batch, n, s, LE.CBYTES[prec])])
    x, ref = LE.complex_base(n, K, FWD)
    _run(gpu, f"any {cid}", "bluestein", prec, n, x, ref, batch, s, lambda t, o: api.fft1d_any(t, 1, FWD, out=o), True, scratch=scratch)


# ---- real ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forward", [True, False], ids=["fwd", "bwd"])
@pytest.mark.parametrize("cid,n,s,batch,prec,fused", REAL, ids=[c[0] for c in REAL])
def test_real(gpu, cid, n, s, batch, prec, fused, forward):
    from distributedfft_amd import api
    lib = _lib()
    scratch = 0
    if fused is not None:
        assert bool(lib.dfft_rfft_cols_fused_applies(n, s, CODE[prec])) == fused
        scratch = int(lib.dfft_rfft1d_strided_scratch_bytes(n, s, batch, CODE[prec]))
        assert (scratch == 0) == fused
    nh = n // 2 + 1
    K = _k([(batch, n, s, LE.CBYTES[prec] // 2), (batch, nh, s, LE.CBYTES[prec])])
    if forward:
        x, ref = LE.real_base(n, K)
        call = (lambda t, o: api.rfft1d(t.view(batch, n), out=o.view(batch, nh))) if s == 1 else (lambda t, o: api.rfft1d(t, out=o, dim=1))
    else:
        x, ref = LE.half_base(n, K)
        call = (lambda t, o: api.irfft1d(t.view(batch, nh), n, out=o.view(batch, n))) if s == 1 else (lambda t, o: api.irfft1d(t, n, out=o, dim=1))
    _run(gpu, f"{'rfft' if forward else 'irfft'} {cid}", "real", prec, n, x, ref, batch, s, call, False, scratch=scratch)


# ---- real to real ----------------------------------------------------------------------------------------------------------------------------
def _r2r_params():
    for cid, n, s, batch, prec, kinds, places, fused in R2R:
        for kind in kinds:
            for inplace in places:
                yield pytest.param(n, s, batch, prec, kind, inplace, fused, id=f"{cid}-{kind}-{'in-place' if inplace else 'out-of-place'}")


@pytest.mark.parametrize("n,s,batch,prec,kind,inplace,fused", list(_r2r_params()))
def test_r2r(gpu, n, s, batch, prec, kind, inplace, fused):
    from distributedfft_amd import api
    lib = _lib()
    vec = int(s > 1 and s % 2 == 0)   # torch's allocations are aligned to two reals
    assert bool(lib.dfft_r2r_fused_applies(n, s, CODE[prec], api.R2R_KINDS[kind], vec)) == fused
    scratch = int(lib.dfft_r2r1d_strided_scratch_bytes(n, s, batch, CODE[prec], api.R2R_KINDS[kind], vec))
    assert (scratch == 0) == fused
    K = _k([(batch, n, s, LE.CBYTES[prec] // 2)])
    x, ref = LE.r2r_base(n, K, kind)
    _run(gpu, f"r2r {kind} n={n} s={s} batch={batch} {'in place' if inplace else 'out of place'}", "r2r", prec, n, x, ref, batch, s,
         lambda t, o: api.r2r(t, kind, dim=1, out=o), inplace, scratch=scratch)


# ---- 2-D ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,n1,n2,batch,prec", FFT2D, ids=[c[0] for c in FFT2D])
def test_fft2d(gpu, cid, n1, n2, batch, prec):
    from distributedfft_amd import api
    K = _k([(batch, n1 * n2, 1, LE.CBYTES[prec])])
    x, ref = LE.planes_base(n1, n2, K, FWD)
    assert batch > 4096   # past ZY_MAX_PLANES: two launches per cache chunk, not the one-launch stage -- the "2d" family
    _run(gpu, f"fft2d {cid}", "2d", prec, n1 * n2, x, ref, batch, 1,
         lambda t, o: api.fft2d_batch(t.view(batch, n1, n2), FWD, out=o.view(batch, n1, n2)), True)


@pytest.mark.parametrize("forward", [True, False], ids=["fwd", "bwd"])
@pytest.mark.parametrize("cid,n1,n2,batch,prec", RFFT2D, ids=[c[0] for c in RFFT2D])
def test_rfft2d(gpu, cid, n1, n2, batch, prec, forward):
    from distributedfft_amd import api
    nh = n2 // 2 + 1
    K = _k([(batch, n1 * n2, 1, LE.CBYTES[prec] // 2), (batch, n1 * nh, 1, LE.CBYTES[prec])])
    if forward:
        x, ref = LE.real_planes_base(n1, n2, K)
        call = lambda t, o: api.rfft2d_batch(t.view(batch, n1, n2), out=o.view(batch, n1, nh))  # noqa: E731
    else:
        x, ref = LE.half_planes_base(n1, n2, K)
        call = lambda t, o: api.irfft2d_batch(t.view(batch, n1, nh), n2, out=o.view(batch, n1, n2))  # noqa: E731
    # backward: one 256 MiB group of bins plus the inner transforms' scratch, at most as much again
    _run(gpu, f"{'rfft2d' if forward else 'irfft2d'} {cid}", "real", prec, n1 * n2, x, ref, batch, 1, call, False, scratch=0 if forward else 1 << 29)
