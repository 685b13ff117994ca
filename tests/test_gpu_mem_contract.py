"""-m gpu: the buffer contract of the complex transforms -- dfft_fft1d_rows, dfft_fft1d_cols, dfft_fft1d_any, dfft_fft2d_batch, the c2c
plans and the spectral-filter plans (include/dfft.h): any element-aligned pointers; out of place `in` is never written; nothing outside
`out` is written; in place gives what out of place gives.

Every buffer is a view inside a larger allocation with sentinel regions on both sides (tests/mem_contract.py): at least 64 elements and
two rows of the innermost pitch, compared bit for bit after every call.  Offset cases start ONE ELEMENT past a 16-byte boundary: for
complex64 that is an 8-byte-aligned base, which fp32 column launches cannot run on column pairs (16-byte accesses) -- they take the
scalar float2 fall-back with its own tile geometry, whole-tile and ragged kernels of every length, which aligned torch allocations of an
even width never reach.  Results are judged with the long-double references and bounds of tests/accuracy_ref.py (one line = one row /
column / plane / rank), so a misplaced or dropped column fails even where the guards hold; the figures are printed, and the worst per
family at the end of the module."""
import math
import threading

import numpy as np
import pytest

import accuracy_ref as A
import mem_contract as M
from test_gpu_parity import GENERIC, TUNED

pytestmark = pytest.mark.gpu
FWD, BWD = +1, -1
ALIGNED, OFFSET = (0, 0), (1, 1)
FOUR_WAYS = [(1, 1), (1, 0), (0, 1), (0, 0)]     # (in, out) one element past a 16-byte boundary: both, in only, out only, neither
EDGE_LENGTHS = [2, 7, 16, 64, 125, 343, 512, 768, 1000, 1024, 2048, 4096, 15, 360, 3600]


@pytest.fixture(scope="module", autouse=True)
def _worst_per_family():
    before = dict(A.WORST)
    yield
    for (family, prec), (value, what) in sorted(A.WORST.items()):
        if before.get((family, prec)) != (value, what):
            print(f"mem-contract worst {family} {prec}: nu {value:.3f} (bound {A.BOUND[family][prec]})  {what}")


def _cdt(prec):
    import torch
    return torch.complex128 if prec == "f64" else torch.complex64


def _rdt(prec):
    import torch
    return torch.float64 if prec == "f64" else torch.float32


def _load(view, x):
    """numpy values (float32-exact) -> the guarded view, in its precision"""
    import torch
    view.copy_(torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).to(view.device).to(view.dtype))
    torch.cuda.synchronize()


def _family(n):
    return "tuned" if n in TUNED else "generic"


def _sign(d):
    return "fwd" if d > 0 else "bwd"


def _one(gpu, call, prec, x, shape, pitch, offs, d, score, what):
    """One out-of-place call on guarded buffers with (in, out) offsets `offs`, then -- where both sides share one alignment -- the same
    call in place at that alignment.  score(numpy result) checks the values; here: the guards around `out` and `in`, `in` bit-equal,
    in place bit-equal to out of place."""
    import torch
    count = math.prod(shape)
    ibuf, iv = M.guarded(count, _cdt(prec), gpu, offs[0], pitch)
    obuf, ov = M.guarded(count, _cdt(prec), gpu, offs[1], pitch)
    _load(iv, x)
    keep = iv.clone()
    assert iv.data_ptr() % 16 == (offs[0] * iv.element_size()) % 16 and ov.data_ptr() % 16 == (offs[1] * ov.element_size()) % 16
    call(iv.view(shape), d, ov.view(shape))
    tag = f"{what} {_sign(d)} in+{offs[0]} out+{offs[1]}"
    M.guards_intact(obuf, ov, tag + " (out)")
    M.guards_intact(ibuf, iv, tag + " (in)")
    assert M.bits_equal(iv, keep), f"{tag}: an out-of-place call changed `in`"
    score(ov.view(shape).cpu().numpy(), tag)
    if offs[0] == offs[1]:
        pbuf, pv = M.guarded(count, _cdt(prec), gpu, offs[1], pitch)
        pv.copy_(keep)
        call(pv.view(shape), d, pv.view(shape))
        M.guards_intact(pbuf, pv, tag + " (in place)")
        assert M.bits_equal(pv, ov), f"{tag}: in place differs from out of place at the same alignment"


def _lines(gpu, call, family, prec, n, shape, axis, offsets, what):
    """Scaled random lines of length n along `axis` of `shape` (A.complex_lines: a line that picks up a fraction of its neighbour fails on
    its own norm), forward and backward, for every (in, out) offset pair; unit impulses once per direction at the first pair."""
    x, F = A.complex_lines(n, shape, axis, 1000 + n)
    refs = {FWD: F, BWD: A.reverse_bins(F, [axis])}
    pitch = shape[-1]
    for offs in offsets:
        for d in (FWD, BWD):
            _one(gpu, call, prec, x, shape, pitch, offs, d,
                 lambda got, tag, d=d: A.check(family, prec, A.nu(got, refs[d], n, prec, (axis,)), tag), what)
    pos = tuple(A.impulse_positions(n))
    xi, Fi = A.impulse_lines(n, shape, axis, pos)
    irefs = {FWD: Fi, BWD: np.conj(Fi)}
    for d in (FWD, BWD):
        _one(gpu, call, prec, xi, shape, pitch, offsets[0], d,
             lambda got, tag, d=d: A.check(family + "-impulse", prec, A.nu_impulse(got, irefs[d], prec), tag + " impulses"), what)


def _rows(t, d, out):
    from distributedfft_amd import api
    return api.fft1d_rows(t, d, out=out)


def _cols(t, d, out):
    from distributedfft_amd import api
    return api.fft1d_cols(t, d, out=out)


def _any(dim):
    def call(t, d, out):
        from distributedfft_amd import api
        return api.fft1d_any(t, dim, d, out=out)
    return call


# ---- 1. columns, fp32, 8-byte-aligned base: the scalar fall-back's whole-tile (width 32) and ragged (width 20) kernels of every length ----
@pytest.mark.parametrize("width", [32, 20])
@pytest.mark.parametrize("n", TUNED + GENERIC)
def test_cols_fp32_on_an_8_byte_aligned_base(gpu, n, width):
    """Width 32 is a multiple of every scalar tile width (at most 16 columns): whole tiles.  Width 20 is ragged and even: GENERAL scalar
    where the aligned control runs GENERAL pairs.  One misaligned side is enough to leave the pair kernels (make_pair_launch)."""
    _lines(gpu, _cols, _family(n), "f32", n, (2, n, width), 1, FOUR_WAYS, f"cols n={n} width={width}")


# ---- 2. columns, both precisions, edge widths and batches ---------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("n", EDGE_LENGTHS)
def test_cols_edge_widths(gpu, n, prec):
    """Width 1 and batch 1: the degenerate tile counts; 17 and 33: one column past a tile; 2 and 3: less than any tile."""
    for batch in (1, 3):
        for width in (1, 2, 3, 17, 33):
            _lines(gpu, _cols, _family(n), prec, n, (batch, n, width), 1, [OFFSET, ALIGNED], f"cols n={n} width={width} batch={batch}")


# ---- 3. rows --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("n", EDGE_LENGTHS)
def test_rows(gpu, n, prec):
    """(fp32, odd n: every second row of an aligned buffer is only 8-byte aligned already; the offset moves that to the even rows)"""
    for batch in (1, 2, 37):
        _lines(gpu, _rows, _family(n), prec, n, (batch, n), 1, [OFFSET, ALIGNED], f"rows n={n} batch={batch}")


# ---- 4. four-step lengths: the passes alternate between caller memory and 16-byte-aligned scratch ----------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("n", [8192, 6561, 10000])
def test_four_step(gpu, n, prec):
    from distributedfft_amd import api
    assert api.length_kind(n) == 2
    _lines(gpu, _rows, "four-step", prec, n, (2, n), 1, FOUR_WAYS, f"rows n={n}")
    _lines(gpu, _cols, "four-step", prec, n, (2, n, 4), 1, FOUR_WAYS, f"cols n={n} width=4")
    _lines(gpu, _cols, "four-step", prec, n, (1, n, 3), 1, FOUR_WAYS, f"cols n={n} width=3 batch=1")


# ---- 5. Bluestein ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("n", [11, 1009, 4099])
def test_bluestein(gpu, n, prec):
    """4099: the padded length is above 4096, so a four-step transform runs inside.  Pad, chirp multiply and finish work through scratch:
    `in` must come back untouched."""
    from distributedfft_amd import api
    assert api.length_kind(n) == 3 and (n != 4099 or api.bluestein_length(n) > 4096)
    _lines(gpu, _any(-1), "bluestein", prec, n, (3, n), 1, [OFFSET, ALIGNED], f"any n={n} last axis")
    _lines(gpu, _any(1), "bluestein", prec, n, (2, n, 3), 1, [OFFSET, ALIGNED], f"any n={n} middle axis s=3")
    _lines(gpu, _any(1), "bluestein", prec, n, (2, n, 4), 1, [OFFSET, ALIGNED], f"any n={n} middle axis s=4")


# ---- 6. batched 2-D -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("n1,n2,batch", [(64, 21, 3), (7, 8, 5), (16, 2, 3), (360, 360, 2), (256, 256, 3), (512, 256, 2), (8192, 8, 2)])
def test_fft2d_batch(gpu, n1, n2, batch, prec):
    """(256, 256) and (512, 256) run the one-launch stage in fp64; (8192, 8) the four-step axis route on the 1-D entry points."""
    from distributedfft_amd import _lib, api
    one_launch = (n1, n2) in ((256, 256), (512, 256))
    fam = "2d-one-launch" if one_launch else "2d"
    x, F = A.complex_planes(n1, n2, batch, 7000 + n1)
    refs = {FWD: F, BWD: A.reverse_bins(F, (1, 2))}
    for offs in (OFFSET, ALIGNED):
        for d in (FWD, BWD):
            _one(gpu, lambda t, dd, out: api.fft2d_batch(t, dd, out=out), prec, x, (batch, n1, n2), n2, offs, d,
                 lambda got, tag, d=d: A.check(fam, prec, A.nu(got, refs[d], n1 * n2, prec, (1, 2)), tag), f"fft2 {n1}x{n2}x{batch}")
    if one_launch:
        assert _lib.load().dfft_fft2d_batch_status(None) == 0


# ---- 7. empty batches -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
def test_batch_zero_writes_nothing(gpu, prec):
    """batch == 0 through the C ABI (an empty torch view has no data pointer): DFFT_OK, and not one byte of either buffer changes."""
    import torch
    from distributedfft_amd import _lib as L
    lib = L.load()
    code = L.F64 if prec == "f64" else L.F32
    for off in (1, 0):
        ibuf, iv = M.guarded(0, _cdt(prec), gpu, off, 33)
        obuf, ov = M.guarded(0, _cdt(prec), gpu, off, 33)
        ip = ibuf.data_ptr() + M.view_start(ibuf, iv) * ibuf.element_size()
        op = obuf.data_ptr() + M.view_start(obuf, ov) * obuf.element_size()
        with torch.cuda.device(gpu):
            for a, b in ((ip, op), (op, op)):
                for n in (16, 360, 8192):
                    assert lib.dfft_fft1d_rows(a, b, n, 0, code, FWD, None) == L.OK
                    assert lib.dfft_fft1d_cols(a, b, n, 33, 0, code, BWD, None) == L.OK
                for n, s in ((16, 1), (360, 33), (8192, 3), (11, 1), (1009, 3), (4099, 4)):
                    assert lib.dfft_fft1d_any(a, b, n, s, 0, code, FWD, None) == L.OK
                for n1, n2 in ((7, 8), (256, 256), (8192, 8)):
                    assert lib.dfft_fft2d_batch(a, b, n1, n2, 0, code, BWD, None) == L.OK
            torch.cuda.synchronize()
        M.guards_intact(ibuf, iv, f"batch 0 +{off} (in)")
        M.guards_intact(obuf, ov, f"batch 0 +{off} (out)")


# ---- plans: P virtual devices on one GPU, every caller buffer guarded ---------------------------------------------------------------------
def _run_guarded(gpu, P, make, prepare=None):
    """make(g, comm) -> (plan, ins, outs): lists of (buf, view) pairs of device g's caller buffers, the plan created on the views.
    prepare(g, plan): filters and factors, from device g's thread.  Executes once from P threads and returns the plans (to describe and
    destroy), the buffers and bit copies of the inputs taken before the execute."""
    import torch
    from distributedfft_amd import api
    comm = api.Comm.local(P) if P > 1 else None
    made = [make(g, comm) for g in range(P)]
    keeps = [[v.clone() for _, v in ins] for _, ins, _ in made]
    torch.cuda.synchronize()
    errs = []

    def work(g):
        try:
            if prepare is not None:
                prepare(g, made[g][0])
            made[g][0].execute()
            made[g][0].sync()
        except Exception as e:  # pragma: no cover
            errs.append(e)

    th = [threading.Thread(target=work, args=(g,)) for g in range(P)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    return made, keeps, comm


def _finish(made, comm):
    for plan, _, _ in made:
        plan.destroy()
    if comm:
        comm.destroy()


def _check_guards(made, keeps, tag, in_untouched=True):
    for g, (_, ins, outs) in enumerate(made):
        for k, (buf, view) in enumerate(outs):
            M.guards_intact(buf, view, f"{tag} rank {g} (out {k})")
        for k, (buf, view) in enumerate(ins):
            M.guards_intact(buf, view, f"{tag} rank {g} (in)")
            if in_untouched:
                assert M.bits_equal(view, keeps[g][k]), f"{tag} rank {g}: the execute changed `in`"


# ---- 8. c2c plans -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("flags", [0, 1], ids=["fused", "unfused"])
@pytest.mark.parametrize("direction", [FWD, BWD], ids=["fwd", "bwd"])
@pytest.mark.parametrize("N,P", [((16, 12, 10), 1), ((64, 64, 64), 2), ((25, 10, 16), 4), ((2048, 4, 16), 2), ((8, 2048, 16), 1)])
def test_plan_c2c(gpu, N, P, direction, flags, prec):
    """in / out: exactly get_max_data_count elements inside guarded buffers, aligned and one element off, with the input captured at plan
    time and (DFFT_PLAN_INPUT_FROM_IN) read from `in` at execute, which must then stay bit-equal.  Results as test_plan_3d judges them."""
    from distributedfft_amd import api
    assert flags in (0, api.PLAN_UNFUSED)
    x, F = A.complex_volume(N, 8000 + N[0])
    if direction == FWD:
        inputs, refs = A.split_x(x, P), A.split_bins(F, P)
    else:
        inputs, refs = A.split_bins(x, P), A.split_x(A.reverse_bins(F, (0, 1, 2)), P)
    for off in (1, 0):
        for from_in in (api.PLAN_INPUT_FROM_IN, 0):
            def make(g, comm):
                import torch
                mc = api.get_max_data_count(*N, P, g == P - 1)
                ibuf, iv = M.guarded(mc, _cdt(prec), gpu, off, max(N))
                obuf, ov = M.guarded(mc, _cdt(prec), gpu, off, max(N))
                iv.zero_()
                ov.zero_()
                _load(iv[:inputs[g].size], inputs[g])
                return api.Plan(*N, iv, ov, comm, g, P, direction, flags | from_in), [(ibuf, iv)], [(obuf, ov)]

            made, keeps, comm = _run_guarded(gpu, P, make)
            tag = f"plan {N} P={P} {_sign(direction)} flags={flags | from_in} +{off}"
            _check_guards(made, keeps, tag, in_untouched=bool(from_in))
            pairs = [(made[g][2][0][1][:refs[g].size].cpu().numpy().reshape(refs[g].shape), refs[g]) for g in range(P)]
            _finish(made, comm)
            A.check("3d", prec, A.nu_parts(pairs, N[0] * N[1] * N[2], prec), tag)


# ---- 9. spectral-filter plans at the fused lengths, and r2c plans -------------------------------------------------------------------------
def _conv_make(kind, N, P, prec, gpu, xs, off, K=2):
    from distributedfft_amd import api
    dt = _cdt(prec) if kind == "conv" else _rdt(prec)

    def make(g, comm):
        cnt = api.get_data_count(N, P, g)
        ibuf, iv = M.guarded(cnt, dt, gpu, off, N[2])
        _load(iv, xs[g])
        outs = [M.guarded(cnt, dt, gpu, off, N[2]) for _ in range(K if kind == "multi" else 1)]
        if kind == "conv":
            plan = api.PlanConv(*N, iv, outs[0][1], comm, g, P)
        elif kind == "real":
            plan = api.PlanConvReal(*N, iv, outs[0][1], comm, g, P)
        else:
            plan = api.PlanConvRealMulti(*N, iv, [v for _, v in outs], comm, g, P)
        return plan, [(ibuf, iv)], outs
    return make


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("kind", ["conv", "real", "multi"])
@pytest.mark.parametrize("N,P", [((64, 8, 16), 1), ((64, 8, 16), 2), ((128, 6, 8), 1), ((128, 6, 8), 2)])
def test_filter_plans(gpu, N, P, kind, prec):
    """PlanConv, PlanConvReal and PlanConvRealMulti (K = 2, unit factors: both outputs are the filtered field) at fused X lengths, in / out
    aligned and one element of their own type off; judged as test_conv of test_gpu_accuracy.py.  The fused X stage moves fp32 column pairs
    (16 bytes): where it would touch a caller's 8-byte-aligned buffer -- PlanConv, P = 1, natural layout stores into `out` -- the plan must
    say xconv=multi; every other case keeps the stage it has with aligned buffers."""
    import torch
    real = kind != "conv"
    x, H, ref = A.conv_case(N, real, 9500 + N[0])
    xs = A.split_x(x, P)
    hs = A.split_bins(H, P)
    stage = {}
    for off in (0, 1):
        def prepare(g, plan):
            plan.set_filter(torch.from_numpy(np.ascontiguousarray(hs[g]).reshape(-1)).to(gpu).to(_rdt(prec)))

        made, keeps, comm = _run_guarded(gpu, P, _conv_make(kind, N, P, prec, gpu, xs, off), prepare)
        tag = f"{kind} {N} P={P} +{off}"
        desc = [plan.describe() for plan, _, _ in made]
        _check_guards(made, keeps, tag)
        outs = [[made[g][2][k][1].cpu().numpy().reshape(-1, N[1], N[2]) for g in range(P)] for k in range(len(made[0][2]))]
        _finish(made, comm)
        stage[off] = ["xconv=fused" in t for t in desc]
        assert all(("xconv=fused" in t) != ("xconv=multi" in t) for t in desc), desc
        for k, parts in enumerate(outs):
            A.check("conv", prec, A.nu_parts(list(zip(parts, A.split_x(ref, P))), (N[0] * N[1] * N[2]) ** 2, prec), f"{tag} out {k}")
    assert all(stage[0]), f"{kind} {N} P={P}: aligned buffers must keep the fused X stage"
    caller_memory = kind == "conv" and P == 1 and prec == "f32"       # the only X stage that works on a caller's buffer
    assert stage[1] == [not caller_memory] * P, (kind, N, P, prec, stage)


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("N,P", [((16, 12, 10), 1), ((32, 48, 24), 2)])
def test_plan_r2c_offset(gpu, N, P, prec):
    """Forward r2c plans with the real `in` and the complex `out` one element of their own type off (4 / 8 and 8 / 16 bytes)."""
    from distributedfft_amd import api
    x, F = A.real_volume(N, 9000 + N[0])
    xs, refs = A.split_x(x, P), A.split_bins(F, P)

    def make(g, comm):
        rc, cc = api.r2c_counts(*N, P, g)
        ibuf, iv = M.guarded(rc, _rdt(prec), gpu, 1, N[2])
        obuf, ov = M.guarded(cc, _cdt(prec), gpu, 1, N[0])
        iv.zero_()
        _load(iv[:xs[g].size], xs[g])
        return api.PlanR2C(*N, iv, ov, comm, g, P, api.FORWARD, api.PLAN_INPUT_FROM_IN), [(ibuf, iv)], [(obuf, ov)]

    made, keeps, comm = _run_guarded(gpu, P, make)
    _check_guards(made, keeps, f"r2c plan {N} P={P} +1")
    pairs = [(made[g][2][0][1][:refs[g].size].cpu().numpy().reshape(refs[g].shape), refs[g]) for g in range(P)]
    _finish(made, comm)
    A.check("r2c-3d", prec, A.nu_parts(pairs, N[0] * N[1] * N[2], prec), f"r2c plan {N} P={P} +1")
