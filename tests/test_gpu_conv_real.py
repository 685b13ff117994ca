"""-m gpu: real-field spectral-filter plans (dfft_plan_create_conv_real, api.PlanConvReal) against numpy:
y = irfftn(rfftn(x) * H, s=N, axes=(0, 1, 2)) in float64.

Error measure and bounds are the project's own (tests/test_gpu_conv.py, tests/test_gpu_r2c.py): max|got - ref| / max|ref| below 1e-11 (fp64) /
5e-4 (fp32).  Inputs have unit variance and filters |H| <= 1, so max|ref| stays O(1).  Single-GPU plans, P virtual devices on one GPU
(LOCAL communicator, one thread per device) and one multi-process case on the stream-ordered IPC communicator."""
import os
import subprocess
import sys
import threading
from contextlib import contextmanager
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
TOL = {"f64": 1e-11, "f32": 5e-4}
GUARD = 64
SENT = -12345.0

FUSED_SHAPES = [(128, 16, 32), (256, 8, 32), (384, 8, 16), (512, 8, 32), (768, 4, 16), (1024, 6, 32), (64, 64, 64), (128, 96, 64)]
# Nh = 5 (less than one tile), 3, 16 (exactly two fp64 tiles; the half-length 15 takes the two-launch real rows), 6
WIDTH_SHAPES = [(128, 8, 8), (128, 8, 4), (128, 8, 30), (64, 12, 10)]
MULTI_SHAPES = [(2048, 4, 16), (1000, 8, 16), (343, 8, 8), (20, 36, 40)]
MULTI_GPU = [((64, 64, 64), 2), ((64, 64, 64), 4), ((128, 128, 32), 8), ((10, 10, 8), 4), ((25, 10, 16), 4), ((24, 10, 12), 3), ((1024, 8, 64), 4)]


@contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _rdt(prec):
    import torch
    return torch.float64 if prec == "f64" else torch.float32


def _slab(n, P, g):
    blk = -(-n // P)
    return g * blk, (blk if g < P - 1 else n - (P - 1) * blk)


def _rel(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def _width(nh, prec):
    """The plan's private complex width."""
    g = 8 if prec == "f64" else 16
    while g > 2:
        w = -(-nh // g) * g
        if (w - nh) * 32 <= nh:
            return w
        g //= 2
    return -(-nh // 2) * 2


def _input(N, prec, seed=1):
    x = np.random.default_rng(seed).standard_normal(N)  # unit variance
    return x.astype(np.float32) if prec == "f32" else x


def _hshape(N):
    return (N[0], N[1], N[2] // 2 + 1)


def _filter(N, kind, prec, seed=2):
    """|H| <= 1 on the half spectrum [N0][N1][N2/2+1]: a random complex filter (imaginary parts in the kz = 0 and kz = N2/2 planes
    included: numpy ignores what the Hermitian symmetry forbids, and so must the plan), or a real Gaussian low-pass."""
    if kind == "complex":
        r = np.random.default_rng(seed)
        H = (r.uniform(-1, 1, _hshape(N)) + 1j * r.uniform(-1, 1, _hshape(N))) / np.sqrt(2.0)
        return H.astype(np.complex64) if prec == "f32" else H
    k = [np.fft.fftfreq(N[0]), np.fft.fftfreq(N[1]), np.fft.rfftfreq(N[2])]
    k2 = k[0][:, None, None] ** 2 + k[1][None, :, None] ** 2 + k[2][None, None, :] ** 2
    H = np.exp(-k2 / (2 * 0.15 ** 2))
    return H.astype(np.float32) if prec == "f32" else H


def _split_x(x, P):
    return [np.ascontiguousarray(x[s:s + n]) for s, n in (_slab(x.shape[0], P, g) for g in range(P))]


def _split_bins(X, P):
    """[N0][N1][Nh] -> per device [ys][Nh][N0] (a forward R2C plan's output layout = the filter layout)."""
    return [np.ascontiguousarray(X[:, s:s + n, :].transpose(1, 2, 0)) for s, n in (_slab(X.shape[1], P, g) for g in range(P))]


def _ref(x, H):
    Hd = H.astype(np.complex128 if np.iscomplexobj(H) else np.float64)
    return np.fft.irfftn(np.fft.rfftn(x.astype(np.float64), axes=(0, 1, 2)) * Hd, s=x.shape, axes=(0, 1, 2))


def _run(gpu, N, P, prec, x, H=None, kernel=None, env=None, inplace=False, reps=1, scale=None):
    """P real conv plans (virtual devices on one GPU when P > 1) executed `reps` times from P threads.  Returns the gathered outputs of
    every execute ([N0][N1][N2] each) and the describe() strings; checks the guards behind both buffers and that `in` is left alone."""
    import torch
    from distributedfft_amd import api
    n0, n1, n2 = N
    rdt = _rdt(prec)
    xs_, hs_ = _split_x(x, P), (_split_bins(H, P) if H is not None else None)
    ks_ = _split_x(kernel, P) if kernel is not None else None
    with _env(**(env or {})):
        comm = api.Comm.local(P) if P > 1 else None
        plans, bufs = [], []
        for g in range(P):
            cnt = api.get_data_count(N, P, g)
            a = torch.full((cnt + GUARD,), SENT, dtype=rdt, device=gpu)
            a[:cnt] = torch.from_numpy(xs_[g].reshape(-1)).to(gpu).to(rdt)
            b = a if inplace else torch.full((cnt + GUARD,), SENT, dtype=rdt, device=gpu)
            torch.cuda.synchronize()
            plans.append(api.PlanConvReal(n0, n1, n2, a, None if inplace else b, comm, g, P))
            if scale is not None:
                plans[-1].set_scale(scale)
            bufs.append((a, b, cnt, a.clone()))
    outs = [[None] * P for _ in range(reps)]
    errs = []

    def work(g):
        try:
            a, b, cnt, a0 = bufs[g]
            if hs_ is not None:
                h = torch.from_numpy(hs_[g].reshape(-1)).to(gpu)
                assert h.numel() == api.conv_real_filter_count(n0, n1, n2, P, g)
                plans[g].set_filter(h)
                h.fill_(7.0)  # the plan keeps a private copy: the caller's tensor may be overwritten right away
            else:
                plans[g].set_kernel(torch.from_numpy(ks_[g].reshape(-1)).to(gpu).to(rdt))
            for r in range(reps):
                if inplace and r > 0:
                    a[:cnt] = a0[:cnt]
                    torch.cuda.synchronize()
                plans[g].execute()
                plans[g].sync()
                outs[r][g] = b[:cnt].cpu().numpy().reshape(-1, n1, n2).copy()
        except Exception as e:  # pragma: no cover
            errs.append(e)

    th = [threading.Thread(target=work, args=(g,)) for g in range(P)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    desc = [p.describe() for p in plans]
    for g, (a, b, cnt, a0) in enumerate(bufs):
        assert bool((b[cnt:] == SENT).all()), f"device {g}: the plan wrote past dfft_local_count into out"
        assert bool((a[cnt:] == SENT).all()), f"device {g}: the plan wrote past dfft_local_count into in"
        if not inplace:
            assert torch.equal(a, a0), f"device {g}: an out-of-place execute changed `in`"
    for p in plans:
        p.destroy()
    if comm:
        comm.destroy()
    return [np.concatenate(o, axis=0) for o in outs], desc


def _check(gpu, N, P, prec, kind, env=None, expect=None):
    x, H = _input(N, prec), _filter(N, kind, prec)
    outs, desc = _run(gpu, N, P, prec, x, H, env=env)
    err = _rel(outs[0], _ref(x, H))
    print(f"conv-real {N} P={P} {prec} {kind} {env or ''}: err {err:.3e}  [{desc[0]}]")
    for d in desc:
        assert "pipeline=conv-real" in d and f"filter={kind}" in d and f"width={_width(N[2] // 2 + 1, prec)} " in d, d
        if expect:
            assert f"xconv={expect}" in d, (expect, d)
    assert err < TOL[prec], (N, P, prec, kind, err)
    return outs[0]


@pytest.mark.parametrize("kind", ["complex", "real"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N", FUSED_SHAPES)
def test_conv_real_fused_and_its_multi_twin(gpu, N, prec, kind):
    """Every fused X length on the odd-Nh geometry (N2 % 4 == 0), both precisions and filter kinds: the fused kernel, the DFFT_CONV_FUSED=0
    twin, and the two against each other."""
    fused = _check(gpu, N, 1, prec, kind, expect="fused")
    multi = _check(gpu, N, 1, prec, kind, env={"DFFT_CONV_FUSED": "0"}, expect="multi")
    d = _rel(fused, multi)
    print(f"  fused vs multi {d:.3e}")
    assert d < 2 * TOL[prec], (N, prec, kind, d)


@pytest.mark.parametrize("kind", ["complex", "real"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N", WIDTH_SHAPES)
def test_conv_real_widths(gpu, N, prec, kind):
    _check(gpu, N, 1, prec, kind, expect="fused")


@pytest.mark.parametrize("kind", ["complex", "real"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N", MULTI_SHAPES)
def test_conv_real_multi_route_shapes(gpu, N, prec, kind):
    _check(gpu, N, 1, prec, kind, expect="multi")


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_conv_real_chunked_is_bit_identical(gpu, prec):
    """DFFT_CHUNK_PLANES=3 on 128 planes: 43 Z / Y chunks, the last one 2 planes short."""
    N = (128, 16, 32)
    x, H = _input(N, prec), _filter(N, "complex", prec)
    whole, d0 = _run(gpu, N, 1, prec, x, H)
    parts, d1 = _run(gpu, N, 1, prec, x, H, env={"DFFT_CHUNK_PLANES": "3"})
    assert "chunk_planes=0" in d0[0] and "chunk_planes=3" in d1[0], (d0[0], d1[0])
    assert _rel(whole[0], _ref(x, H)) < TOL[prec]
    assert np.array_equal(whole[0], parts[0])


@pytest.mark.parametrize("kind", ["complex", "real"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N,P", MULTI_GPU)
def test_conv_real_virtual_devices(gpu, N, P, prec, kind):
    _check(gpu, N, P, prec, kind, expect="fused" if N[0] in (64, 128, 1024) else "multi")


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N,P", [((64, 64, 64), 1), ((128, 16, 32), 1), ((20, 36, 40), 1), ((64, 64, 64), 4), ((10, 10, 8), 4)])
def test_conv_real_impulse_kernel_is_a_roll(gpu, N, P, prec):
    """Index conventions, exactly: set_kernel with a unit impulse at (a, b, c) returns np.roll(x, (a, b, c), (0, 1, 2)); at the origin, x."""
    x = _input(N, prec, 5)
    for at in [(0, 0, 0), (3, 5, 2)]:
        k = np.zeros(N, dtype=x.dtype)
        k[at] = 1
        outs, desc = _run(gpu, N, P, prec, x, kernel=k)
        ref = np.roll(x.astype(np.float64), at, (0, 1, 2))
        err = _rel(outs[0], ref)
        print(f"impulse {at} {N} P={P} {prec}: err {err:.3e}")
        assert "filter=complex" in desc[0]
        assert err < TOL[prec], (N, P, prec, at, err)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N,P", [((128, 96, 64), 1), ((1000, 8, 16), 1), ((64, 64, 64), 2), ((25, 10, 16), 4)])
def test_conv_real_set_kernel_equals_set_filter_of_r2c_plan(gpu, N, P, prec):
    """The documented filter layout IS the forward R2C plan's output layout: set_kernel(k) and set_filter(api.PlanR2C forward of k) agree."""
    import torch
    from distributedfft_amd import api
    x = _input(N, prec, 6)
    k = (np.random.default_rng(7).standard_normal(N) / np.sqrt(float(np.prod(N)))).astype(x.dtype)  # |rfftn(k)| = O(1)
    a, _ = _run(gpu, N, P, prec, x, kernel=k)
    rdt, cdt = _rdt(prec), (torch.complex128 if prec == "f64" else torch.complex64)
    nh = N[2] // 2 + 1
    comm = api.Comm.local(P) if P > 1 else None
    plans, res = [], []
    for g in range(P):
        rc, cc = api.r2c_counts(*N, P, g)
        i = torch.from_numpy(_split_x(k, P)[g].reshape(-1)).to(gpu).to(rdt)
        assert i.numel() == rc
        o = torch.zeros(cc, dtype=cdt, device=gpu)
        torch.cuda.synchronize()
        plans.append(api.PlanR2C(*N, i, o, comm, g, P, api.FORWARD))
        res.append(o)
    th = [threading.Thread(target=lambda p=p: (p.execute(), p.sync())) for p in plans]
    [t.start() for t in th]
    [t.join() for t in th]
    ys = [_slab(N[1], P, g)[1] for g in range(P)]
    Hs = [res[g][:ys[g] * nh * N[0]].cpu().numpy().reshape(ys[g], nh, N[0]) for g in range(P)]
    for p in plans:
        p.destroy()
    if comm:
        comm.destroy()
    H = np.concatenate([h.transpose(2, 0, 1) for h in Hs], axis=1)  # back to [N0][N1][Nh]
    b, _ = _run(gpu, N, P, prec, x, H)
    ref = _ref(x, np.fft.rfftn(k.astype(np.float64), axes=(0, 1, 2)))
    ea, eb, d = _rel(a[0], ref), _rel(b[0], ref), _rel(a[0], b[0])
    print(f"set_kernel {ea:.3e} set_filter(R2C plan) {eb:.3e} difference {d:.3e}")
    assert ea < TOL[prec] and eb < TOL[prec] and d < TOL[prec], (N, P, prec, ea, eb, d)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N,P", [((64, 64, 64), 1), ((128, 96, 64), 1), ((64, 64, 64), 4)])
def test_conv_real_filter_solves_poisson(gpu, N, P, prec):
    """H = -1/|k|^2 (0 at k = 0) applied to f = -|k0|^2 sin(k0 . r) returns sin(k0 . r) -- on a real tensor."""
    m = [np.fft.fftfreq(N[0], 1.0 / N[0]), np.fft.fftfreq(N[1], 1.0 / N[1]), np.fft.rfftfreq(N[2], 1.0 / N[2])]  # integer wavenumbers: |H| <= 1
    k2 = m[0][:, None, None] ** 2 + m[1][None, :, None] ** 2 + m[2][None, None, :] ** 2
    H = np.zeros(_hshape(N))
    H[k2 > 0] = -1.0 / k2[k2 > 0]
    k0 = (1, 2, 1)
    r = [2 * np.pi * np.arange(n) / n for n in N]
    u = np.sin(k0[0] * r[0][:, None, None] + k0[1] * r[1][None, :, None] + k0[2] * r[2][None, None, :])
    f = -float(sum(k * k for k in k0)) * u
    if prec == "f32":
        H, f = H.astype(np.float32), f.astype(np.float32)
    outs, desc = _run(gpu, N, P, prec, f, H)
    err = _rel(outs[0], u)
    print(f"poisson {N} P={P} {prec}: err {err:.3e} [{desc[0]}]")
    assert "filter=real" in desc[0]
    assert err < TOL[prec], (N, P, prec, err)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N", [(128, 96, 64), (20, 36, 40)])
def test_conv_real_gaussian_agrees_with_the_c2c_plan_on_the_widened_field(gpu, N, prec):
    """An even real filter: api.PlanConv on the field widened to complex returns the same real part (within twice the bound) and an
    imaginary part below the bound."""
    import torch
    from distributedfft_amd import api
    x = _input(N, prec)
    k = [np.fft.fftfreq(n) for n in N]
    k2 = k[0][:, None, None] ** 2 + k[1][None, :, None] ** 2 + k[2][None, None, :] ** 2
    Hfull = np.exp(-k2 / (2 * 0.15 ** 2)).astype(x.dtype)
    Hhalf = np.ascontiguousarray(Hfull[:, :, :N[2] // 2 + 1])
    got, _ = _run(gpu, N, 1, prec, x, Hhalf)
    cdt = torch.complex128 if prec == "f64" else torch.complex64
    a = torch.from_numpy(x.reshape(-1)).to(gpu).to(cdt)
    b = torch.zeros_like(a)
    torch.cuda.synchronize()
    p = api.PlanConv(*N, a, b, None, 0, 1)
    p.set_filter(torch.from_numpy(np.ascontiguousarray(Hfull.transpose(1, 2, 0)).reshape(-1)).to(gpu))
    p.execute()
    p.sync()
    c2c = b.cpu().numpy().reshape(N)
    p.destroy()
    scale = np.abs(c2c).max()
    d, im = _rel(got[0], c2c.real), float(np.abs(c2c.imag).max() / scale)
    print(f"real vs C2C {N} {prec}: real parts {d:.3e}, C2C imaginary part {im:.3e}")
    assert _rel(got[0], _ref(x, Hhalf)) < TOL[prec]
    assert d < 2 * TOL[prec] and im < TOL[prec], (N, prec, d, im)


@pytest.mark.parametrize("N,P", [((128, 16, 32), 1), ((20, 36, 40), 1), ((64, 64, 64), 2)])
def test_conv_real_inplace_and_repeats_are_bit_identical(gpu, N, P):
    x, H = _input(N, "f64"), _filter(N, "complex", "f64")
    oop, _ = _run(gpu, N, P, "f64", x, H, reps=10)
    for r in range(1, 10):
        assert np.array_equal(oop[0], oop[r]), f"execute {r} differs from execute 0"
    inp, _ = _run(gpu, N, P, "f64", x, H, inplace=True, reps=2)
    assert np.array_equal(oop[0], inp[0]) and np.array_equal(oop[0], inp[1]), "in place differs from out of place"


def test_conv_real_contract(gpu):
    """Replacing the filter, set_scale's documented rule, execute without a filter, stage_times, tune / kernel_times / buffer accessors."""
    import time

    import torch
    from distributedfft_amd import _lib as L
    from distributedfft_amd import api
    N = (128, 16, 32)
    cnt = int(np.prod(N))
    x, H1, H2 = _input(N, "f64"), _filter(N, "complex", "f64"), _filter(N, "real", "f64")
    a = torch.from_numpy(x.reshape(-1)).to(gpu)
    b = torch.zeros(cnt, dtype=torch.float64, device=gpu)
    torch.cuda.synchronize()
    p = api.PlanConvReal(*N, a, b, None, 0, 1)
    assert "pipeline=conv-real" in p.describe() and "filter=unset" in p.describe()
    with pytest.raises(L.DfftError) as e:
        p.execute()
    assert e.value.code == L.EINVAL and "filter" in str(e.value)
    p.tune()  # a no-op
    with pytest.raises(L.DfftError) as e:
        p.kernel_times()
    assert e.value.code == L.EUNSUPPORTED
    lib = L.load()
    assert not lib.dfft_plan_buffer1(p.handle) and not lib.dfft_plan_result(p.handle) and not lib.dfft_plan_workbuf(p.handle, None)
    assert p.stream != 0

    def run(flags=api.EXEC_ASYNC):
        p.execute(flags)
        p.sync()
        return b.cpu().numpy().reshape(N).copy()

    p.set_filter(torch.from_numpy(_split_bins(H1, 1)[0].reshape(-1)).to(gpu))
    assert "filter=complex" in p.describe()
    y1 = run()
    assert _rel(y1, _ref(x, H1)) < TOL["f64"]
    t = p.stage_times()
    assert len(t) == 4 and all(v >= 0 for v in t), t
    # the four stages lie inside the execute: their sum is within the wall time of an ASYNC execute + sync
    t0 = time.perf_counter()
    p.execute()
    p.sync()
    wall = time.perf_counter() - t0
    t = p.stage_times()
    assert all(v >= 0 for v in t) and sum(t) <= wall, (t, wall)
    ts = run(api.EXEC_SYNC_STAGES)
    assert np.array_equal(ts, y1)
    assert len(p.stage_times()) == 4
    run(api.EXEC_NO_TIMING)
    with pytest.raises(L.DfftError):
        p.stage_times()
    # a new filter (now a real one) between executes: the copy's bytes are re-read as reals, its padding must still read as zero
    p.set_filter(torch.from_numpy(_split_bins(H2, 1)[0].reshape(-1)).to(gpu))
    assert "filter=real" in p.describe()
    y2 = run()
    assert _rel(y2, _ref(x, H2)) < TOL["f64"]
    # ... and back to a complex one
    p.set_filter(torch.from_numpy(_split_bins(H1, 1)[0].reshape(-1)).to(gpu))
    assert np.array_equal(run(), y1)
    p.set_filter(torch.from_numpy(_split_bins(H2, 1)[0].reshape(-1)).to(gpu))
    assert np.array_equal(run(), y2)
    # set_scale takes effect at the next set_filter / set_kernel (the stored copy is not re-folded)
    p.set_scale(2.0)
    assert np.array_equal(run(), y2)
    p.set_filter(torch.from_numpy(_split_bins(H2, 1)[0].reshape(-1)).to(gpu))
    y3 = run()
    assert _rel(y3, 2.0 * _ref(x, H2)) < TOL["f64"] and np.array_equal(y3, 2.0 * y2)
    p.destroy()


def test_conv_real_beyond_the_infinity_cache(gpu):
    """(512, 512, 512) fp32 with a real filter: a 539 MB spectrum, chunked Z / Y stages, Nh = 257 at width 264."""
    N, prec = (512, 512, 512), "f32"
    x, H = _input(N, prec), _filter(N, "real", prec)
    outs, desc = _run(gpu, N, 1, prec, x, H)
    err = _rel(outs[0], _ref(x, H))
    print(f"conv-real {N} {prec} real: err {err:.3e}  [{desc[0]}]")
    assert "xconv=fused" in desc[0] and "width=264 " in desc[0] and "chunk_planes=0" not in desc[0], desc[0]
    assert err < TOL[prec], (N, prec, err)


WORKER = r'''
import os, sys
import numpy as np, torch
sys.path.insert(0, os.environ["DFFT_ROOT"])
from distributedfft_amd import api
N = (64, 20, 40)
rank, P = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
n0, n1, n2 = N
nh = n2 // 2 + 1
dev = torch.device("cuda:0")
torch.cuda.set_device(0)
comm = api.Comm.ipc(P, rank, True)
r = np.random.default_rng(11)                                   # same arrays on every rank
x = r.standard_normal(N)
H = (r.uniform(-1, 1, (n0, n1, nh)) + 1j * r.uniform(-1, 1, (n0, n1, nh))) / np.sqrt(2.0)
ref = np.fft.irfftn(np.fft.rfftn(x, axes=(0, 1, 2)) * H, s=N, axes=(0, 1, 2))
xb = -(-n0 // P); x0 = rank * xb; xs = min(xb, n0 - x0)
yb = -(-n1 // P); y0 = rank * yb; ys = min(yb, n1 - y0)
a = torch.from_numpy(np.ascontiguousarray(x[x0:x0 + xs]).reshape(-1)).to(dev)
b = torch.zeros_like(a)
torch.cuda.synchronize()
p = api.PlanConvReal(n0, n1, n2, a, b, comm, rank, P)           # collective
p.set_filter(torch.from_numpy(np.ascontiguousarray(H[:, y0:y0 + ys, :].transpose(1, 2, 0)).reshape(-1)).to(dev))
p.execute(); p.sync()
e1 = float(np.abs(b.cpu().numpy().reshape(xs, n1, n2) - ref[x0:x0 + xs]).max() / np.abs(ref).max())
k = np.zeros(N); k[2, 3, 4] = 1
p.set_kernel(torch.from_numpy(np.ascontiguousarray(k[x0:x0 + xs]).reshape(-1)).to(dev))   # collective
p.execute(); p.sync()
roll = np.roll(x, (2, 3, 4), (0, 1, 2))
e2 = float(np.abs(b.cpu().numpy().reshape(xs, n1, n2) - roll[x0:x0 + xs]).max() / np.abs(roll).max())
d = p.describe()
p.destroy()                                                      # collective
comm.destroy()
print(f"rank {rank} conv-real {e1:.3e} roll {e2:.3e} [{d}] done", flush=True)
assert e1 < 1e-11 and e2 < 1e-11, (e1, e2)
'''


def test_conv_real_two_processes_ipc_async(gpu, tmp_path):
    """P = 2 across real process boundaries: two ranks share cuda:0 on the stream-ordered IPC communicator."""
    import socket
    import time
    script = tmp_path / "conv_real_worker.py"
    script.write_text(WORKER)
    port = None
    for _ in range(64):
        s, s2 = socket.socket(), socket.socket()
        s.bind(("127.0.0.1", 0))
        cand = s.getsockname()[1]
        try:
            s2.bind(("127.0.0.1", cand + 1))
            port = cand
        except OSError:
            pass
        finally:
            s.close()
            s2.close()
        if port:
            break
    assert port
    procs, logs = [], []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   DFFT_ROOT=str(ROOT), HSA_ENABLE_IPC_MODE_LEGACY="0", DFFT_EXCHANGE="ipc-async")
        env.pop("DFFT_MASTER_PORT", None)
        log = open(tmp_path / f"rank{r}.log", "w+")
        logs.append(log)
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=log, stderr=subprocess.STDOUT, cwd=str(ROOT)))
    t_end = time.monotonic() + 240
    failed_at = None
    while any(p.poll() is None for p in procs):
        now = time.monotonic()
        if failed_at is None and any(p.poll() not in (None, 0) for p in procs):
            failed_at = now
        if now > t_end or (failed_at is not None and now > failed_at + 10):
            for p in procs:
                if p.poll() is None:
                    p.kill()
            break
        time.sleep(0.1)
    for p in procs:
        p.wait()
    text = []
    for log in logs:
        log.seek(0)
        text.append(log.read())
        log.close()
    assert all(p.returncode == 0 for p in procs), "\n".join(f"--- rank {r} rc={p.returncode}\n{t[-2000:]}" for r, (p, t) in enumerate(zip(procs, text)))
    assert all("done" in t for t in text)
