"""-m gpu: spectral-filter plans (dfft_plan_create_conv, api.PlanConv) against numpy: y = ifftn(fftn(x) * H) in fp64.

Error measure and bounds are the project's own (tests/test_gpu_r2c.py): max|got - ref| / max|ref| below 1e-11 (fp64) / 5e-4 (fp32).  Inputs have
unit variance and filters |H| <= 1, so max|ref| stays O(1).  Single-GPU plans, P virtual devices on one GPU (LOCAL communicator, one thread
per device) and one multi-process case on the IPC communicator."""
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

FUSED_SHAPES = [(128, 16, 32), (256, 8, 32), (384, 8, 16), (512, 8, 32), (768, 4, 16), (1024, 6, 32), (64, 64, 64), (128, 128, 128), (128, 96, 64)]
MULTI_SHAPES = [(2048, 4, 16), (1000, 8, 16), (343, 8, 8), (20, 36, 40), (512, 8, 9)]
MULTI_GPU = [((64, 64, 64), 2, {}), ((64, 64, 64), 4, {}), ((128, 128, 32), 8, {}), ((10, 10, 8), 4, {}), ((25, 10, 16), 4, {}), ((24, 10, 12), 4, {}),
             ((24, 10, 12), 3, {}), ((1024, 8, 64), 4, {}), ((512, 8, 32), 2, {"DFFT_ROT": "1"})]


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


def _cdt(prec):
    import torch
    return torch.complex128 if prec == "f64" else torch.complex64


def _slab(n, P, g):
    blk = -(-n // P)
    return g * blk, (blk if g < P - 1 else n - (P - 1) * blk)


def _rel(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def _input(N, prec, seed=1):
    r = np.random.default_rng(seed)
    x = (r.standard_normal(N) + 1j * r.standard_normal(N)) / np.sqrt(2.0)  # unit variance
    return x.astype(np.complex64) if prec == "f32" else x


def _filter(N, kind, prec, seed=2):
    """|H| <= 1: a random complex filter, or a real Gaussian low-pass."""
    if kind == "complex":
        r = np.random.default_rng(seed)
        H = (r.uniform(-1, 1, N) + 1j * r.uniform(-1, 1, N)) / np.sqrt(2.0)
        return H.astype(np.complex64) if prec == "f32" else H
    k = [np.fft.fftfreq(n) for n in N]
    k2 = k[0][:, None, None] ** 2 + k[1][None, :, None] ** 2 + k[2][None, None, :] ** 2
    H = np.exp(-k2 / (2 * 0.15 ** 2))
    return H.astype(np.float32) if prec == "f32" else H


def _split_x(x, P):
    return [np.ascontiguousarray(x[s:s + n]) for s, n in (_slab(x.shape[0], P, g) for g in range(P))]


def _split_bins(X, P):
    """[N0][N1][N2] -> per device [ys][N2][N0] (a forward plan's output layout = the filter layout)."""
    return [np.ascontiguousarray(X[:, s:s + n, :].transpose(1, 2, 0)) for s, n in (_slab(X.shape[1], P, g) for g in range(P))]


def _ref(x, H):
    return np.fft.ifftn(np.fft.fftn(x.astype(np.complex128)) * H.astype(np.complex128 if np.iscomplexobj(H) else np.float64))


def _run(gpu, N, P, prec, x, H=None, kernel=None, env=None, inplace=False, reps=1, scale=None):
    """P conv plans (virtual devices on one GPU when P > 1) executed `reps` times from P threads.  Returns the gathered outputs of every
    execute ([N0][N1][N2] each), the describe() strings and the input buffers' contents afterwards."""
    import torch
    from distributedfft_amd import api
    n0, n1, n2 = N
    cdt = _cdt(prec)
    xs_, hs_ = _split_x(x, P), (_split_bins(H, P) if H is not None else None)
    ks_ = _split_x(kernel, P) if kernel is not None else None
    with _env(**(env or {})):
        comm = api.Comm.local(P) if P > 1 else None
        plans, bufs = [], []
        for g in range(P):
            cnt = api.get_data_count(N, P, g)
            a = torch.full((cnt + GUARD,), SENT, dtype=cdt, device=gpu)
            a[:cnt] = torch.from_numpy(xs_[g].reshape(-1)).to(gpu).to(cdt)
            b = a if inplace else torch.full((cnt + GUARD,), SENT, dtype=cdt, device=gpu)
            torch.cuda.synchronize()
            plans.append(api.PlanConv(n0, n1, n2, a, None if inplace else b, comm, g, P))
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
                plans[g].set_filter(h)
                h.fill_(7.0)  # the plan keeps a private copy: the caller's tensor may be overwritten right away
            else:
                plans[g].set_kernel(torch.from_numpy(ks_[g].reshape(-1)).to(gpu).to(cdt))
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
        assert bool((b[cnt:].real == SENT).all()), f"device {g}: the plan wrote past dfft_local_count into out"
        assert bool((a[cnt:].real == SENT).all()), f"device {g}: the plan wrote past dfft_local_count into in"
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
    ref = _ref(x, H)
    err = _rel(outs[0], ref)
    print(f"conv {N} P={P} {prec} {kind} {env or ''}: err {err:.3e}  [{desc[0]}]")
    assert "pipeline=conv" in desc[0] and f"filter={kind}" in desc[0], desc[0]
    if expect:
        assert all(f"xconv={expect}" in d for d in desc), (expect, desc[0])
    assert err < TOL[prec], (N, P, prec, kind, err)
    return outs[0]


@pytest.mark.parametrize("kind", ["complex", "real"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N", FUSED_SHAPES)
def test_conv_fused_and_its_multi_twin(gpu, N, prec, kind):
    """Every required fused X length, the cubes and (128, 96, 64): the fused kernel, the DFFT_CONV_FUSED=0 twin, and the two against each other."""
    fused = _check(gpu, N, 1, prec, kind, expect="fused")
    multi = _check(gpu, N, 1, prec, kind, env={"DFFT_CONV_FUSED": "0"}, expect="multi")
    d = _rel(fused, multi)
    print(f"  fused vs multi {d:.3e}")
    assert d < 2 * TOL[prec], (N, prec, kind, d)


@pytest.mark.parametrize("kind", ["complex", "real"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N", MULTI_SHAPES)
def test_conv_multi_route_shapes(gpu, N, prec, kind):
    # (512, 8, 9): a fused X length with an odd N2 -- no fp32 column pairs, so fp32 takes the multi route; fp64 tiles may be ragged
    expect = "fused" if (N == (512, 8, 9) and prec == "f64") else "multi"
    _check(gpu, N, 1, prec, kind, expect=expect)


@pytest.mark.parametrize("kind", ["complex", "real"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N,P,env", MULTI_GPU)
def test_conv_virtual_devices(gpu, N, P, env, prec, kind):
    x, H = _input(N, prec), _filter(N, kind, prec)
    outs, desc = _run(gpu, N, P, prec, x, H, env=env)
    err = _rel(outs[0], _ref(x, H))
    print(f"conv {N} P={P} {prec} {kind}: err {err:.3e}  [{desc[0]}]")
    if env.get("DFFT_ROT") == "1":
        assert "rotated_exchange_rows=0" not in desc[0] and "xconv=fused" in desc[0], desc[0]
    assert err < TOL[prec], (N, P, prec, kind, err)


@pytest.mark.parametrize("N,prec,kind", [((256, 256, 256), "f64", "complex"), ((512, 512, 512), "f64", "real"), ((512, 512, 512), "f32", "complex")])
def test_conv_full_size(gpu, N, prec, kind):
    """Slabs beyond the Infinity Cache: the one-launch YZ stage where the C2C plan uses it, and at 512^3 fp64 the padded hand-over buffer
    (the X stage in place on it, the filter copy in its padded layout, the inverse YZ stage rows first)."""
    x, H = _input(N, prec), _filter(N, kind, prec)
    outs, desc = _run(gpu, N, 1, prec, x, H)
    err = _rel(outs[0], _ref(x, H))
    print(f"conv {N} {prec} {kind}: err {err:.3e}  [{desc[0]}]")
    assert "xconv=fused" in desc[0], desc[0]
    if N == (512, 512, 512) and prec == "f64":
        assert "handover=padded-buffer" in desc[0] and "yz_stage=one-launch" in desc[0], desc[0]
    assert err < TOL[prec], (N, prec, kind, err)


def test_conv_rotated_rows_multi_twin(gpu):
    """DFFT_CONV_FUSED=0 with DFFT_ROT=1: the multi route keeps plain rows in the exchange buffers (documented) and computes the same."""
    N, P = (512, 8, 32), 2
    x, H = _input(N, "f64"), _filter(N, "complex", "f64")
    a, da = _run(gpu, N, P, "f64", x, H, env={"DFFT_ROT": "1"})
    b, db = _run(gpu, N, P, "f64", x, H, env={"DFFT_ROT": "1", "DFFT_CONV_FUSED": "0"})
    assert "xconv=multi" in db[0] and "rotated_exchange_rows=0" in db[0], db[0]
    assert _rel(b[0], _ref(x, H)) < TOL["f64"] and _rel(a[0], b[0]) < 2 * TOL["f64"]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N,P", [((64, 64, 64), 1), ((128, 16, 32), 1), ((20, 36, 40), 1), ((64, 64, 64), 4), ((10, 10, 8), 4)])
def test_conv_impulse_kernel_is_a_roll(gpu, N, P, prec):
    """Index conventions, exactly: set_kernel with a unit impulse at (a, b, c) returns np.roll(x, (a, b, c), (0, 1, 2)); at the origin, x."""
    x = _input(N, prec, 5)
    for at in [(0, 0, 0), (3, 5, 2)]:
        k = np.zeros(N, dtype=x.dtype)
        k[at] = 1
        outs, _ = _run(gpu, N, P, prec, x, kernel=k)
        ref = np.roll(x.astype(np.complex128), at, (0, 1, 2))
        err = _rel(outs[0], ref)
        print(f"impulse {at} {N} P={P} {prec}: err {err:.3e}")
        assert err < TOL[prec], (N, P, prec, at, err)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N,P", [((128, 96, 64), 1), ((1000, 8, 16), 1), ((64, 64, 64), 2), ((25, 10, 16), 4)])
def test_conv_set_kernel_equals_set_filter_of_forward_plan(gpu, N, P, prec):
    """The documented filter layout IS the forward plan's output layout: set_kernel(k) and set_filter(api.Plan forward of k) agree."""
    import torch
    from distributedfft_amd import api
    x = _input(N, prec, 6)
    r = np.random.default_rng(7)
    k = (r.standard_normal(N) + 1j * r.standard_normal(N)) / np.sqrt(2.0 * np.prod(N))  # |fftn(k)| = O(1)
    k = k.astype(x.dtype)
    a, _ = _run(gpu, N, P, prec, x, kernel=k)
    # H by the existing forward plans, per device
    cdt = _cdt(prec)
    comm = api.Comm.local(P) if P > 1 else None
    plans, res = [], []
    for g in range(P):
        mc = api.get_max_data_count(*N, P, g == P - 1)
        i = torch.zeros(mc, dtype=cdt, device=gpu)
        src = _split_x(k, P)[g].reshape(-1)
        i[:src.size] = torch.from_numpy(src).to(gpu)
        o = torch.zeros(mc, dtype=cdt, device=gpu)
        torch.cuda.synchronize()
        plans.append(api.Plan(*N, i, o, comm, g, P, api.FORWARD))
        res.append(o)
    th = [threading.Thread(target=lambda p=p: (p.execute(), p.sync())) for p in plans]
    [t.start() for t in th]
    [t.join() for t in th]
    ys = [_slab(N[1], P, g)[1] for g in range(P)]
    Hs = [res[g][:ys[g] * N[2] * N[0]].cpu().numpy().reshape(ys[g], N[2], N[0]) for g in range(P)]
    for p in plans:
        p.destroy()
    if comm:
        comm.destroy()
    H = np.concatenate([h.transpose(2, 0, 1) for h in Hs], axis=1)  # back to [N0][N1][N2]
    b, _ = _run(gpu, N, P, prec, x, H)
    ref = _ref(x, np.fft.fftn(k.astype(np.complex128)))
    ea, eb, d = _rel(a[0], ref), _rel(b[0], ref), _rel(a[0], b[0])
    print(f"set_kernel {ea:.3e} set_filter(forward plan) {eb:.3e} difference {d:.3e}")
    assert ea < TOL[prec] and eb < TOL[prec] and d < TOL[prec], (N, P, prec, ea, eb, d)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N,P", [((64, 64, 64), 1), ((128, 96, 64), 1), ((64, 64, 64), 4)])
def test_conv_real_filter_solves_poisson(gpu, N, P, prec):
    """H = -1/|k|^2 (0 at k = 0) applied to f = -|k0|^2 sin(k0 . r) returns sin(k0 . r)."""
    m = [np.fft.fftfreq(n, 1.0 / n) for n in N]  # integer wavenumbers of the 2 pi-periodic box: |H| <= 1
    k2 = m[0][:, None, None] ** 2 + m[1][None, :, None] ** 2 + m[2][None, None, :] ** 2
    H = np.zeros(N)
    H[k2 > 0] = -1.0 / k2[k2 > 0]
    k0 = (1, 2, 1)
    r = [2 * np.pi * np.arange(n) / n for n in N]
    u = np.sin(k0[0] * r[0][:, None, None] + k0[1] * r[1][None, :, None] + k0[2] * r[2][None, None, :])
    f = -float(sum(k * k for k in k0)) * u
    if prec == "f32":
        H, f = H.astype(np.float32), f.astype(np.float32)
    outs, desc = _run(gpu, N, P, prec, f.astype(np.complex64 if prec == "f32" else np.complex128), H)
    err = _rel(outs[0], u)
    print(f"poisson {N} P={P} {prec}: err {err:.3e} [{desc[0]}]")
    assert "filter=real" in desc[0]
    assert err < TOL[prec], (N, P, prec, err)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N", [(128, 96, 64), (512, 8, 32), (20, 36, 40)])
def test_conv_vs_composed_route(gpu, N, prec):
    """Plan forward -> torch.mul by H in the result layout -> Plan backward with set_scale(1/N): agreement within twice the bound."""
    import torch
    from distributedfft_amd import api
    x, H = _input(N, prec), _filter(N, "complex", prec)
    got, _ = _run(gpu, N, 1, prec, x, H)
    cdt = _cdt(prec)
    cnt = int(np.prod(N))
    a = torch.from_numpy(x.reshape(-1)).to(gpu).to(cdt)
    b, c = torch.zeros(cnt, dtype=cdt, device=gpu), torch.zeros(cnt, dtype=cdt, device=gpu)
    h = torch.from_numpy(_split_bins(H, 1)[0].reshape(-1)).to(gpu).to(cdt)
    torch.cuda.synchronize()
    f = api.Plan(*N, a, b, None, 0, 1, api.FORWARD, api.PLAN_INPUT_FROM_IN)
    f.execute()
    f.sync()
    b.mul_(h)
    torch.cuda.synchronize()
    q = api.Plan(*N, b, c, None, 0, 1, api.BACKWARD, api.PLAN_INPUT_FROM_IN)
    q.set_scale(1.0 / cnt)
    q.execute()
    q.sync()
    comp = c.cpu().numpy().reshape(N)
    f.destroy()
    q.destroy()
    d = _rel(got[0], comp)
    print(f"conv vs composed {N} {prec}: {d:.3e}")
    assert d < 2 * TOL[prec], (N, prec, d)


@pytest.mark.parametrize("N,P", [((128, 16, 32), 1), ((20, 36, 40), 1), ((64, 64, 64), 2)])
def test_conv_inplace_and_repeats_are_bit_identical(gpu, N, P):
    x, H = _input(N, "f64"), _filter(N, "complex", "f64")
    oop, _ = _run(gpu, N, P, "f64", x, H, reps=10)
    for r in range(1, 10):
        assert np.array_equal(oop[0], oop[r]), f"execute {r} differs from execute 0"
    inp, _ = _run(gpu, N, P, "f64", x, H, inplace=True, reps=2)
    assert np.array_equal(oop[0], inp[0]) and np.array_equal(oop[0], inp[1]), "in place differs from out of place"


def test_conv_plan_created_and_destroyed_without_an_execute(gpu):
    """Both half plans, the shared stream and the send-less P = 1 handle go away cleanly when nothing has run; the input is untouched."""
    import torch
    from distributedfft_amd import api
    N = (16, 6, 8)
    x = _input(N, "f64")
    a = torch.from_numpy(x.reshape(-1)).to(gpu)
    b = torch.zeros(int(np.prod(N)), dtype=torch.complex128, device=gpu)
    torch.cuda.synchronize()
    p = api.PlanConv(*N, a, b, None, 0, 1)
    assert "pipeline=conv " in p.describe() and "filter=unset" in p.describe()
    p.destroy()  # raises on any return code but DFFT_OK
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), x.reshape(-1)) and not bool(b.any())


def test_conv_contract(gpu):
    """Replacing the filter, set_scale's documented rule, execute without a filter, stage_times, tune / kernel_times / buffer accessors."""
    import torch
    from distributedfft_amd import _lib as L
    from distributedfft_amd import api
    N = (128, 16, 32)
    cnt = int(np.prod(N))
    x, H1, H2 = _input(N, "f64"), _filter(N, "complex", "f64"), _filter(N, "real", "f64")
    a = torch.from_numpy(x.reshape(-1)).to(gpu)
    b = torch.zeros(cnt, dtype=torch.complex128, device=gpu)
    torch.cuda.synchronize()
    p = api.PlanConv(*N, a, b, None, 0, 1)
    assert "filter=unset" in p.describe()
    with pytest.raises(L.DfftError) as e:
        p.execute()
    assert e.value.code == L.EINVAL and "filter" in str(e.value)
    p.tune()  # a no-op
    with pytest.raises(L.DfftError) as e:
        p.kernel_times()
    assert e.value.code == L.EUNSUPPORTED
    assert not L.load().dfft_plan_buffer1(p.handle) and not L.load().dfft_plan_result(p.handle)
    assert p.stream != 0

    def run(flags=api.EXEC_ASYNC):
        p.execute(flags)
        p.sync()
        return b.cpu().numpy().reshape(N).copy()

    p.set_filter(torch.from_numpy(_split_bins(H1, 1)[0].reshape(-1)).to(gpu))
    y1 = run()
    assert _rel(y1, _ref(x, H1)) < TOL["f64"]
    t = p.stage_times()
    assert len(t) == 4 and all(v >= 0 for v in t), t
    # the four stages lie inside the execute: their sum is within the wall time of an ASYNC execute + sync
    import time
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
    # a new filter (now a real one) between executes
    p.set_filter(torch.from_numpy(_split_bins(H2, 1)[0].reshape(-1)).to(gpu))
    assert "filter=real" in p.describe()
    y2 = run()
    assert _rel(y2, _ref(x, H2)) < TOL["f64"]
    # set_scale takes effect at the next set_filter / set_kernel (the stored copy is not re-folded)
    p.set_scale(2.0)
    assert np.array_equal(run(), y2)
    p.set_filter(torch.from_numpy(_split_bins(H2, 1)[0].reshape(-1)).to(gpu))
    y3 = run()
    assert _rel(y3, 2.0 * _ref(x, H2)) < TOL["f64"] and np.array_equal(y3, 2.0 * y2)
    p.destroy()


WORKER = r'''
import os, sys
import numpy as np, torch
sys.path.insert(0, os.environ["DFFT_ROOT"])
from distributedfft_amd import api
N = (64, 20, 40)
rank, P = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
n0, n1, n2 = N
dev = torch.device("cuda:0")
torch.cuda.set_device(0)
comm = api.Comm.ipc(P, rank, True)
r = np.random.default_rng(11)                                   # same arrays on every rank
x = (r.standard_normal(N) + 1j * r.standard_normal(N)) / np.sqrt(2.0)
H = (r.uniform(-1, 1, N) + 1j * r.uniform(-1, 1, N)) / np.sqrt(2.0)
ref = np.fft.ifftn(np.fft.fftn(x) * H)
xb = -(-n0 // P); x0 = rank * xb; xs = min(xb, n0 - x0)
yb = -(-n1 // P); y0 = rank * yb; ys = min(yb, n1 - y0)
a = torch.from_numpy(np.ascontiguousarray(x[x0:x0 + xs]).reshape(-1)).to(dev)
b = torch.zeros_like(a)
torch.cuda.synchronize()
p = api.PlanConv(n0, n1, n2, a, b, comm, rank, P)               # collective
p.set_filter(torch.from_numpy(np.ascontiguousarray(H[:, y0:y0 + ys, :].transpose(1, 2, 0)).reshape(-1)).to(dev))
p.execute(); p.sync()
e1 = float(np.abs(b.cpu().numpy().reshape(xs, n1, n2) - ref[x0:x0 + xs]).max() / np.abs(ref).max())
k = np.zeros(N, dtype=np.complex128); k[2, 3, 4] = 1
p.set_kernel(torch.from_numpy(np.ascontiguousarray(k[x0:x0 + xs]).reshape(-1)).to(dev))   # collective
p.execute(); p.sync()
roll = np.roll(x, (2, 3, 4), (0, 1, 2))
e2 = float(np.abs(b.cpu().numpy().reshape(xs, n1, n2) - roll[x0:x0 + xs]).max() / np.abs(roll).max())
d = p.describe()
p.destroy()                                                      # collective
comm.destroy()
print(f"rank {rank} conv {e1:.3e} roll {e2:.3e} [{d}] done", flush=True)
assert e1 < 1e-11 and e2 < 1e-11, (e1, e2)
'''


def test_conv_two_processes_ipc_async(gpu, tmp_path):
    """P = 2 across real process boundaries: two ranks share cuda:0 on the stream-ordered IPC communicator."""
    import socket
    import time
    script = tmp_path / "conv_worker.py"
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
