"""-m gpu: multi-output real-field spectral-filter plans (dfft_plan_create_conv_real_multi, api.PlanConvRealMulti) against numpy in float64:
y_k = irfftn(rfftn(x) * H * a_k[:, None, None] * b_k[None, :, None] * c_k[None, None, :], s=N, axes=(0, 1, 2)).

Error measure and bounds are the project's own (tests/test_gpu_conv_real.py): max|got - ref| / max|ref| below 1e-11 (fp64) / 5e-4 (fp32).
Inputs are unit-variance normals, the base filter is that file's _filter (|H| <= 1) and the factors are unit-modulus random phases
exp(i theta), seeded per output, so |H_k| = |H| and max|ref| stays O(1) (2.1 - 2.7 for the plain filter on these shapes).  The Poisson
case uses the factors i k on a band-limited input with an analytic answer.  Single-GPU plans, P virtual devices on one GPU (LOCAL
communicator, one thread per device) and one two-process case on the stream-ordered IPC communicator."""
import importlib.util
import os
import subprocess
import sys
import threading
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

_spec = importlib.util.spec_from_file_location("_conv_real_tests", Path(__file__).with_name("test_gpu_conv_real.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)
TOL, GUARD, SENT = R.TOL, R.GUARD, R.SENT
_env, _rdt, _slab, _rel, _width, _input, _filter, _split_x, _split_bins = (R._env, R._rdt, R._slab, R._rel, R._width, R._input, R._filter,
                                                                            R._split_x, R._split_bins)

FUSED_SHAPES = [(128, 16, 32), (256, 8, 32), (384, 8, 16), (512, 8, 32), (768, 4, 16), (1024, 6, 32), (64, 64, 64)]
WIDTH_SHAPES = [(128, 8, 8), (128, 8, 4), (128, 8, 30), (64, 12, 10)]
MULTI_SHAPES = [(2048, 4, 16), (1000, 8, 16), (343, 8, 8), (20, 36, 40)]
MULTI_GPU = [((64, 64, 64), 2), ((25, 10, 16), 4), ((24, 10, 12), 3), ((1024, 8, 64), 4)]


def _cdt(prec):
    import torch
    return torch.complex128 if prec == "f64" else torch.complex64


def _phases(N, k, prec):
    """Unit-modulus factors of output k along kx, ky, kz (lengths N0, N1, N2/2 + 1), seeded per output."""
    r = np.random.default_rng(100 + k)
    f = [np.exp(1j * r.uniform(0, 2 * np.pi, n)) for n in (N[0], N[1], N[2] // 2 + 1)]
    return [v.astype(np.complex64) if prec == "f32" else v for v in f]


def _ref(x, H, fac):
    a, b, c = [np.ones(n) if v is None else v.astype(np.complex128) for v, n in zip(fac, (x.shape[0], x.shape[1], x.shape[2] // 2 + 1))]
    Hd = H.astype(np.complex128 if np.iscomplexobj(H) else np.float64)
    S = np.fft.rfftn(x.astype(np.float64), axes=(0, 1, 2)) * Hd * a[:, None, None] * b[None, :, None] * c[None, None, :]
    return np.fft.irfftn(S, s=x.shape, axes=(0, 1, 2))


def _run(gpu, N, P, prec, x, K, factors, H=None, kernel=None, env=None, alias0=False, reps=1):
    """P multi-output plans (virtual devices on one GPU when P > 1) executed `reps` times from P threads.  factors: K triples (ax, ay,
    az) of numpy vectors or None.  Returns outs[rep][k] ([N0][N1][N2] each, gathered) and the describe() strings; checks the guard
    elements behind `in` and every out and, unless output 0 aliases it, that `in` is left alone."""
    import torch
    from distributedfft_amd import api
    n0, n1, n2 = N
    rdt, cdt = _rdt(prec), _cdt(prec)
    xs_, hs_ = _split_x(x, P), (_split_bins(H, P) if H is not None else None)
    ks_ = _split_x(kernel, P) if kernel is not None else None
    with _env(**(env or {})):
        comm = api.Comm.local(P) if P > 1 else None
        plans, bufs = [], []
        for g in range(P):
            cnt = api.get_data_count(N, P, g)
            a = torch.full((cnt + GUARD,), SENT, dtype=rdt, device=gpu)
            a[:cnt] = torch.from_numpy(xs_[g].reshape(-1)).to(gpu).to(rdt)
            outs = [a if (alias0 and k == 0) else torch.full((cnt + GUARD,), SENT, dtype=rdt, device=gpu) for k in range(K)]
            torch.cuda.synchronize()
            plans.append(api.PlanConvRealMulti(n0, n1, n2, a, outs, comm, g, P))
            bufs.append((a, outs, cnt, a.clone()))
    res = [[[None] * P for _ in range(K)] for _ in range(reps)]
    errs = []

    def work(g):
        try:
            a, outs, cnt, a0 = bufs[g]
            if hs_ is not None:
                h = torch.from_numpy(hs_[g].reshape(-1)).to(gpu)
                plans[g].set_filter(h)
                h.fill_(7.0)  # the plan keeps a private copy
            else:
                plans[g].set_kernel(torch.from_numpy(ks_[g].reshape(-1)).to(gpu).to(rdt))
            for k, fac in enumerate(factors):
                if fac is None or all(v is None for v in fac):
                    continue
                t = [None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(gpu).to(cdt) for v in fac]
                plans[g].set_factors(k, *t)
                for v in t:
                    if v is not None:
                        v.fill_(7.0)  # private copies here too
            for r in range(reps):
                if alias0 and r > 0:
                    a[:cnt] = a0[:cnt]
                    torch.cuda.synchronize()
                plans[g].execute()
                plans[g].sync()
                for k in range(K):
                    res[r][k][g] = outs[k][:cnt].cpu().numpy().reshape(-1, n1, n2).copy()
        except Exception as e:  # pragma: no cover
            errs.append(e)

    th = [threading.Thread(target=work, args=(g,)) for g in range(P)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    desc = [p.describe() for p in plans]
    for g, (a, outs, cnt, a0) in enumerate(bufs):
        for k, o in enumerate(outs):
            assert bool((o[cnt:] == SENT).all()), f"device {g}: the plan wrote past dfft_local_count into out {k}"
        assert bool((a[cnt:] == SENT).all()), f"device {g}: the plan wrote past dfft_local_count into in"
        if not alias0:
            assert torch.equal(a, a0), f"device {g}: the execute changed `in`"
    for p in plans:
        p.destroy()
    if comm:
        comm.destroy()
    return [[np.concatenate(o, axis=0) for o in rr] for rr in res], desc


def _check(gpu, N, P, prec, kind, K, env=None, expect=None):
    x, H = _input(N, prec), _filter(N, kind, prec)
    factors = [_phases(N, k, prec) for k in range(K)]
    outs, desc = _run(gpu, N, P, prec, x, K, factors, H, env=env)
    for d in desc:
        assert "pipeline=conv-real-multi " in d and f"outputs={K} " in d and f"filter={kind}" in d, d
        assert f"width={_width(N[2] // 2 + 1, prec)} " in d, d
        if expect:
            assert f"xconv={expect}" in d, (expect, d)
    for k in range(K):
        err = _rel(outs[0][k], _ref(x, H, factors[k]))
        print(f"conv-real-multi {N} P={P} {prec} {kind} K={K} {env or ''} output {k}: err {err:.3e}  [{desc[0]}]")
        assert err < TOL[prec], (N, P, prec, kind, K, k, err)
    return outs[0]


# 1
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("kind", ["complex", "real"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N", FUSED_SHAPES)
def test_multi_every_fused_length_and_its_multi_route_twin(gpu, N, prec, kind, K):
    _check(gpu, N, 1, prec, kind, K, expect="fused")
    _check(gpu, N, 1, prec, kind, K, env={"DFFT_CONV_FUSED": "0"}, expect="multi")


# 2
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N", [(64, 64, 64), (1024, 6, 32)])
def test_multi_eight_outputs(gpu, N, prec):
    """The register-pressure and many-pointer cases."""
    _check(gpu, N, 1, prec, "complex", 8, expect="fused")


# 3
@pytest.mark.parametrize("kind", ["complex", "real"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N", WIDTH_SHAPES)
def test_multi_widths_and_ragged_tiles(gpu, N, prec, kind):
    """Nh = 5, 3, 16, 6: less than a tile, ragged last tiles; _run checks the guards behind `in` and every out and that `in` is unchanged."""
    _check(gpu, N, 1, prec, kind, 2, expect="fused")


# 4
@pytest.mark.parametrize("kind", ["complex", "real"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N", MULTI_SHAPES)
def test_multi_route_lengths(gpu, N, prec, kind):
    _check(gpu, N, 1, prec, kind, 3, expect="multi")


# 5
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N", [(128, 16, 32), (20, 36, 40)])
def test_multi_defaults_are_ones_and_set_factors_leaves_the_other_outputs_alone(gpu, N, prec):
    import torch
    from distributedfft_amd import api
    x, H = _input(N, prec), _filter(N, "complex", prec)
    single, _ = R._run(gpu, N, 1, prec, x, H)
    cnt = int(np.prod(N))
    a = torch.from_numpy(x.reshape(-1)).to(gpu).to(_rdt(prec))
    outs = [torch.zeros(cnt, dtype=_rdt(prec), device=gpu) for _ in range(3)]
    torch.cuda.synchronize()
    p = api.PlanConvRealMulti(*N, a, outs, None, 0, 1)
    p.set_filter(torch.from_numpy(_split_bins(H, 1)[0].reshape(-1)).to(gpu))

    def run():
        p.execute()
        p.sync()
        return [o.cpu().numpy().reshape(N).copy() for o in outs]

    y = run()
    for k in range(3):
        d = _rel(y[k], single[0])
        print(f"defaults {N} {prec} output {k} vs PlanConvReal: {d:.3e}")
        assert d < TOL[prec] and _rel(y[k], _ref(x, H, (None, None, None))) < TOL[prec], (N, prec, k, d)
    b = _phases(N, 1, prec)[1]
    p.set_factors(1, ay=torch.from_numpy(b).to(gpu).to(_cdt(prec)))
    z = run()
    assert np.array_equal(z[0], y[0]) and np.array_equal(z[2], y[2]), "set_factors(1) disturbed another output"
    e = _rel(z[1], _ref(x, H, (None, b, None)))
    print(f"ay alone {N} {prec}: {e:.3e}")
    assert e < TOL[prec], (N, prec, e)
    p.set_factors(1)  # back to ones
    w = run()
    assert np.array_equal(w[1], y[1])
    p.destroy()


# 6
@pytest.mark.parametrize("kind", ["complex", "real"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N,P", MULTI_GPU)
def test_multi_virtual_devices(gpu, N, P, prec, kind):
    """Uneven splits of both axes; the random phases along ky are not constant, so a wrong y0 shows."""
    _check(gpu, N, P, prec, kind, 3, expect="fused" if N[0] in (64, 1024) else "multi")


# 7
@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_multi_poisson_with_forces(gpu, prec, P):
    """H = -1/|k|^2 (0 at k = 0), output 0 with ones, outputs 1 - 3 with i k along one axis each (Nyquist bin zeroed), on
    f = laplace(u), u = sin(x) sin(2 y) sin(z): the potential u and its analytic gradient."""
    N = (64, 64, 64)
    m = [np.fft.fftfreq(N[0], 1.0 / N[0]), np.fft.fftfreq(N[1], 1.0 / N[1]), np.fft.rfftfreq(N[2], 1.0 / N[2])]  # integer wavenumbers
    k2 = m[0][:, None, None] ** 2 + m[1][None, :, None] ** 2 + m[2][None, None, :] ** 2
    H = np.zeros(k2.shape)
    H[k2 > 0] = -1.0 / k2[k2 > 0]
    ik = []
    for ax in range(3):
        v = 1j * m[ax]
        v[N[ax] // 2] = 0
        ik.append(v)
    r = [2 * np.pi * np.arange(n) / n for n in N]
    sx, sy, sz = np.sin(r[0])[:, None, None], np.sin(2 * r[1])[None, :, None], np.sin(r[2])[None, None, :]
    cx, cy, cz = np.cos(r[0])[:, None, None], 2 * np.cos(2 * r[1])[None, :, None], np.cos(r[2])[None, None, :]
    u = sx * sy * sz
    f = -6.0 * u
    want = [u, cx * sy * sz, sx * cy * sz, sx * sy * cz]
    if prec == "f32":
        H, f = H.astype(np.float32), f.astype(np.float32)
    factors = [None, (ik[0], None, None), (None, ik[1], None), (None, None, ik[2])]
    outs, desc = _run(gpu, N, P, prec, f, 4, factors, H)
    assert "filter=real" in desc[0] and "outputs=4 " in desc[0], desc[0]
    for k in range(4):
        err = _rel(outs[0][k], want[k] * np.ones(N))
        print(f"poisson with forces P={P} {prec} output {k}: err {err:.3e}")
        assert err < TOL[prec], (P, prec, k, err)


# 8
@pytest.mark.parametrize("N,P,env", [((128, 16, 32), 1, None), ((128, 16, 32), 1, {"DFFT_CHUNK_PLANES": "3"}), ((20, 36, 40), 1, None),
                                     ((64, 64, 64), 2, None)])
def test_multi_aliasing_and_repeats_are_bit_identical(gpu, N, P, env):
    K = 3
    x, H = _input(N, "f64"), _filter(N, "complex", "f64")
    factors = [_phases(N, k, "f64") for k in range(K)]
    oop, d0 = _run(gpu, N, P, "f64", x, K, factors, H, reps=3)
    for k in range(K):
        assert _rel(oop[0][k], _ref(x, H, factors[k])) < TOL["f64"]
        for r in (1, 2):
            assert np.array_equal(oop[0][k], oop[r][k]), f"execute {r} differs from execute 0 in output {k}"
    inp, d1 = _run(gpu, N, P, "f64", x, K, factors, H, alias0=True, reps=2, env=env)
    if env:  # the chunk loop forced as in test_conv_real_chunked_is_bit_identical
        assert "chunk_planes=0" in d0[0] and "chunk_planes=3" in d1[0], (d0[0], d1[0])
    for k in range(K):
        assert np.array_equal(oop[0][k], inp[0][k]) and np.array_equal(oop[0][k], inp[1][k]), f"outs[0] is in: output {k} differs"


# 9
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N,P", [((128, 96, 64), 1), ((25, 10, 16), 4)])
def test_multi_set_kernel_agrees_with_set_filter(gpu, N, P, prec):
    x = _input(N, prec, 6)
    k = (np.random.default_rng(7).standard_normal(N) / np.sqrt(float(np.prod(N)))).astype(x.dtype)  # |rfftn(k)| = O(1)
    H = np.fft.rfftn(k.astype(np.float64), axes=(0, 1, 2))
    Hc = H.astype(np.complex64) if prec == "f32" else H
    factors = [_phases(N, q, prec) for q in range(2)]
    a, _ = _run(gpu, N, P, prec, x, 2, factors, kernel=k)
    b, _ = _run(gpu, N, P, prec, x, 2, factors, Hc)
    for q in range(2):
        ref = _ref(x, H, factors[q])
        ea, eb, d = _rel(a[0][q], ref), _rel(b[0][q], ref), _rel(a[0][q], b[0][q])
        print(f"set_kernel {ea:.3e} set_filter(rfftn(k)) {eb:.3e} difference {d:.3e}")
        assert ea < TOL[prec] and eb < TOL[prec] and d < TOL[prec], (N, P, prec, q, ea, eb, d)


# 10
def test_multi_plan_created_and_destroyed_without_an_execute(gpu):
    """The forward half, one C2R half per output and the factor tables go away cleanly when nothing has run; the buffers are untouched."""
    import torch
    from distributedfft_amd import api
    N = (16, 6, 8)
    cnt = int(np.prod(N))
    x = _input(N, "f64")
    a = torch.from_numpy(x.reshape(-1)).to(gpu)
    outs = [torch.zeros(cnt, dtype=torch.float64, device=gpu) for _ in range(3)]
    torch.cuda.synchronize()
    p = api.PlanConvRealMulti(*N, a, outs, None, 0, 1)
    assert "pipeline=conv-real-multi outputs=3 " in p.describe() and "filter=unset" in p.describe()
    p.destroy()  # raises on any return code but DFFT_OK
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), x.reshape(-1)) and not any(bool(o.any()) for o in outs)


def test_multi_contract_on_a_live_device(gpu):
    import torch
    from distributedfft_amd import _lib as L
    from distributedfft_amd import api
    N = (128, 16, 32)
    cnt = int(np.prod(N))
    x, H = _input(N, "f64"), _filter(N, "real", "f64")
    a = torch.from_numpy(x.reshape(-1)).to(gpu)
    outs = [torch.zeros(cnt, dtype=torch.float64, device=gpu) for _ in range(2)]
    torch.cuda.synchronize()
    p = api.PlanConvRealMulti(*N, a, outs, None, 0, 1)
    assert "pipeline=conv-real-multi outputs=2 " in p.describe() and "filter=unset" in p.describe()
    with pytest.raises(L.DfftError) as e:
        p.execute()
    assert e.value.code == L.EINVAL and "filter" in str(e.value)
    good = [torch.ones(n, dtype=torch.complex128, device=gpu) for n in (N[0], N[1], N[2] // 2 + 1)]
    with pytest.raises(ValueError):
        p.set_factors(2, *good)
    with pytest.raises(ValueError):
        p.set_factors(-1, *good)
    lib = L.load()
    assert lib.dfft_conv_set_factors(p.handle, 2, None, None, None) == L.EINVAL
    assert lib.dfft_conv_set_factors(p.handle, -1, None, None, None) == L.EINVAL
    with pytest.raises(ValueError, match="elements expected"):
        p.set_factors(0, ax=torch.ones(N[0] + 1, dtype=torch.complex128, device=gpu))
    with pytest.raises(ValueError, match="elements expected"):
        p.set_factors(0, az=torch.ones(N[2], dtype=torch.complex128, device=gpu))
    with pytest.raises(TypeError, match="precision"):
        p.set_factors(0, ay=torch.ones(N[1], dtype=torch.complex64, device=gpu))
    with pytest.raises(TypeError, match="precision"):
        p.set_factors(0, ay=torch.ones(N[1], dtype=torch.float64, device=gpu))
    with pytest.raises(ValueError, match="device"):
        p.set_factors(0, ay=torch.ones(N[1], dtype=torch.complex128))
    # a plain PlanConvReal handle is not a multi plan
    b = torch.zeros(cnt, dtype=torch.float64, device=gpu)
    q = api.PlanConvReal(*N, a, b, None, 0, 1)
    assert lib.dfft_conv_set_factors(q.handle, 0, None, None, None) == L.EINVAL
    q.destroy()

    def run():
        p.execute()
        p.sync()
        return [o.cpu().numpy().reshape(N).copy() for o in outs]

    fac = _phases(N, 1, "f64")
    p.set_factors(1, *[torch.from_numpy(v).to(gpu) for v in fac])
    h = torch.from_numpy(_split_bins(H, 1)[0].reshape(-1)).to(gpu)
    p.set_filter(h)
    assert "filter=real" in p.describe()
    y = run()
    assert _rel(y[0], _ref(x, H, (None, None, None))) < TOL["f64"] and _rel(y[1], _ref(x, H, fac)) < TOL["f64"]
    t = p.stage_times()
    assert len(t) == 4 and all(v >= 0 for v in t), t
    # set_scale takes effect at the next set_filter
    p.set_scale(2.0)
    y2 = run()
    assert np.array_equal(y2[0], y[0]) and np.array_equal(y2[1], y[1])
    p.set_filter(h)
    y3 = run()
    assert np.array_equal(y3[0], 2.0 * y[0]) and np.array_equal(y3[1], 2.0 * y[1])
    p.destroy()
    p.destroy()  # twice


WORKER = r'''
import os, sys
import numpy as np, torch
sys.path.insert(0, os.environ["DFFT_ROOT"])
from distributedfft_amd import api
N = (64, 20, 40)
K = 2
rank, P = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
n0, n1, n2 = N
nh = n2 // 2 + 1
dev = torch.device("cuda:0")
torch.cuda.set_device(0)
comm = api.Comm.ipc(P, rank, True)
r = np.random.default_rng(11)                                   # same arrays on every rank
x = r.standard_normal(N)
H = (r.uniform(-1, 1, (n0, n1, nh)) + 1j * r.uniform(-1, 1, (n0, n1, nh))) / np.sqrt(2.0)
fac = [[np.exp(1j * r.uniform(0, 2 * np.pi, n)) for n in (n0, n1, nh)] for k in range(K)]
S = np.fft.rfftn(x, axes=(0, 1, 2)) * H
refs = [np.fft.irfftn(S * f[0][:, None, None] * f[1][None, :, None] * f[2][None, None, :], s=N, axes=(0, 1, 2)) for f in fac]
xb = -(-n0 // P); x0 = rank * xb; xs = min(xb, n0 - x0)
yb = -(-n1 // P); y0 = rank * yb; ys = min(yb, n1 - y0)
a = torch.from_numpy(np.ascontiguousarray(x[x0:x0 + xs]).reshape(-1)).to(dev)
outs = [torch.zeros_like(a) for k in range(K)]
torch.cuda.synchronize()
p = api.PlanConvRealMulti(n0, n1, n2, a, outs, comm, rank, P)   # collective
p.set_filter(torch.from_numpy(np.ascontiguousarray(H[:, y0:y0 + ys, :].transpose(1, 2, 0)).reshape(-1)).to(dev))
for k in range(K):
    p.set_factors(k, *[torch.from_numpy(v).to(dev) for v in fac[k]])
errs = []
for rep in range(2):
    p.execute(); p.sync()
    errs += [float(np.abs(outs[k].cpu().numpy().reshape(xs, n1, n2) - refs[k][x0:x0 + xs]).max() / np.abs(refs[k]).max()) for k in range(K)]
d = p.describe()
p.destroy()                                                      # collective
comm.destroy()
print(f"rank {rank} conv-real-multi {errs} [{d}] done", flush=True)
assert max(errs) < 1e-11, errs
'''


# 11
def test_multi_two_processes_ipc_async(gpu, tmp_path):
    """P = 2 across real process boundaries: two ranks share cuda:0 on the stream-ordered IPC communicator (the WORKER pattern of
    tests/test_gpu_conv_real.py: one time limit, every exit status checked)."""
    import socket
    import time
    script = tmp_path / "conv_multi_worker.py"
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
