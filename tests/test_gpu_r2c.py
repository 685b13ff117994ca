"""-m gpu: real-to-complex / complex-to-real slab plans (dfft_plan_create_r2c, api.PlanR2C) against numpy's rfftn / irfftn.

Single-GPU plans and P virtual devices on one GPU (LOCAL communicator, one thread per device), one multi-process case on the IPC
communicator; guard regions past r2c_counts, INPUT_FROM_IN leaving `in` alone, bit-identical repeated executes."""
import os
import subprocess
import sys
import threading
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
TOL = {"f64": 1e-11, "f32": 5e-4}
GUARD = 64  # sentinel elements past r2c_counts in every caller buffer
SENT = -12345.0


def _dtypes(prec):
    import torch
    return (torch.float64, torch.complex128) if prec == "f64" else (torch.float32, torch.complex64)


def _slab(n, P, g):
    blk = -(-n // P)
    return g * blk, (blk if g < P - 1 else n - (P - 1) * blk)


def _rel(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def _run(gpu, N, P, prec, inputs, direction, flags=0, scale=None, reps=1, check_guards=True):
    """P plans (virtual devices on one GPU when P > 1), executed `reps` times from P threads.  Returns per device the outputs of every
    execute (the first r2c_counts elements) and the input buffers afterwards."""
    import torch
    from distributedfft_amd import api
    n0, n1, n2 = N
    rdt, cdt = _dtypes(prec)
    comm = api.Comm.local(P) if P > 1 else None
    plans, bufs = [], []
    for g in range(P):
        rc, cc = api.r2c_counts(n0, n1, n2, P, g)
        ni, no = (rc, cc) if direction == api.FORWARD else (cc, rc)
        idt, odt = (rdt, cdt) if direction == api.FORWARD else (cdt, rdt)
        a = torch.full((ni + GUARD,), SENT, dtype=idt, device=gpu)
        b = torch.full((no + GUARD,), SENT, dtype=odt, device=gpu)
        src = torch.from_numpy(np.ascontiguousarray(inputs[g]).reshape(-1)).to(gpu).to(idt)
        a[:src.numel()] = src
        torch.cuda.synchronize()
        plans.append(api.PlanR2C(n0, n1, n2, a, b, comm, g, P, direction, flags))
        if scale is not None:
            plans[-1].set_scale(scale)
        bufs.append((a, b, ni, no, a.clone()))
    outs = [[] for _ in range(P)]
    errs = []

    def work(g):
        try:
            for _ in range(reps):
                if not flags & api.PLAN_INPUT_FROM_IN and _ > 0:
                    plans[g].load_input(bufs[g][4][:bufs[g][2]])
                plans[g].execute()
                plans[g].sync()
                outs[g].append(bufs[g][1][:bufs[g][3]].cpu().numpy().copy())
        except Exception as e:  # pragma: no cover
            errs.append(e)

    th = [threading.Thread(target=work, args=(g,)) for g in range(P)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    for g, (a, b, ni, no, a0) in enumerate(bufs):
        assert "pipeline=" + ("r2c" if direction == api.FORWARD else "c2r") in plans[g].describe()
        if check_guards:
            assert bool((b[no:] == SENT).all()), f"device {g}: the plan wrote past r2c_counts into out"
            assert bool((a[ni:] == SENT).all()), f"device {g}: the plan wrote past r2c_counts into in"
    ins = [b[0][:b[2]].cpu().numpy() for b in bufs]
    ins0 = [b[4][:b[2]].cpu().numpy() for b in bufs]
    for p in plans:
        p.destroy()
    if comm:
        comm.destroy()
    return outs, ins, ins0


def _real_input(N, prec, seed):
    x = np.random.default_rng(seed).standard_normal(N)
    return x.astype(np.float32) if prec == "f32" else x


def _split_real(x, P):
    return [x[s:s + n] for s, n in (_slab(x.shape[0], P, g) for g in range(P))]


def _split_bins(X, P):
    """[N0][N1][Nh] -> per device [ys][Nh][N0] (the R2C output layout)."""
    return [np.ascontiguousarray(X[:, s:s + n, :].transpose(1, 2, 0)) for s, n in (_slab(X.shape[1], P, g) for g in range(P))]


def _forward_case(gpu, N, P, prec, seed=1, flags=0):
    from distributedfft_amd import api
    x = _real_input(N, prec, seed)
    outs, _, _ = _run(gpu, N, P, prec, _split_real(x, P), api.FORWARD, flags)
    ref = _split_bins(np.fft.rfftn(x.astype(np.float64)), P)
    err = max(_rel(outs[g][0][:ref[g].size].reshape(ref[g].shape), ref[g]) for g in range(P))
    assert err < TOL[prec], (N, P, prec, err)
    return x, outs


FWD = [((25, 10, 16), 4), ((24, 10, 12), 4), ((48, 100, 12), 1), ((48, 100, 12), 3), ((14, 49, 16), 1), ((14, 49, 16), 2),
       ((8, 6, 40), 1), ((9, 8, 72), 2), ((4, 3, 7200), 1), ((5, 4, 4802), 2), ((4, 3, 8192), 1), ((64, 64, 64), 1), ((32, 48, 24), 2),
       ((16, 12, 10), 1), ((512, 8, 18), 1)]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N,P", FWD)
def test_r2c_forward_vs_rfftn(gpu, N, P, prec):
    _forward_case(gpu, N, P, prec)


@pytest.mark.parametrize("N,prec", [((256, 256, 256), "f64"), ((512, 512, 512), "f64"), ((512, 512, 512), "f32")])
def test_r2c_forward_full_size_cache_chunked(gpu, N, prec):
    """Slabs larger than the Infinity Cache: the Z and Y passes run chunk by chunk (describe() shows more than one chunk)."""
    import torch
    from distributedfft_amd import api
    x = _real_input(N, prec, 3)
    rdt, cdt = _dtypes(prec)
    rc, cc = api.r2c_counts(*N, 1, 0)
    a = torch.from_numpy(x.reshape(-1)).to(gpu)
    b = torch.empty(cc, dtype=cdt, device=gpu)
    p = api.PlanR2C(*N, a, b, None, 0, 1, api.FORWARD)
    if N[0] == 512:
        assert "chunks=1x" not in p.describe(), p.describe()
    p.execute()
    p.sync()
    got = b.cpu().numpy().reshape(N[1], N[2] // 2 + 1, N[0])  # (P = 1: r2c_counts is exactly the result)
    p.destroy()
    ref = np.fft.rfftn(x.astype(np.float64)).transpose(1, 2, 0)
    assert _rel(got, ref) < TOL[prec]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N,P", [((25, 10, 16), 4), ((48, 100, 12), 1), ((14, 49, 16), 2), ((8, 6, 40), 1), ((5, 4, 4802), 2),
                                 ((64, 64, 64), 1), ((256, 256, 256), 1)])
def test_c2r_round_trip(gpu, N, P, prec):
    """C2R of the forward output is N * x; with set_scale(1/N) it is x."""
    from distributedfft_amd import api
    x, outs = _forward_case(gpu, N, P, prec)
    bins = [outs[g][0] for g in range(P)]
    xs = _split_real(x.astype(np.float64), P)
    n = float(np.prod(N))
    back, _, _ = _run(gpu, N, P, prec, bins, api.BACKWARD)
    assert max(_rel(back[g][0].reshape(xs[g].shape), n * xs[g]) for g in range(P)) < TOL[prec]
    back, _, _ = _run(gpu, N, P, prec, bins, api.BACKWARD, scale=1.0 / n)
    assert max(_rel(back[g][0].reshape(xs[g].shape), xs[g]) for g in range(P)) < TOL[prec]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N,P", [((8, 6, 16), 1), ((25, 10, 16), 4), ((12, 10, 40), 2), ((6, 5, 4802), 1), ((64, 64, 64), 2)])
def test_c2r_non_hermitian_input_vs_irfftn(gpu, N, P, prec):
    """Arbitrary complex bins: inverse C2C along X and Y, then C2R along Z, the imaginary parts of kz = 0 and kz = N2/2 ignored --
    N * numpy.fft.irfftn.  Pins the Z-last order: any other order gives another result on such input."""
    from distributedfft_amd import api
    n0, n1, n2 = N
    rng = np.random.default_rng(7)
    X = rng.standard_normal((n0, n1, n2 // 2 + 1)) + 1j * rng.standard_normal((n0, n1, n2 // 2 + 1))
    if prec == "f32":
        X = X.astype(np.complex64)
    back, _, _ = _run(gpu, N, P, prec, _split_bins(X, P), api.BACKWARD)
    ref = _split_real(float(np.prod(N)) * np.fft.irfftn(X.astype(np.complex128), s=N, axes=(0, 1, 2)), P)
    assert max(_rel(back[g][0].reshape(ref[g].shape), ref[g]) for g in range(P)) < TOL[prec]


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("N,P,prec", [((25, 10, 16), 4, "f64"), ((48, 100, 12), 1, "f32"), ((8, 6, 40), 2, "f64"), ((64, 64, 64), 1, "f64")])
def test_r2c_input_from_in_guards_and_determinism(gpu, N, P, prec, direction):
    """INPUT_FROM_IN: `in` is never written, two executes give bit-identical results, nothing past r2c_counts is touched (_run)."""
    from distributedfft_amd import api
    x = _real_input(N, prec, 5)
    if direction == api.FORWARD:
        inputs = _split_real(x, P)
    else:
        inputs = _split_bins(np.fft.rfftn(x.astype(np.float64)).astype(np.complex64 if prec == "f32" else np.complex128), P)
    outs, ins, ins0 = _run(gpu, N, P, prec, inputs, direction, api.PLAN_INPUT_FROM_IN, reps=2)
    for g in range(P):
        assert np.array_equal(ins[g], ins0[g]), f"device {g}: INPUT_FROM_IN wrote into in"
        assert np.array_equal(outs[g][0], outs[g][1]), f"device {g}: two executes differ"
    # the default plan (input captured into bufferDev1, reloaded before the second execute): the same bits
    outs2, _, _ = _run(gpu, N, P, prec, inputs, direction, 0, reps=2)
    for g in range(P):
        assert np.array_equal(outs2[g][0], outs[g][0]) and np.array_equal(outs2[g][1], outs[g][0])


def test_r2c_plan_api_checks(gpu):
    import torch
    from distributedfft_amd import api, _lib as L
    a = torch.zeros(16 * 16 * 16, dtype=torch.float64, device=gpu)
    with pytest.raises(TypeError):
        api.PlanR2C(16, 16, 16, a, torch.zeros(16 * 16 * 9, dtype=torch.complex64, device=gpu), None, 0, 1, api.FORWARD)
    with pytest.raises(ValueError):
        api.PlanR2C(16, 16, 16, a, torch.zeros(10, dtype=torch.complex128, device=gpu), None, 0, 1, api.FORWARD)
    p = api.PlanR2C(16, 16, 16, a, torch.zeros(16 * 16 * 9, dtype=torch.complex128, device=gpu), None, 0, 1, api.FORWARD)
    p.tune()  # no hand-over buffer to place: a no-op
    p.execute()
    p.sync()
    assert len(p.stage_times()) == 4
    with pytest.raises(L.DfftError) as e:
        p.kernel_times()
    assert e.value.code == L.EUNSUPPORTED
    assert p.buffer1_tensor().dtype == torch.float64 and p.buffer1_tensor().numel() == 16 * 16 * 16
    p.destroy()


WORKER = r'''
import os, sys
import numpy as np, torch
sys.path.insert(0, os.environ["DFFT_ROOT"])
from distributedfft_amd import api
N = (24, 20, 40)
rank, P = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
n0, n1, n2 = N
nh = n2 // 2 + 1
dev = torch.device("cuda:0")
torch.cuda.set_device(0)
comm = api.Comm.ipc(P, rank, True)
x = np.random.default_rng(11).standard_normal(N)              # same array on every rank
X = np.fft.rfftn(x)
xb = -(-n0 // P); x0 = rank * xb; xs = min(xb, n0 - x0)
yb = -(-n1 // P); y0 = rank * yb; ys = min(yb, n1 - y0)
rc, cc = api.r2c_counts(n0, n1, n2, P, rank)
a = torch.from_numpy(np.ascontiguousarray(x[x0:x0 + xs]).reshape(-1)).to(dev)
b = torch.zeros(cc, dtype=torch.complex128, device=dev)
torch.cuda.synchronize()
p = api.PlanR2C(n0, n1, n2, a, b, comm, rank, P, api.FORWARD)      # collective
p.execute(); p.sync()
got = b[:ys * nh * n0].cpu().numpy().reshape(ys, nh, n0)
ref = X[:, y0:y0 + ys, :].transpose(1, 2, 0)
ef = float(np.abs(got - ref).max() / np.abs(X).max())
c = torch.zeros(rc, dtype=torch.float64, device=dev)
q = api.PlanR2C(n0, n1, n2, b.clone(), c, comm, rank, P, api.BACKWARD)
q.set_scale(1.0 / (n0 * n1 * n2))
q.execute(); q.sync()
eb = float(np.abs(c.cpu().numpy().reshape(xs, n1, n2) - x[x0:x0 + xs]).max())
p.destroy(); q.destroy()                                             # collective
comm.destroy()
print(f"rank {rank} forward {ef:.3e} roundtrip {eb:.3e}", flush=True)
assert ef < 1e-11 and eb < 1e-11, (ef, eb)
'''


def test_r2c_two_processes_ipc_async(gpu, tmp_path):
    """P = 2 across real process boundaries: two ranks share cuda:0 on the stream-ordered IPC communicator, forward against rfftn and the
    round trip through the C2R plan."""
    import socket
    import time
    script = tmp_path / "r2c_worker.py"
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
    assert all("roundtrip" in t for t in text)
