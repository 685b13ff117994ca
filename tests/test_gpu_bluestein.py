"""-m gpu tests of the any-length transforms (Bluestein's chirp-z algorithm, csrc/dfft_bluestein.hip): dfft_fft1d_any against numpy in
both forms (fused for n <= 2048, multi-pass above and under DFFT_BLUESTEIN_FUSED=0), bit-identity with the existing 1-D entry points on
7-smooth lengths, and 3D plans with DFFT_PLAN_ANY_LENGTH on one GPU and on virtual devices.

Error bound: max|err| / max|ref| < 1e-11 in fp64 (heFFTe's bar), < 1e-4 in fp32.

The per-length sweep -- every tuned length of this family, both precisions, every kernel variant -- lives in tests/test_gpu_tuned_sweep.py."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

from oracle import slab_oracle as so

pytestmark = pytest.mark.gpu

TOL = {"f64": 1e-11, "f32": 1e-4}
LENGTHS = [1, 11, 13, 17, 97, 101, 211, 509, 1009, 1021, 2039, 2049, 4099, 8191, 65537, 1000003]
MAX_ELEMS = 1 << 22  # per tensor, for the (batch, s) combinations of a length


def _tdt(prec):
    import torch
    return torch.complex128 if prec == "f64" else torch.complex64


def _rel_err(got, ref):
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-300))


def _rand(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)


def _ref(x, direction):
    n = x.shape[1]
    return np.fft.fft(x, axis=1) if direction > 0 else np.fft.ifft(x, axis=1) * n


def _configs(n):
    """(batch, s): batch 1 and a ragged batch, s in {1, 3, 64, 1000} where memory allows"""
    out = []
    for s in (1, 3, 64, 1000):
        for batch in (1, 5):
            if batch * n * s <= MAX_ELEMS:
                out.append((batch, s))
    return out


def _check_any(gpu, n, prec, direction, worst):
    import torch
    from distributedfft_amd import api
    for i, (batch, s) in enumerate(_configs(n)):
        x = _rand((batch, n, s), seed=n + 7 * i + s)
        xt = torch.from_numpy(x).to(gpu).to(_tdt(prec))
        ref = _ref(x.astype(np.complex128) if prec == "f64" else xt.cpu().numpy().astype(np.complex128), direction)
        got = api.fft1d_any(xt, dim=1, direction=direction).cpu().numpy()
        err = _rel_err(got, ref)
        worst[0] = max(worst[0], err)
        assert err < TOL[prec], (n, batch, s, err)
        if i == 0 or s == 3:  # in place
            y = xt.clone()
            api.fft1d_any(y, dim=1, direction=direction, out=y)
            err = _rel_err(y.cpu().numpy(), ref)
            assert err < TOL[prec], ("in place", n, batch, s, err)


@pytest.mark.parametrize("direction", [1, -1], ids=["fwd", "bwd"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n", LENGTHS)
def test_fft1d_any_vs_numpy(gpu, n, prec, direction):
    """Worst observed over every length, configuration and direction of this test on an MI355X: fp64 1.3e-15, fp32 3.1e-7
    (max|err| / max|ref|)."""
    worst = [0.0]
    _check_any(gpu, n, prec, direction, worst)


@pytest.mark.parametrize("direction", [1, -1], ids=["fwd", "bwd"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n", [n for n in LENGTHS if 1 < n <= 2048])
def test_fft1d_any_multi_pass_form_vs_numpy(gpu, n, prec, direction, monkeypatch):
    """DFFT_BLUESTEIN_FUSED=0: the multi-pass form on the fused form's M (single-pass kernels between the elementwise passes)."""
    monkeypatch.setenv("DFFT_BLUESTEIN_FUSED", "0")
    worst = [0.0]
    _check_any(gpu, n, prec, direction, worst)


@pytest.mark.parametrize("n", [11, 1009, 2039, 4099, 65537])
def test_round_trip(gpu, n):
    import torch
    from distributedfft_amd import api
    x = _rand((3, n), seed=n)
    xt = torch.from_numpy(x).to(gpu)
    back = api.fft1d_any(api.fft1d_any(xt, direction=api.FORWARD), direction=api.BACKWARD).cpu().numpy()
    assert np.abs(back / n - x).max() < 1e-12


def test_dim_argument_maps_to_batch_n_s(gpu):
    import torch
    from distributedfft_amd import api
    x = _rand((2, 13, 3, 5), seed=3)
    xt = torch.from_numpy(x).to(gpu)
    for dim in (0, 1, 2, -1):
        got = api.fft1d_any(xt, dim=dim).cpu().numpy()
        assert _rel_err(got, np.fft.fft(x, axis=dim)) < 1e-11, dim


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n", [64, 768, 1000, 8192])
def test_smooth_lengths_are_bit_identical_to_the_existing_entry_points(gpu, n, prec):
    import torch
    from distributedfft_amd import api
    x = torch.from_numpy(_rand((4, n), seed=n)).to(gpu).to(_tdt(prec))
    for d in (api.FORWARD, api.BACKWARD):
        assert torch.equal(api.fft1d_any(x, dim=1, direction=d), api.fft1d_rows(x, d))
    c = torch.from_numpy(_rand((2, n, 24), seed=n + 1)).to(gpu).to(_tdt(prec))
    for d in (api.FORWARD, api.BACKWARD):
        assert torch.equal(api.fft1d_any(c, dim=1, direction=d), api.fft1d_cols(c, d))


@pytest.mark.parametrize("n,s", [(1009, 1), (97, 64), (2039, 3), (4099, 1), (4099, 5)])
def test_deterministic(gpu, n, s):
    import torch
    from distributedfft_amd import api
    x = torch.from_numpy(_rand((3, n, s), seed=n)).to(gpu)
    a = api.fft1d_any(x, dim=1)
    b = api.fft1d_any(x, dim=1)
    assert torch.equal(a, b)


def test_heffte_dft_of_1_to_11(gpu):
    """test_units_stock.cpp:230-253 (heFFTe's stock back-end): DFT of [1..11] = 66, then -5.5 +- i*{18.73.., ...}."""
    import torch
    from distributedfft_amd import api
    imag = [18.731279813890875, 8.55816705136493, 4.765777128986846, 2.5117658384695547, 0.790780616972353]
    ref = np.empty(11, dtype=np.complex128)
    ref[0] = 66
    for i in range(1, 6):
        ref[i] = complex(-5.5, imag[i - 1])
        ref[11 - i] = complex(-5.5, -imag[i - 1])
    x = torch.arange(1, 12, dtype=torch.float64).to(torch.complex128).to(gpu)[None, :]
    got = api.fft1d_any(x).cpu().numpy()[0]
    assert np.abs(got - ref).max() < 1e-13


def test_trim_then_call_again(gpu):
    import torch
    from distributedfft_amd import _lib, api
    x = torch.from_numpy(_rand((2, 4099), seed=1)).to(gpu)
    a = api.fft1d_any(x)
    _lib.check(_lib.load().dfft_trim(), "dfft_trim")
    assert torch.equal(api.fft1d_any(x), a)


# ---- 3D plans with DFFT_PLAN_ANY_LENGTH ----------------------------------------------------------------------------------------------
def _run_plans(gpu, N, P, prec, inputs, direction, flags):
    """P plans (virtual devices on one GPU, LOCAL communicator) executed from P threads; returns the outputs and the describes."""
    import torch
    from distributedfft_amd import api
    n0, n1, n2 = N
    comm = api.Comm.local(P) if P > 1 else None
    plans, outs = [], []
    for g in range(P):
        mc = api.get_max_data_count(n0, n1, n2, P, g == P - 1)
        a = torch.zeros(mc, dtype=_tdt(prec), device=gpu)
        b = torch.zeros(mc, dtype=_tdt(prec), device=gpu)
        src = torch.from_numpy(np.ascontiguousarray(inputs[g]).reshape(-1)).to(gpu).to(_tdt(prec))
        a[:src.numel()] = src
        torch.cuda.synchronize()
        plans.append(api.Plan(n0, n1, n2, a, b, comm, g, P, direction, flags))
        outs.append(b)
    describes = [p.describe() for p in plans]
    errs = []

    def work(g):
        try:
            plans[g].execute()
            plans[g].sync()
        except Exception as e:  # pragma: no cover
            errs.append(e)

    th = [threading.Thread(target=work, args=(g,)) for g in range(P)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    res = [o.cpu().numpy() for o in outs]
    for p in plans:
        p.destroy()
    if comm:
        comm.destroy()
    return res, describes


SHAPES_3D = [(11, 13, 17), (13, 8, 8), (64, 97, 48), (97, 64, 101), (8, 8, 4099)]


@pytest.mark.parametrize("direction", [1, -1], ids=["fwd", "bwd"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("P", [1, 2, 4])
@pytest.mark.parametrize("N", SHAPES_3D)
def test_any_length_3d_plans_vs_fftn(gpu, N, P, prec, direction):
    from distributedfft_amd import api
    n0, n1, n2 = N
    x = so.random_input(N, seed=sum(N) + P)
    flags = api.PLAN_ANY_LENGTH | (api.PLAN_INPUT_FROM_IN if P != 2 else 0)
    if direction > 0:
        refs = so.fftn_reference(x, P)
        inputs = [x[so.slab_start(n0, P, g):so.slab_start(n0, P, g) + so.slab_size(n0, P, g)] for g in range(P)]
    else:  # input: x seen as a forward result in the [yy][z][kx] slabs; output: N * ifftn(x) in the X slabs
        inputs = [np.ascontiguousarray(x[:, so.slab_start(n1, P, d):so.slab_start(n1, P, d) + so.slab_size(n1, P, d), :].transpose(1, 2, 0))
                  for d in range(P)]
        full = np.fft.ifftn(x) * x.size
        refs = [full[so.slab_start(n0, P, g):so.slab_start(n0, P, g) + so.slab_size(n0, P, g)] for g in range(P)]
    outs, desc = _run_plans(gpu, N, P, prec, inputs, direction, flags)
    assert all("pipeline=unfused" in d and "bluestein_axis" in d for d in desc), desc
    scale = max(np.abs(r).max() for r in refs)
    for d in range(P):
        got = outs[d][:refs[d].size].reshape(refs[d].shape)
        assert np.abs(got - refs[d]).max() / scale < TOL[prec], (N, P, d)


@pytest.mark.parametrize("N,P", [((16, 12, 10), 1), ((64, 64, 64), 1), ((32, 48, 24), 2), ((8192, 16, 24), 1)])
def test_flag_on_smooth_shapes_is_bit_identical(gpu, N, P):
    from distributedfft_amd import api
    n0 = N[0]
    x = so.random_input(N, seed=5)
    inputs = [x[so.slab_start(n0, P, g):so.slab_start(n0, P, g) + so.slab_size(n0, P, g)] for g in range(P)]
    for direction in (1, -1):
        a, da = _run_plans(gpu, N, P, "f64", inputs, direction, 0)
        b, db = _run_plans(gpu, N, P, "f64", inputs, direction, api.PLAN_ANY_LENGTH)
        assert da == db
        for g in range(P):
            assert np.array_equal(a[g], b[g]), (N, P, g, direction)


def test_any_length_natural_is_unsupported(gpu):
    import torch
    from distributedfft_amd import api
    a = torch.zeros(11 * 8 * 8, dtype=torch.complex128, device=gpu)
    with pytest.raises(api.DfftError) as ei:
        api.Plan(11, 8, 8, a, torch.zeros_like(a), None, 0, 1, api.FORWARD, api.PLAN_ANY_LENGTH | api.PLAN_NATURAL)
    assert ei.value.code == api.L.EUNSUPPORTED


def test_plan_without_the_flag_still_refuses(gpu):
    import torch
    from distributedfft_amd import api
    a = torch.zeros(11 * 8 * 8, dtype=torch.complex128, device=gpu)
    with pytest.raises(api.DfftError):
        api.Plan(11, 8, 8, a, torch.zeros_like(a), None, 0, 1, api.FORWARD)
    with pytest.raises(api.DfftError):  # and 1-D: the existing entry points keep their refusals
        api.fft1d_rows(a.reshape(8, 88)[:, :11].contiguous())


def test_r2c_plan_rejects_the_flag(gpu):
    import torch
    from distributedfft_amd import _lib, api
    import ctypes as C
    a = torch.zeros(16 * 8 * 8, dtype=torch.float64, device=gpu)
    b = torch.zeros(16 * 8 * 5, dtype=torch.complex128, device=gpu)
    h = C.c_void_p()
    rc = _lib.load().dfft_plan_create_r2c(C.byref(h), 16, 8, 8, api.F64, api.FORWARD, a.data_ptr(), b.data_ptr(), None, 0, 1,
                                          api.PLAN_ANY_LENGTH)
    assert rc == _lib.EUNSUPPORTED


def test_distfftopt_any_length(gpu, tmp_path):
    """distFFTOpt 11 13 17 1 with DFFT_ANY_LENGTH=1: the drop-in driver's stage line and round-trip error."""
    from distributedfft_amd import _lib
    env = dict(os.environ, DFFT_ANY_LENGTH="1")
    r = subprocess.run([str(_lib.DRIVER_PATH), "11", "13", "17", "1"], capture_output=True, text=True, timeout=300, env=env,
                       cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "t0:" in r.stdout
    assert float(re.search(r"Max error:\s*([0-9.eE+-]+)", r.stdout).group(1)) < 1e-11


# ---- the multi-pass form's batch chunks (tests/large_extent.py: tiled inputs, every line checked) ------------------------------------------
# (n, s, prec, DFFT_BLUESTEIN_FUSED): two whole scratch chunks and a ragged third, by the mirrored chunk rule
CHUNK_EDGE = [(4099, 5, "f64", None), (4099, 1, "f32", None), (1009, 3, "f64", "0")]


@pytest.mark.parametrize("inplace", [True, False], ids=["in-place", "out-of-place"])
@pytest.mark.parametrize("n,s,prec,fused_env", CHUNK_EDGE)
def test_multi_pass_chunk_edges(gpu, n, s, prec, fused_env, inplace, monkeypatch):
    """The chunk loop of bluestein_fft with more than one chunk: the b0 offsets of in, out and the ragged last chunk."""
    import large_extent as LE
    from distributedfft_amd import _lib, api
    if fused_env is not None:
        monkeypatch.setenv("DFFT_BLUESTEIN_FUSED", fused_env)
    lib, code = _lib.load(), {"f64": api.F64, "f32": api.F32}[prec]
    assert lib.dfft_bluestein_fused_applies(n, s) == 0
    M = lib.dfft_bluestein_length(n)
    cu = LE.bluestein_chunk(M, s, 1 << 40, prec)
    batch = LE.ragged_batch(cu)
    scratch = int(lib.dfft_fft1d_any_scratch_bytes(n, s, batch, code))
    assert cu > 1 and scratch == cu * LE.bluestein_per_transform_bytes(M, s, prec)   # the library chunks at the mirrored size
    K = LE.pick_k([(batch, n, s, LE.CBYTES[prec])])
    x, ref = LE.complex_base(n, K, +1)
    LE.run_case(gpu, f"any n={n} s={s} batch={batch} ({cu} per chunk) {'in place' if inplace else 'out of place'}", "bluestein", prec, n, x, ref,
                batch, s, lambda t, o: api.fft1d_any(t, 1, api.FORWARD, out=o), inplace, scratch=scratch)
