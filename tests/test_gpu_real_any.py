"""-m gpu: any-length real transforms -- dfft_rfft1d (api.rfft1d / api.irfft1d) against numpy's rfft / irfft for every real form, and
dfft_plan_create_r2c_any (api.PlanR2C(any_length=True)) against rfftn / irfftn on one GPU and on P virtual devices; guard regions,
INPUT_FROM_IN, determinism, the cross-talk bound of the two-for-one pairs, and bit-identity with dfft_plan_create_r2c for form-1 axes.

The per-length sweep -- every tuned length of this family, both precisions, every kernel variant -- lives in tests/test_gpu_tuned_sweep.py."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = {"f64": 1e-11, "f32": 5e-4}
GUARD = 64
SENT = -12345.0

FORM1 = [16, 30, 8192]
FORM2_TUNED = [3, 9, 125, 243, 2187, 3125]
FORM2_GENERIC = [15, 45, 375, 3375]
FORM3_FOUR_STEP = [15625, 16384]
FORM3_BLUESTEIN = [1, 11, 97, 1009, 2039, 4099, 8198]


def _rel(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def _np_real(prec):
    return np.float64 if prec == "f64" else np.float32


def _np_cplx(prec):
    return np.complex128 if prec == "f64" else np.complex64


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n", FORM1 + FORM2_TUNED + FORM2_GENERIC + FORM3_FOUR_STEP + FORM3_BLUESTEIN)
def test_rfft1d_vs_numpy(gpu, n, prec):
    import torch
    from distributedfft_amd import api
    expect = 1 if n in FORM1 else (2 if n in FORM2_TUNED + FORM2_GENERIC else 3)
    assert api.real_form(n) == expect
    rng = np.random.default_rng(n)
    for batch in (1, 2, 5, 64):
        x = rng.standard_normal((batch, n)).astype(_np_real(prec))
        got = api.rfft1d(torch.from_numpy(x).to(gpu)).cpu().numpy()
        assert got.shape == (batch, n // 2 + 1)
        err = _rel(got, np.fft.rfft(x.astype(np.float64), axis=1))
        assert err < TOL[prec], (n, batch, prec, err)


def _guarded(shape, dtype, gpu):
    import torch
    count = int(np.prod(shape))
    buf = torch.full((count + GUARD,), SENT, dtype=dtype, device=gpu)
    return buf, buf[:count].view(shape)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n", [16, 30, 8192, 3, 125, 2187, 15, 375, 15625, 16384, 1, 97, 4099, 8198])
def test_irfft1d_non_hermitian_vs_numpy(gpu, n, prec):
    """Arbitrary bins (imaginary DC / Nyquist parts not zero): n * numpy.fft.irfft.  The input is left alone, nothing past `out` is written,
    and irfft1d(rfft1d(x)) / n is x."""
    import torch
    from distributedfft_amd import api
    rdt, cdt = (torch.float64, torch.complex128) if prec == "f64" else (torch.float32, torch.complex64)
    rng = np.random.default_rng(n + 1)
    for batch in (1, 2, 5, 64):
        nh = n // 2 + 1
        X = (rng.standard_normal((batch, nh)) + 1j * rng.standard_normal((batch, nh))).astype(_np_cplx(prec))
        Xd = torch.from_numpy(X).to(gpu)
        obuf, out = _guarded((batch, n), rdt, gpu)
        api.irfft1d(Xd, n, out=out)
        ref = n * np.fft.irfft(X.astype(np.complex128), n, axis=1)
        err = _rel(out.cpu().numpy(), ref)
        assert err < TOL[prec], (n, batch, prec, err)
        assert np.array_equal(Xd.cpu().numpy(), X), "irfft1d wrote into its input"
        assert bool((obuf[batch * n:] == SENT).all()), "irfft1d wrote past out"
        x = rng.standard_normal((batch, n)).astype(_np_real(prec))
        xd = torch.from_numpy(x).to(gpu)
        cbuf, bins = _guarded((batch, nh), cdt, gpu)
        api.rfft1d(xd, out=bins)
        assert bool((cbuf[batch * nh:] == SENT).all()), "rfft1d wrote past out"
        assert np.array_equal(xd.cpu().numpy(), x), "rfft1d wrote into its input"
        back = api.irfft1d(bins, n).cpu().numpy() / n
        assert float(np.abs(back - x).max() / max(np.abs(x).max(), 1e-300)) < TOL[prec], (n, batch, prec)


@pytest.mark.parametrize("n", [8192, 3125, 375, 15625, 1009])
def test_rfft1d_batch_above_256_mib(gpu, n):
    """At least 256 MiB of fp64 reals per call: the launch grids, and for the paired multi-pass forms several scratch chunks."""
    import torch
    from distributedfft_amd import api
    batch = -(-(256 << 20) // (8 * n))
    batch += batch % 2 == 0  # an odd row count: the last pair has a zero partner
    x = np.random.default_rng(n).standard_normal((batch, n))
    xd = torch.from_numpy(x).to(gpu)
    X = api.rfft1d(xd)
    ref = np.fft.rfft(x, axis=1)
    assert _rel(X.cpu().numpy(), ref) < TOL["f64"]
    del ref
    back = api.irfft1d(X, n)
    assert float(np.abs(back.cpu().numpy() / n - x).max() / np.abs(x).max()) < TOL["f64"]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n", [125, 375, 97, 16, 15625])
def test_pair_cross_talk_bound(gpu, n, prec):
    """The two rows of a pair share one transform: a row next to a partner 1e3 times larger keeps an error within tolerance relative to the
    pair's maximum (not to its own magnitude)."""
    import torch
    from distributedfft_amd import api
    rng = np.random.default_rng(3)
    x = rng.standard_normal((8, n))
    x[0::2] *= 1e3
    x = x.astype(_np_real(prec))
    ref = np.fft.rfft(x.astype(np.float64), axis=1)
    got = api.rfft1d(torch.from_numpy(x).to(gpu)).cpu().numpy()
    for p in range(4):
        scale = np.abs(ref[2 * p:2 * p + 2]).max()
        for r in (2 * p, 2 * p + 1):
            assert float(np.abs(got[r] - ref[r]).max() / scale) < TOL[prec], (n, prec, r)
    X = (rng.standard_normal((8, n // 2 + 1)) + 1j * rng.standard_normal((8, n // 2 + 1)))
    X[1::2] *= 1e3
    X = X.astype(_np_cplx(prec))
    ref = n * np.fft.irfft(X.astype(np.complex128), n, axis=1)
    got = api.irfft1d(torch.from_numpy(X).to(gpu), n).cpu().numpy()
    for p in range(4):
        scale = np.abs(ref[2 * p:2 * p + 2]).max()
        for r in (2 * p, 2 * p + 1):
            assert float(np.abs(got[r] - ref[r]).max() / scale) < TOL[prec], (n, prec, r)


# ---- 3D plans ----------------------------------------------------------------------------------------------------------------------
def _dtypes(prec):
    import torch
    return (torch.float64, torch.complex128) if prec == "f64" else (torch.float32, torch.complex64)


def _slab(n, P, g):
    blk = -(-n // P)
    return g * blk, (blk if g < P - 1 else n - (P - 1) * blk)


def _split_real(x, P):
    return [x[s:s + n] for s, n in (_slab(x.shape[0], P, g) for g in range(P))]


def _split_bins(X, P):
    return [np.ascontiguousarray(X[:, s:s + n, :].transpose(1, 2, 0)) for s, n in (_slab(X.shape[1], P, g) for g in range(P))]


def _run(gpu, N, P, prec, inputs, direction, flags=0, reps=1, any_length=True):
    """P plans (virtual devices on one GPU when P > 1), executed `reps` times from P threads; checks the guards past r2c_counts.  Returns
    per device the outputs of every execute, the input buffers afterwards and before, and the plans' describe() lines."""
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
        plans.append(api.PlanR2C(n0, n1, n2, a, b, comm, g, P, direction, flags, any_length=any_length))
        bufs.append((a, b, ni, no, a.clone()))
    outs = [[] for _ in range(P)]
    errs = []

    def work(g):
        try:
            for r in range(reps):
                if not flags & api.PLAN_INPUT_FROM_IN and r > 0:
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
    desc = [p.describe() for p in plans]
    for g, (a, b, ni, no, a0) in enumerate(bufs):
        assert bool((b[no:] == SENT).all()), f"device {g}: the plan wrote past r2c_counts into out"
        assert bool((a[ni:] == SENT).all()), f"device {g}: the plan wrote past r2c_counts into in"
    ins = [b[0][:b[2]].cpu().numpy() for b in bufs]
    ins0 = [b[4][:b[2]].cpu().numpy() for b in bufs]
    for p in plans:
        p.destroy()
    if comm:
        comm.destroy()
    return outs, ins, ins0, desc


PLAN_CASES = [((16, 16, 15), 1), ((16, 16, 15), 2), ((12, 10, 125), 1), ((12, 10, 125), 3), ((8, 6, 97), 1), ((8, 6, 97), 3),
              ((6, 4, 22), 1), ((6, 4, 22), 2), ((4, 4, 16384), 1), ((4, 4, 16384), 2), ((5, 7, 2187), 1), ((5, 7, 2187), 3),
              ((25, 10, 375), 1), ((25, 10, 375), 4)]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N,P", PLAN_CASES)
def test_r2c_any_plan_forward_vs_rfftn(gpu, N, P, prec):
    from distributedfft_amd import api
    x = np.random.default_rng(1).standard_normal(N).astype(_np_real(prec))
    outs, _, _, desc = _run(gpu, N, P, prec, _split_real(x, P), api.FORWARD)
    form = api.real_form(N[2])
    assert all(f"real_form={form}" in d and "pipeline=r2c" in d for d in desc), desc
    if N[2] == 16384:
        assert "complex_form=four-step/" in desc[0], desc[0]
    if N[2] in (97, 22):
        assert "complex_form=bluestein/" in desc[0], desc[0]
    ref = _split_bins(np.fft.rfftn(x.astype(np.float64)), P)
    err = max(_rel(outs[g][0][:ref[g].size].reshape(ref[g].shape), ref[g]) for g in range(P))
    assert err < TOL[prec], (N, P, prec, err)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N,P", PLAN_CASES)
def test_r2c_any_plan_backward_non_hermitian_vs_irfftn(gpu, N, P, prec):
    from distributedfft_amd import api
    n0, n1, n2 = N
    rng = np.random.default_rng(7)
    X = (rng.standard_normal((n0, n1, n2 // 2 + 1)) + 1j * rng.standard_normal((n0, n1, n2 // 2 + 1))).astype(_np_cplx(prec))
    back, _, _, desc = _run(gpu, N, P, prec, _split_bins(X, P), api.BACKWARD)
    assert all("pipeline=c2r" in d for d in desc)
    ref = _split_real(float(np.prod(N)) * np.fft.irfftn(X.astype(np.complex128), s=N, axes=(0, 1, 2)), P)
    err = max(_rel(back[g][0].reshape(ref[g].shape), ref[g]) for g in range(P))
    assert err < TOL[prec], (N, P, prec, err)


def test_r2c_any_plan_full_size_cache_chunked(gpu):
    """375^3 fp64: the Z and Y passes run per cache chunk, the paired generic rows with the plan's chunk-sized scratch."""
    import torch
    from distributedfft_amd import api
    N = (375, 375, 375)
    x = np.random.default_rng(3).standard_normal(N)
    rc, cc = api.r2c_counts(*N, 1, 0)
    a = torch.from_numpy(x.reshape(-1)).to(gpu)
    b = torch.empty(cc, dtype=torch.complex128, device=gpu)
    p = api.PlanR2C(*N, a, b, None, 0, 1, api.FORWARD, any_length=True)
    assert "chunks=1x" not in p.describe() and "real_form=2" in p.describe(), p.describe()
    p.execute()
    p.sync()
    got = b.cpu().numpy().reshape(N[1], N[2] // 2 + 1, N[0])
    c = torch.empty(rc, dtype=torch.float64, device=gpu)
    q = api.PlanR2C(*N, b, c, None, 0, 1, api.BACKWARD, any_length=True)
    q.set_scale(1.0 / float(np.prod(N)))
    q.execute()
    q.sync()
    back = c.cpu().numpy()
    p.destroy()
    q.destroy()
    ref = np.fft.rfftn(x).transpose(1, 2, 0)
    assert _rel(got, ref) < TOL["f64"]
    assert float(np.abs(back - x.reshape(-1)).max()) < 1e-11


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("N,P,prec", [((16, 16, 15), 2, "f64"), ((8, 6, 97), 1, "f32"), ((4, 4, 16384), 2, "f64"), ((12, 10, 125), 3, "f32")])
def test_r2c_any_input_from_in_guards_and_determinism(gpu, N, P, prec, direction):
    """INPUT_FROM_IN leaves `in` alone; two executes are bit-identical, and equal to the default plan's (input captured, reloaded)."""
    from distributedfft_amd import api
    x = np.random.default_rng(5).standard_normal(N).astype(_np_real(prec))
    if direction == api.FORWARD:
        inputs = _split_real(x, P)
    else:
        inputs = _split_bins(np.fft.rfftn(x.astype(np.float64)).astype(_np_cplx(prec)), P)
    outs, ins, ins0, _ = _run(gpu, N, P, prec, inputs, direction, api.PLAN_INPUT_FROM_IN, reps=2)
    for g in range(P):
        assert np.array_equal(ins[g], ins0[g]), f"device {g}: INPUT_FROM_IN wrote into in"
        assert np.array_equal(outs[g][0], outs[g][1]), f"device {g}: two executes differ"
    outs2, _, _, _ = _run(gpu, N, P, prec, inputs, direction, 0, reps=2)
    for g in range(P):
        assert np.array_equal(outs2[g][0], outs[g][0]) and np.array_equal(outs2[g][1], outs[g][0])


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("N,P", [((8, 6, 16), 1), ((12, 10, 40), 2), ((5, 4, 4802), 1)])
def test_form1_axis_bit_identical_to_r2c_plan(gpu, N, P, direction):
    """For a real axis of form 1 the any-length plan is dfft_plan_create_r2c's: the same bits in both directions."""
    from distributedfft_amd import api
    x = np.random.default_rng(9).standard_normal(N)
    if direction == api.FORWARD:
        inputs = _split_real(x, P)
    else:
        X = np.random.default_rng(10).standard_normal((N[0], N[1], N[2] // 2 + 1)) * (1 + 1j)
        inputs = _split_bins(X, P)
    a, _, _, d_any = _run(gpu, N, P, "f64", inputs, direction, any_length=True)
    b, _, _, d_old = _run(gpu, N, P, "f64", inputs, direction, any_length=False)
    assert "real_form=1" in d_any[0] and "real_form" not in d_old[0]
    for g in range(P):
        assert np.array_equal(a[g][0], b[g][0]), f"device {g}: the form-1 plans differ"
