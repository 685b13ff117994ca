"""-m gpu: the state the plan-less entry points carry from one call to the next, checked call by call against numpy.

dfft_fft2d_batch caches, per (device, stream, n1, n2, direction), the control block of its one-launch stage (dfft_zy.hip) with the
host's running ticket / execute counters; dfft_fft1d_rows / dfft_fft1d_cols keep a grow-only four-step scratch buffer per (device,
stream) (dfft_long.hip); all of them share the twiddle caches.  A single call per test never exercises any of that: here every test
runs a SEQUENCE of calls on one stream -- batch sizes that grow, shrink and grow again, Infinity-Cache phases, both directions, in
place and out of place, fp32 between fp64, dfft_trim() in the middle, the ZY_MAX_PLANES edge, several host threads -- and compares the
output of every call (a counter out of step makes column units read unpublished rows: O(1) errors, far above the bars).

The C entry points are called directly on a torch stream of the test's own and that stream is waited for; dfft_fft2d_batch_status()
then reports a one-launch stage that gave up (ZY_ERR_DESYNC: counters out of step) on the call that made it.  torch hands streams out
of a pool, so a test may meet a context an earlier test left behind on the same stream: the results must not depend on that either.
Bars: relative max error 1e-11 (fp64), 5e-4 (fp32), as in test_gpu_parity.py."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = {"f64": 1e-11, "f32": 5e-4}
# the plane shapes the one-launch stage is built for (dfft_zy.hip: zy_supported), fp64 only
ZY_SHAPES = [(256, 256), (256, 512), (512, 256), (512, 512), (768, 512)]
ZY_MAX_PLANES = 4096  # dfft_zy.h


def _rel_err(got, ref):
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-300))


def _torch_dtype(prec):
    import torch
    return torch.complex128 if prec == "f64" else torch.complex64


def _planes(seed, batch, n1, n2):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (batch, n1, n2)) + 1j * rng.uniform(-1, 1, (batch, n1, n2))


def _ref2d(x, direction):
    from distributedfft_amd import api
    return np.fft.fft2(x, axes=(1, 2)) if direction == api.FORWARD else np.fft.ifft2(x, axes=(1, 2)) * (x.shape[1] * x.shape[2])


def _fft2d(x, out, direction, stream):
    """dfft_fft2d_batch of the (batch, n1, n2) tensor x into out on `stream`; waits for the stream and reads the stage's status."""
    from distributedfft_amd import _lib, api
    lib = _lib.load()
    _lib.check(lib.dfft_fft2d_batch(x.data_ptr(), out.data_ptr(), x.shape[1], x.shape[2], x.shape[0], api._dtype_code(x), direction,
                                    stream.cuda_stream), "dfft_fft2d_batch")
    stream.synchronize()
    _lib.check(lib.dfft_fft2d_batch_status(stream.cuda_stream), "dfft_fft2d_batch_status")
    return out


def _run_sequence(gpu, stream, n1, n2, steps, seed, prec="f64"):
    """steps: (batch, direction, in_place) per call; every call's output is compared with numpy, out-of-place inputs must stay put."""
    import torch
    for i, (batch, direction, in_place) in enumerate(steps):
        x = _planes(seed + 7919 * i, batch, n1, n2)
        xt = torch.from_numpy(x).to(gpu).to(_torch_dtype(prec))
        keep = None if in_place else xt.clone()
        out = xt if in_place else torch.empty_like(xt)
        torch.cuda.synchronize()  # inputs are written on the default stream
        got = _fft2d(xt, out, direction, stream).cpu().numpy()
        err = _rel_err(got, _ref2d(x, direction))
        assert err < TOL[prec], f"call {i} of {steps} ({n1}x{n2} {prec}): rel err {err:.3e}"
        if keep is not None:
            assert torch.equal(xt, keep), f"call {i} of {steps}: out of place, but the input changed"


def _fwd(*batches):
    from distributedfft_amd import api
    return [(b, api.FORWARD, False) for b in batches]


# ---- batch sequences on one context ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2", ZY_SHAPES)
def test_growing_batches_on_one_stream(gpu, n1, n2):
    import torch
    _run_sequence(gpu, torch.cuda.Stream(gpu), n1, n2, _fwd(1, 2, 8, 3), seed=11)


@pytest.mark.parametrize("n1,n2", ZY_SHAPES)
def test_shrink_then_grow_on_one_stream(gpu, n1, n2):
    import torch
    _run_sequence(gpu, torch.cuda.Stream(gpu), n1, n2, _fwd(8, 2, 8), seed=12)


@pytest.mark.parametrize("n1,n2", ZY_SHAPES)
def test_infinity_cache_phases_then_batch_1(gpu, n1, n2):
    """More planes than fit 256 MiB (512 x 512 fp64: more than 64), so the launch runs in several phases; then a single plane."""
    import torch
    phased = (256 << 20) // (n1 * n2 * 16) + 6
    _run_sequence(gpu, torch.cuda.Stream(gpu), n1, n2, _fwd(phased, 1), seed=13)


@pytest.mark.parametrize("n1,n2", ZY_SHAPES)
def test_forward_and_backward_interleaved(gpu, n1, n2):
    import torch
    from distributedfft_amd import api
    F, B = api.FORWARD, api.BACKWARD
    steps = [(2, F, False), (2, B, False), (5, F, False), (1, B, False), (1, F, False), (5, B, False), (3, B, True), (3, F, True)]
    _run_sequence(gpu, torch.cuda.Stream(gpu), n1, n2, steps, seed=14)


@pytest.mark.parametrize("n1,n2", ZY_SHAPES)
def test_in_place_and_out_of_place_mixed(gpu, n1, n2):
    import torch
    from distributedfft_amd import api
    F = api.FORWARD
    steps = [(3, F, False), (3, F, True), (1, F, False), (4, F, True), (4, F, False), (2, F, True)]
    _run_sequence(gpu, torch.cuda.Stream(gpu), n1, n2, steps, seed=15)


@pytest.mark.parametrize("n1,n2", ZY_SHAPES)
def test_fp32_interleaved_with_fp64(gpu, n1, n2):
    """The context key has no dtype: fp32 calls (two launches per chunk) between fp64 calls (one launch) on the same shape."""
    import torch
    from distributedfft_amd import api
    s = torch.cuda.Stream(gpu)
    for i, (prec, batch) in enumerate([("f64", 2), ("f32", 2), ("f64", 3), ("f32", 1), ("f64", 1), ("f32", 5), ("f64", 5)]):
        _run_sequence(gpu, s, n1, n2, [(batch, api.FORWARD, i % 3 == 1)], seed=16 + i, prec=prec)


def test_trim_in_the_middle_of_a_sequence(gpu):
    """dfft_trim() drops every cached context; the next calls rebuild theirs and stay right."""
    import torch
    from distributedfft_amd import _lib, api
    s = torch.cuda.Stream(gpu)
    for n1, n2 in [(512, 512), (256, 512)]:
        _run_sequence(gpu, s, n1, n2, _fwd(1, 2), seed=17)
        _run_sequence(gpu, s, n1, n2, [(2, api.BACKWARD, False)], seed=18)
        _lib.check(_lib.load().dfft_trim(), "dfft_trim")
        _run_sequence(gpu, s, n1, n2, _fwd(2, 8, 1), seed=19)
        _run_sequence(gpu, s, n1, n2, [(3, api.BACKWARD, True)], seed=20)


# ---- streams and host threads ---------------------------------------------------------------------------------------------------
def _in_threads(fns):
    errors = []

    def wrap(fn):
        try:
            fn()
        except BaseException as e:  # noqa: BLE001 -- reported below, with the thread's traceback text
            errors.append(e)

    ts = [threading.Thread(target=wrap, args=(fn,)) for fn in fns]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=600)
    assert not any(t.is_alive() for t in ts), "a host thread did not finish"
    assert not errors, errors


@pytest.mark.parametrize("n1,n2", [(512, 512), (256, 256)])
def test_two_streams_from_two_threads(gpu, n1, n2):
    """Same shape on two streams at once: a context each."""
    import torch
    streams = [torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)]
    seqs = [_fwd(1, 2, 8, 3, 8, 1), _fwd(8, 2, 8, 1, 3, 2)]

    def job(k):
        torch.cuda.set_device(gpu)
        _run_sequence(gpu, streams[k], n1, n2, seqs[k], seed=21 + 100 * k)

    _in_threads([lambda: job(0), lambda: job(1)])


@pytest.mark.parametrize("n1,n2", [(512, 512), (256, 256)])
def test_two_threads_on_one_stream_with_different_batches(gpu, n1, n2):
    """Two host threads share one stream and so one context (under its mutex) while their batch sizes keep changing it."""
    import torch
    s = torch.cuda.Stream(gpu)
    seqs = [_fwd(1, 3, 1, 3, 1, 3), _fwd(2, 5, 2, 8, 2, 5)]

    def job(k):
        torch.cuda.set_device(gpu)
        _run_sequence(gpu, s, n1, n2, seqs[k], seed=31 + 100 * k)

    _in_threads([lambda: job(0), lambda: job(1)])


# ---- the ZY_MAX_PLANES edge -----------------------------------------------------------------------------------------------------
def test_zy_max_planes_edge_then_batch_1(gpu):
    """256 x 256 fp64: ZY_MAX_PLANES planes (one launch), one plane more (two launches per chunk), then a single plane again, all on
    one stream.  4 GiB per batch, so the input is generated on the GPU and a fixed sample of planes is compared with numpy."""
    import torch
    from distributedfft_amd import api
    n1 = n2 = 256
    s = torch.cuda.Stream(gpu)
    for batch, seed in [(ZY_MAX_PLANES, 41), (ZY_MAX_PLANES + 1, 42), (1, 43)]:
        g = torch.Generator(device=gpu)
        g.manual_seed(seed)
        x = torch.randn((batch, n1, n2), dtype=torch.complex128, device=gpu, generator=g)
        rng = np.random.default_rng(seed)
        sample = sorted({0, batch - 1, *rng.integers(0, batch, 8).tolist()})
        before = x[sample].cpu().numpy()
        out = torch.empty_like(x)
        torch.cuda.synchronize()
        _fft2d(x, out, api.FORWARD, s)
        got = out[sample].cpu().numpy()
        for k, p in enumerate(sample):
            err = _rel_err(got[k], np.fft.fft2(before[k]))
            assert err < TOL["f64"], f"batch {batch}, plane {p}: rel err {err:.3e}"
        assert np.array_equal(x[sample].cpu().numpy(), before), f"batch {batch}: out of place, but the input changed"
        del x, out
        torch.cuda.empty_cache()


# ---- the four-step scratch buffer of the 1-D entry points -----------------------------------------------------------------------
def _fft1d(kind, x, out, direction, stream):
    from distributedfft_amd import _lib, api
    lib = _lib.load()
    if kind == "rows":
        rc = lib.dfft_fft1d_rows(x.data_ptr(), out.data_ptr(), x.shape[1], x.shape[0], api._dtype_code(x), direction, stream.cuda_stream)
    else:
        rc = lib.dfft_fft1d_cols(x.data_ptr(), out.data_ptr(), x.shape[1], x.shape[2], x.shape[0], api._dtype_code(x), direction,
                                 stream.cuda_stream)
    _lib.check(rc, f"dfft_fft1d_{kind}")
    stream.synchronize()
    return out


def _run_1d(gpu, stream, steps, seed):
    """steps: (kind, n, in_place); rows: (4, n) batches, columns: (2, n, 8).  Each call compared with np.fft.fft along its axis."""
    import torch
    from distributedfft_amd import api
    for i, (kind, n, in_place) in enumerate(steps):
        rng = np.random.default_rng(seed + 131 * i)
        shape, axis = ((4, n), 1) if kind == "rows" else ((2, n, 8), 1)
        x = rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)
        xt = torch.from_numpy(x).to(gpu)
        keep = None if in_place else xt.clone()
        out = xt if in_place else torch.empty_like(xt)
        torch.cuda.synchronize()
        got = _fft1d(kind, xt, out, api.FORWARD, stream).cpu().numpy()
        err = _rel_err(got, np.fft.fft(x, axis=axis))
        assert err < TOL["f64"], f"call {i} of {steps}: rel err {err:.3e}"
        if keep is not None:
            assert torch.equal(xt, keep), f"call {i} of {steps}: out of place, but the input changed"


def test_four_step_scratch_grows_and_is_reused(gpu):
    """n = 8192, then 65536 (the scratch buffer grows), then 8192 again on one stream, columns and rows, with in-place calls."""
    import torch
    steps = [("cols", 8192, False), ("rows", 8192, False), ("cols", 65536, False), ("rows", 65536, True),
             ("cols", 8192, True), ("rows", 8192, False), ("rows", 65536, False), ("cols", 8192, False)]
    _run_1d(gpu, torch.cuda.Stream(gpu), steps, seed=51)


def test_four_step_scratch_two_threads_on_one_stream(gpu):
    import torch
    s = torch.cuda.Stream(gpu)
    seqs = [[("rows", 8192, False), ("cols", 8192, True)] * 3, [("cols", 65536, False), ("rows", 65536, True)] * 3]

    def job(k):
        torch.cuda.set_device(gpu)
        _run_1d(gpu, s, seqs[k], seed=61 + 1000 * k)

    _in_threads([lambda: job(0), lambda: job(1)])


# ---- the Python wrappers check `out` --------------------------------------------------------------------------------------------
def test_wrappers_reject_a_mismatched_out(gpu):
    import torch
    from distributedfft_amd import api
    cases = [(api.fft1d_rows, (3, 64)), (api.fft1d_cols, (2, 64, 8)), (api.fft2d_batch, (2, 64, 32))]
    for fn, shape in cases:
        x = torch.zeros(shape, dtype=torch.complex128, device=gpu)
        bad = [torch.empty(shape[:-1] + (shape[-1] + 1,), dtype=torch.complex128, device=gpu),      # shape
               torch.empty(shape, dtype=torch.complex64, device=gpu),                               # dtype
               torch.empty(shape, dtype=torch.complex128),                                          # device
               torch.empty(shape[::-1], dtype=torch.complex128, device=gpu).permute(*range(len(shape) - 1, -1, -1))]  # not contiguous
        assert bad[-1].shape == x.shape and not bad[-1].is_contiguous()
        for out in bad:
            with pytest.raises(AssertionError):
                fn(x, api.FORWARD, out=out)
        fn(x, api.FORWARD, out=torch.empty_like(x))  # a matching one is taken
