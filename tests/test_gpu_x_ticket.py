"""Forward X pass of fp64 plans with a 512-point X axis: tiles handed out by a ticket counter the plan owns, early wait for the prefetched
tile (TuneTransposedStoreTicketEarly, csrc/dfft_fft_impl.h).  The order of the tiles changes, a tile's arithmetic does not: every form
must produce bit for bit what the static grid-stride loop produces, with the early wait (DFFT_X_VARIANT=static) and with the late one
(static-late, the kernel up to round 6).  Shapes: tiles = N1 * N2 / 8, against 256 workgroups."""
import numpy as np
import pytest

from oracle import slab_oracle as so

pytestmark = pytest.mark.gpu

TOL = {"f64": 1e-11, "f32": 5e-4}  # the suite's bound (tests/test_gpu_parity.py): max error over max |reference|
# 64 tiles: fewer than workgroups, most of them draw only their two end tickets; 320: a ragged second round; 1024: four rounds
SHAPES = [(512, 8, 64), (512, 40, 64), (512, 64, 128)]
_cache = {}


def _case(N):
    """Input and numpy.fft.fftn reference of a shape, computed once and shared (never modified)."""
    if N not in _cache:
        x = so.random_input(N, seed=N[1] * 1009 + N[2])
        ref = so.fftn_reference(x, 1)[0]
        x.setflags(write=False)
        ref.setflags(write=False)
        _cache[N] = (x, ref)
    return _cache[N]


def _plan(gpu, N, x, prec="f64"):
    import torch
    from distributedfft_amd import api
    tdt = torch.complex128 if prec == "f64" else torch.complex64
    a = torch.tensor(x.reshape(-1), device=gpu).to(tdt)  # (a copy: the shared input is read-only)
    b = torch.zeros_like(a)
    torch.cuda.synchronize()
    return api.Plan(*N, a, b, None, 0, 1, api.FORWARD, api.PLAN_INPUT_FROM_IN), a, b


def _forward(gpu, N, x, monkeypatch, variant=None, prec="f64", tune=False):
    """One execute of a freshly created plan; returns (result, describe after the execute)."""
    if variant is None:
        monkeypatch.delenv("DFFT_X_VARIANT", raising=False)
    else:
        monkeypatch.setenv("DFFT_X_VARIANT", variant)
    p, a, b = _plan(gpu, N, x, prec)
    try:
        if tune:
            p.tune()
        p.execute()
        p.sync()
        return b.cpu().numpy(), p.describe()
    finally:
        p.destroy()


@pytest.mark.parametrize("N", SHAPES, ids=lambda N: "x".join(map(str, N)))
def test_ticketed_x_pass_equals_the_static_loop_bit_for_bit(gpu, N, monkeypatch):
    x, ref = _case(N)
    got, desc = _forward(gpu, N, x, monkeypatch)
    assert "x_variant=ticket-early-wait" in desc, desc
    err = np.abs(got.reshape(ref.shape) - ref).max() / np.abs(ref).max()
    print(f"{N}: max error / max |reference| = {err:.3e}")
    assert err < TOL["f64"], (N, err)
    # the static loop, the late wait, and both (the reference form): each A/B partner on its own
    for variant, name in (("static", "static-early-wait"), ("late", "ticket-late-wait"), ("static-late", "static-late-wait")):
        want, d = _forward(gpu, N, x, monkeypatch, variant)
        assert f"x_variant={name}" in d, (variant, d)
        assert np.array_equal(got, want), (N, variant)


def test_back_to_back_executes_and_an_interleaved_second_plan(gpu, monkeypatch):
    """Three executes of one plan with no synchronisation in between, a second plan of another shape in between them: every execute
    starts where the one before left the counter (ticket base += tiles + 2 * workgroups, never reset), and every workgroup has drawn
    exactly its two end tickets -- else a later execute skips or repeats tiles.  A plan launches on a stream of its own, so the two
    streams are chained launch by launch with events (A1 B1 A2 B2 A3 B3 in one device-side order, as on one stream); results are set
    aside by copies on the plan's stream, without a host wait."""
    import torch
    monkeypatch.delenv("DFFT_X_VARIANT", raising=False)
    NA, NB = (512, 40, 64), (512, 8, 64)
    xa, refa = _case(NA)
    xb, refb = _case(NB)
    pa, _, ba = _plan(gpu, NA, xa)
    pb, _, bb = _plan(gpu, NB, xb)
    try:
        sa, sb = torch.cuda.ExternalStream(pa.stream), torch.cuda.ExternalStream(pb.stream)
        snaps_a, snaps_b = [], []
        for _ in range(3):
            pa.execute()
            with torch.cuda.stream(sa):
                snaps_a.append(ba.clone())
            sb.wait_stream(sa)
            pb.execute()
            with torch.cuda.stream(sb):
                snaps_b.append(bb.clone())
            sa.wait_stream(sb)
        pa.sync()
        pb.sync()
        assert "x_variant=ticket-early-wait" in pa.describe() and "x_variant=ticket-early-wait" in pb.describe()
        for snaps, ref in ((snaps_a, refa), (snaps_b, refb)):
            first = snaps[0].cpu().numpy()
            assert np.abs(first.reshape(ref.shape) - ref).max() / np.abs(ref).max() < TOL["f64"]
            for i, s in enumerate(snaps[1:], 2):
                assert np.array_equal(s.cpu().numpy(), first), f"execute {i}"
    finally:
        pa.destroy()
        pb.destroy()


def test_execute_right_after_plan_tune(gpu, monkeypatch):
    """dfft_plan_tune probes with the plan's own X-pass launches, counter included: they move the ticket base on like executes do."""
    N = (512, 40, 64)
    x, _ = _case(N)
    monkeypatch.setenv("DFFT_PAD", "1")         # a padded hand-over buffer at this size: the only kind dfft_plan_tune places
    monkeypatch.setenv("DFFT_TUNE_TRIES", "5")  # (candidates of 20 MiB all behave alike: the walk runs to its bound)
    want, _ = _forward(gpu, N, x, monkeypatch, "static-late")
    got, desc = _forward(gpu, N, x, monkeypatch, tune=True)
    assert "x_variant=ticket-early-wait" in desc and "tuned=1" in desc, desc
    assert np.array_equal(got, want)


def test_fp32_pairs_keep_their_kernel(gpu, monkeypatch):
    """fp32 column pairs lose a quarter with the early wait and have no ticket counter: same kernel, same description as before."""
    N = (512, 8, 64)
    x, ref = _case(N)
    got, desc = _forward(gpu, N, x, monkeypatch, prec="f32")
    assert "x_variant=default" in desc, desc
    assert np.abs(got.reshape(ref.shape) - ref).max() / np.abs(ref).max() < TOL["f32"]
    for variant in ("static", "late", "static-late"):  # switches of the fp64 kernel: nothing to select here
        want, d = _forward(gpu, N, x, monkeypatch, variant, prec="f32")
        assert "x_variant=default" in d, (variant, d)
        assert np.array_equal(got, want), variant
