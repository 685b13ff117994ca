"""-m gpu: real-to-real transforms (DCT / DST, types II and III) -- dfft_r2r1d_strided against the float64 references of
tests/test_r2r_host.py (the direct sums up to n = 1024, the mirror reference above) for every form of n (fused columns and rows, tuned
lengths odd and even; run-time-scheduled, four-step and Bluestein lengths on the composed route), odd and even s, odd row counts at
s = 1, all four kinds and both precisions; the round trip (type III of type II = 2n x), guard regions, untouched input, in place
bit-identical to out of place, misaligned pointers, DFFT_R2R_FUSED=0 against the fused route, two streams with dfft_trim in between,
and api.r2r / api.r2rn.

Error measure: max |got - ref| / max |ref| over the whole output; bounds 1e-11 (fp64) and 5e-4 (fp32), those of
tests/test_gpu_real_strided.py -- the same pair arithmetic plus one twiddle multiply.

Cross-talk: the two sequences of a pair share one complex transform, so a sequence's rounding error is bounded by the tolerance times
the PAIR's combined magnitude, not its own: a column 10^-6 the size of its neighbour keeps an absolute error of at most the tolerance
times the neighbour's magnitude (test_pair_cross_talk_bound).

The per-length sweep -- every tuned length of this family, both precisions, every kernel variant -- lives in tests/test_gpu_tuned_sweep.py."""
import ctypes as C
import os
import re
from pathlib import Path

import numpy as np
import pytest

from test_r2r_host import KINDS, reference

pytestmark = pytest.mark.gpu
TOL = {"f64": 1e-11, "f32": 5e-4}
GUARD = 64
SENT = -12345.0

TUNED_EVEN = [16, 512, 2048]
TUNED_ODD = [125, 243]
GENERIC = [15, 375]
FOUR_STEP = [16384]
BLUESTEIN = [1, 11, 97, 1009]
ALL_N = TUNED_EVEN + TUNED_ODD + GENERIC + FOUR_STEP + BLUESTEIN
S_VALUES = [1, 2, 3, 7, 64, 257]
INVERSE = {"dct2": "dct3", "dst2": "dst3"}


def _rel(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def _rdt(prec):
    import torch
    return torch.float64 if prec == "f64" else torch.float32


def _code(prec):
    from distributedfft_amd import _lib as L
    return L.F64 if prec == "f64" else L.F32


def _call(inp, out, n, s, batch, prec, kind, stream=None):
    from distributedfft_amd import _lib as L
    lib = L.load()
    rc = lib.dfft_r2r1d_strided(C.c_void_p(inp), C.c_void_p(out), n, s, batch, _code(prec), KINDS[kind], C.c_void_p(stream) if stream else None)
    assert rc == 0, (rc, lib.dfft_last_error().decode())


def _guarded(count, dtype, gpu):
    import torch
    buf = torch.full((count + 2 * GUARD,), SENT, dtype=dtype, device=gpu)
    return buf, buf[GUARD:GUARD + count]


def _guards_intact(buf):
    h = buf.cpu()
    return bool((h[:GUARD] == SENT).all() and (h[-GUARD:] == SENT).all())


def _batch_for(n, s):
    return max(1, min(3, 2_000_000 // (n * s)))


def _data(rng, batch, n, s):
    """float64 values that float32 holds exactly, so both precisions share one input and one reference"""
    return rng.standard_normal((batch, n, s)).astype(np.float32).astype(np.float64)


def _transform(gpu, x, kind, prec, inplace=False):
    """x: numpy [batch][n][s] -> numpy result; checks the guard regions of `out` and, out of place, that `in` is unchanged"""
    import torch
    batch, n, s = x.shape
    xi = torch.from_numpy(x).to(_rdt(prec)).to(gpu)
    buf, out = _guarded(batch * n * s, _rdt(prec), gpu)
    if inplace:
        out.copy_(xi.reshape(-1))
        _call(out.data_ptr(), out.data_ptr(), n, s, batch, prec, kind)
    else:
        before = xi.clone()
        _call(xi.data_ptr(), out.data_ptr(), n, s, batch, prec, kind)
    torch.cuda.synchronize()
    if not inplace:
        assert torch.equal(xi, before), "in was written"
    assert _guards_intact(buf), "guard region overwritten"
    return out.cpu().numpy().astype(np.float64).reshape(batch, n, s)


def _check_shape(gpu, rng, n, s, batch, report):
    """all four kinds, both precisions, out of place against the reference, in place bit-identical, and the round trip"""
    x = _data(rng, batch, n, s)
    refs = {kind: reference(x, kind) for kind in KINDS}
    for prec in ("f64", "f32"):
        for kind in KINDS:
            got = _transform(gpu, x, kind, prec)
            err = _rel(got, refs[kind])
            report.append((n, s, batch, prec, kind, err))
            print(f"r2r n={n} s={s} batch={batch} {prec} {kind}: err {err:.3e}")
            assert err < TOL[prec], (n, s, batch, prec, kind, err)
            same = _transform(gpu, x, kind, prec, inplace=True)
            assert np.array_equal(same, got), ("in place differs from out of place", n, s, batch, prec, kind)
            if kind in INVERSE:  # type III of type II = 2n x
                y = got if prec == "f64" else got.astype(np.float32).astype(np.float64)
                back = _transform(gpu, y, INVERSE[kind], prec)
                err = _rel(back, 2 * n * x)
                print(f"r2r n={n} s={s} batch={batch} {prec} {INVERSE[kind]}({kind}): err {err:.3e}")
                assert err < TOL[prec], ("round trip", n, s, batch, prec, kind, err)


@pytest.mark.parametrize("n", ALL_N)
def test_every_kind_vs_reference(gpu, n):
    rng = np.random.default_rng(n)
    report = []
    for s in S_VALUES:
        _check_shape(gpu, rng, n, s, _batch_for(n, s), report)
    for batch in (3, 5):  # s = 1: an odd last row is paired with zeros
        _check_shape(gpu, rng, n, 1, batch, report)


def _tuned_lengths():
    plans = (Path(__file__).resolve().parent.parent / "distributedfft_amd" / "csrc" / "dfft_plans.h").read_text()
    return sorted({int(v) for v in re.findall(r"^\s*X\((\d+),", plans, re.M)} | {768})


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("three", [False, True])
def test_fused_sweep_every_tuned_length(gpu, prec, three):
    """Every tuned length on every fused form -- rows (s = 1, three rows), column pairs as one value (s = 2) and as two reals (s = 3,
    an odd last column) -- or, for the few instantiations routed there, the composed route."""
    lengths = _tuned_lengths()
    assert len(lengths) == 49
    rng = np.random.default_rng(17)
    for n in lengths:
        for s, batch in ((1, 3), (2, 1), (3, 2)):
            x = _data(rng, batch, n, s)
            for kind in (("dct3", "dst3") if three else ("dct2", "dst2")):
                err = _rel(_transform(gpu, x, kind, prec), reference(x, kind))
                assert err < TOL[prec], (n, s, prec, kind, err)


@pytest.mark.parametrize("n", [512, 125, 15, 97])
@pytest.mark.parametrize("s", [64, 7])
def test_pointers_offset_by_one_element(gpu, n, s):
    """in and out one element past an allocation's start: a column pair is then not aligned to two reals, so an even s must not take
    the two-element loads / stores."""
    import torch
    rng = np.random.default_rng(n * s)
    batch = 3
    x = _data(rng, batch, n, s)
    for prec in ("f64", "f32"):
        eb = 8 if prec == "f64" else 4
        for kind in KINDS:
            ib = torch.zeros(batch * n * s + 1, dtype=_rdt(prec), device=gpu)
            ib[1:] = torch.from_numpy(x.reshape(-1)).to(_rdt(prec)).to(gpu)
            ob = torch.full((batch * n * s + 2,), SENT, dtype=_rdt(prec), device=gpu)
            _call(ib.data_ptr() + eb, ob.data_ptr() + eb, n, s, batch, prec, kind)
            torch.cuda.synchronize()
            assert ob[0].item() == SENT and ob[-1].item() == SENT
            got = ob[1:-1].cpu().numpy().astype(np.float64).reshape(batch, n, s)
            err = _rel(got, reference(x, kind))
            assert err < TOL[prec], (n, s, prec, kind, err)
            # in place at the odd offset
            _call(ib.data_ptr() + eb, ib.data_ptr() + eb, n, s, batch, prec, kind)
            torch.cuda.synchronize()
            assert ib[0].item() == 0.0
            assert np.array_equal(ib[1:].cpu().numpy().astype(np.float64).reshape(batch, n, s), got)


@pytest.mark.parametrize("n", [16, 125, 512])
def test_composed_route_agrees_with_the_fused_route(gpu, n):
    """DFFT_R2R_FUSED=0 (read per call) sends a fused length through pre kernel -> n-point transform -> post kernel."""
    rng = np.random.default_rng(n + 3)
    old = os.environ.get("DFFT_R2R_FUSED")
    try:
        for s, batch in ((1, 5), (2, 3), (7, 3), (64, 3)):
            x = _data(rng, batch, n, s)
            for prec in ("f64", "f32"):
                for kind in KINDS:
                    os.environ.pop("DFFT_R2R_FUSED", None)
                    fused = _transform(gpu, x, kind, prec)
                    os.environ["DFFT_R2R_FUSED"] = "0"
                    composed = _transform(gpu, x, kind, prec)
                    inplace = _transform(gpu, x, kind, prec, inplace=True)
                    ref = reference(x, kind)
                    assert _rel(composed, ref) < TOL[prec], (n, s, prec, kind)
                    assert _rel(composed, fused) < TOL[prec], (n, s, prec, kind)
                    assert np.array_equal(inplace, composed)
    finally:
        if old is None:
            os.environ.pop("DFFT_R2R_FUSED", None)
        else:
            os.environ["DFFT_R2R_FUSED"] = old


def test_two_streams_and_trim(gpu):
    """Two streams interleaved with different n (fused 512, composed 375 and 97 with per-stream scratch); dfft_trim between calls
    frees the scratch and the tables, and the calls after it are still correct."""
    import torch
    from distributedfft_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng(11)
    s, batch = 66, 3
    cases = [(512, "dct2"), (375, "dct3"), (97, "dst2")]
    xs = {n: _data(rng, batch, n, s) for n, _ in cases}
    refs = {n: reference(xs[n], kind) for n, kind in cases}
    streams = [torch.cuda.Stream(gpu) for _ in range(2)]
    for rnd in range(3):
        outs = []
        for i, (n, kind) in enumerate(cases + cases[::-1]):
            st = streams[i % 2]
            xi = torch.from_numpy(xs[n]).to(gpu)
            o = torch.empty_like(xi)
            st.wait_stream(torch.cuda.current_stream(gpu))
            _call(xi.data_ptr(), o.data_ptr(), n, s, batch, "f64", kind, stream=st.cuda_stream)
            outs.append((n, xi, o))
        torch.cuda.synchronize()
        for n, _, o in outs:
            assert _rel(o.cpu().numpy(), refs[n]) < TOL["f64"], (rnd, n)
        assert lib.dfft_trim() == 0


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n", [512, 125, 15, 97])
def test_pair_cross_talk_bound(gpu, n, prec):
    """Odd columns 10^-6 the size of their even neighbours: every column's absolute error is bounded by the tolerance times its pair's
    combined magnitude."""
    rng = np.random.default_rng(5)
    s, batch = 64, 2
    x = rng.standard_normal((batch, n, s))
    x[:, :, 1::2] *= 1e-6
    x = x.astype(np.float32).astype(np.float64)
    for kind in KINDS:
        got = _transform(gpu, x, kind, prec)
        ref = reference(x, kind)
        pair = np.maximum(np.abs(ref[:, :, 0::2]).max(axis=1), np.abs(ref[:, :, 1::2]).max(axis=1))   # [batch][s / 2]
        err_small = np.abs(got[:, :, 1::2] - ref[:, :, 1::2]).max(axis=1)
        err_big = np.abs(got[:, :, 0::2] - ref[:, :, 0::2]).max(axis=1)
        assert (err_small <= TOL[prec] * pair).all(), (n, prec, kind, float((err_small / pair).max()))
        assert (err_big <= TOL[prec] * pair).all(), (n, prec, kind, float((err_big / pair).max()))


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_api_r2r_dims_and_out(gpu, prec):
    import torch
    from distributedfft_amd import api
    rng = np.random.default_rng(23)
    x = rng.standard_normal((6, 16, 10)).astype(np.float32).astype(np.float64)
    xt = torch.from_numpy(x).to(_rdt(prec)).to(gpu)
    for dim in (0, 1, 2):
        b, n, s = int(np.prod(x.shape[:dim])), x.shape[dim], int(np.prod(x.shape[dim + 1:]))
        for kind in KINDS:
            ref = reference(x.reshape(b, n, s), kind).reshape(x.shape)
            y = api.r2r(xt, kind, dim=dim)
            assert tuple(y.shape) == x.shape and y.dtype == xt.dtype
            assert _rel(y.cpu().numpy().astype(np.float64), ref) < TOL[prec], (dim, kind)
            y2 = api.r2r(xt, kind, dim=dim - 3, out=torch.empty_like(xt))
            assert torch.equal(y2, y)
            z = xt.clone()
            assert api.r2r(z, kind, dim=dim, out=z) is z   # out=x: in place
            assert torch.equal(z, y)
    with pytest.raises(AssertionError):
        api.r2r(xt, "dct2", out=torch.empty((6, 16, 11), dtype=xt.dtype, device=gpu))
    with pytest.raises(AssertionError):
        api.r2r(xt, "dct2", out=torch.empty(x.shape, dtype=torch.float32 if prec == "f64" else torch.float64, device=gpu))
    with pytest.raises(AssertionError):
        api.r2r(xt, "dct2", out=torch.empty((6, 10, 16), dtype=xt.dtype, device=gpu).transpose(1, 2))
    with pytest.raises(ValueError):
        api.r2r(xt, "dct4")
    for bad in (3, -4):
        with pytest.raises(IndexError):
            api.r2r(xt, "dct2", dim=bad)


def test_api_r2rn_mixed_kinds(gpu):
    import torch
    from distributedfft_amd import api
    rng = np.random.default_rng(29)
    x = rng.standard_normal((16, 15, 12))
    kinds = ["dct2", "dst2", "dct2"]
    ref = x
    for d, kind in enumerate(kinds):
        b, n, s = int(np.prod(x.shape[:d])), x.shape[d], int(np.prod(x.shape[d + 1:]))
        ref = reference(ref.reshape(b, n, s), kind).reshape(x.shape)
    xt = torch.from_numpy(x).to(gpu)
    before = xt.clone()
    y = api.r2rn(xt, kinds)
    assert torch.equal(xt, before)
    assert _rel(y.cpu().numpy(), ref) < TOL["f64"]
    y2 = api.r2rn(xt, kinds[::-1], dims=[2, 1, 0])   # the transforms of different axes commute
    assert _rel(y2.cpu().numpy(), ref) < TOL["f64"]
    z = xt.clone()
    assert api.r2rn(z, kinds, out=z) is z
    assert torch.equal(z, y)
    with pytest.raises(ValueError):
        api.r2rn(xt, ["dct2", "dct2"], dims=[1, -2])


def test_neumann_poisson_solve(gpu):
    """The README's solve: cell-centred second-order Laplacian with homogeneous Neumann walls on 16^3, diagonal in the DCT-II basis --
    u = r2rn(r2rn(f, dct2 x 3) / lambda, dct3 x 3) / (2n)^3 recovers a manufactured zero-mean solution."""
    import torch
    from distributedfft_amd import api
    n = 16
    rng = np.random.default_rng(31)
    u = rng.standard_normal((n, n, n))
    u -= u.mean()
    f = np.zeros_like(u)
    for ax in range(3):   # mirror ghost cells: du/dn = 0 at the walls
        p = np.concatenate([np.take(u, [0], axis=ax), u, np.take(u, [n - 1], axis=ax)], axis=ax)
        f += np.take(p, range(2, n + 2), axis=ax) - 2 * u + np.take(p, range(0, n), axis=ax)
    lam1 = 2 * np.cos(np.pi * np.arange(n) / n) - 2
    lam = lam1[:, None, None] + lam1[None, :, None] + lam1[None, None, :]
    lam[0, 0, 0] = 1.0   # the constant mode: f has none, and the solution's mean is fixed to zero
    ft = torch.from_numpy(f).to(gpu)
    fh = api.r2rn(ft, ["dct2"] * 3) / torch.from_numpy(lam).to(gpu)
    fh[0, 0, 0] = 0.0
    got = api.r2rn(fh.contiguous(), ["dct3"] * 3) / (2 * n) ** 3
    assert _rel(got.cpu().numpy(), u) < TOL["f64"]


# ---- the composed route's batch chunks (tests/large_extent.py: tiled inputs, every line checked) ------------------------------------------------
# (n, s, prec, kinds, environment, odd rows): two whole scratch chunks and a ragged third, by the mirrored chunk rule.  375 points: the
# run-time-scheduled inner transform; s = 1 with an odd row count: the last pair of the last chunk is half empty; 16384: four-step inner,
# scratch 2 zb; 1009: Bluestein inner, one launch, and -- DFFT_BLUESTEIN_FUSED=0 -- its own chunks inside an r2r chunk; 512 points are a
# fused length that DFFT_R2R_FUSED=0 sends to the composed route.
CHUNK_EDGE = [
    (375, 1000, "f64", ("dct2", "dct3", "dst2", "dst3"), {}, False),
    (375, 1, "f64", ("dct2", "dst3"), {}, True),
    (16384, 6, "f64", ("dct3", "dst2"), {}, False),
    (1009, 7, "f64", ("dct2", "dst3"), {}, False),
    (1009, 7, "f64", ("dct3", "dst2"), {"DFFT_BLUESTEIN_FUSED": "0"}, False),
    (512, 64, "f32", ("dct2", "dst3"), {"DFFT_R2R_FUSED": "0"}, False),
]


def _chunk_edge_params():
    for n, s, prec, kinds, env, odd in CHUNK_EDGE:
        for kind in kinds:
            for inplace in (True, False):
                tag = "".join(f"-{k}={v}" for k, v in env.items())
                yield pytest.param(n, s, prec, kind, env, odd, inplace, id=f"n{n}-s{s}-{prec}-{kind}{tag}-{'in-place' if inplace else 'out-of-place'}")


@pytest.mark.parametrize("n,s,prec,kind,env,odd,inplace", list(_chunk_edge_params()))
def test_composed_route_chunk_edges(gpu, n, s, prec, kind, env, odd, inplace, monkeypatch):
    """The chunk loop of dfft::r2r with more than one chunk: the u0 offsets, the ragged last chunk and (s = 1, odd rows) the half-empty
    last row pair.  The plan-less entry point leases exactly r2r_scratch_bytes, so the halving loop for a short scratch has no caller
    ("32-bit guards of the plan-less routes")."""
    import large_extent as LE
    from distributedfft_amd import _lib, api
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    lib, code = _lib.load(), {"f64": api.F64, "f32": api.F32}[prec]
    vec = int(s > 1 and s % 2 == 0)
    assert lib.dfft_r2r_fused_applies(n, s, code, api.R2R_KINDS[kind], vec) == 0
    sp = LE.pair_units(s, 2)[1]
    cu = LE.chunk_units(n, sp, prec, 1 << 40)
    units = LE.ragged_batch(cu)
    batch = 2 * units - 1 if s == 1 else units        # s = 1: units are row pairs, the last one half empty
    assert (batch % 2 == 1) or not odd
    M = lib.dfft_bluestein_length(n)
    bs_fused = bool(M) and bool(lib.dfft_bluestein_fused_applies(n, sp))
    scratch = int(lib.dfft_r2r1d_strided_scratch_bytes(n, s, batch, code, api.R2R_KINDS[kind], vec))
    assert cu > 1 and scratch == LE.chunk_bytes(n, sp, prec, cu, M, bs_fused)   # the library chunks at the mirrored size
    if env.get("DFFT_BLUESTEIN_FUSED") == "0":
        assert LE.bluestein_chunk(M, sp, cu, prec) < cu                        # the inner transform takes its own chunks inside one
    K = LE.pick_k([(batch, n, s, LE.CBYTES[prec] // 2)])
    x, ref = LE.r2r_base(n, K, kind)
    family = "r2r-bluestein" if api.length_kind(n) == 3 else "r2r"
    LE.run_case(gpu, f"r2r {kind} n={n} s={s} batch={batch} ({cu} units per chunk) {'in place' if inplace else 'out of place'}", family, prec, n,
                x, ref, batch, s, lambda t, o: api.r2r(t, kind, dim=1, out=o), inplace, scratch=scratch)
