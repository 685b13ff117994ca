"""Batched short-time Fourier transform and its inverse (dfft_stft1d / dfft_istft1d, api.stft / api.istft) on the GPU, against the
longdouble references of tests/stft_cases.py: both precisions, both pad modes and both output kinds over a table that sweeps one factor
at a time (half length, hop, pad, row length, window), item counts that make a workgroup loop, every fused case once more on the composed
route (DFFT_STFT_FUSED=0), the inverse against the longdouble overlap-add and split into chunks, the round trip, the buffer contract on
guarded buffers, a call sequence with dfft_trim in it, and api.stft / api.istft against torch on the CPU.

Error measure: accuracy_ref.nu per frame (forward) or per row (inverse) with n_eff = m.  The cap is accuracy_ref.CEILING["real"], the
project's cap for real transforms -- a condition, not a fitted bound.  It holds for complex bins and for the inverse, against the
longdouble references, between the fused and the composed route, and against torch on the CPU alike; the power spectrogram, whose error
is relative to |X|^2, takes twice the cap in each of these comparisons, and so does the round trip (two transforms).  Every test prints
its nu, and the module prints the worst per route when its last test has run.
Worst nu measured on an MI355X (fp64 / fp32; the cap is 3.6 / 3.2):
    complex bins, fused 0.475 (M = 25, hop 12) / 0.633 (M = 2), composed 0.495 / 0.517 (M = 18, hop 5)
    power, fused 0.900 (M = 64, hop 1) / 1.335 (M = 2), composed 0.901 / 0.897            (cap x 2)
    fused against composed 0.603 / 1.549 (both on power spectrograms, M = 8 / M = 2)      (cap; power: cap x 2)
    inverse 0.706 / 0.883 (M = 25, hop 12)
    round trip 0.597 (n_fft = 36) / 0.387 (n_fft = 128)                                   (cap x 2)
    against torch on the CPU 1.592 / 1.058 (both on power spectrograms)                   (cap; power: cap x 2)

The per-length sweep -- every tuned length of this family, both precisions, every kernel variant -- lives in tests/test_gpu_tuned_sweep.py."""
import ctypes as C
import os

import numpy as np
import pytest

import accuracy_ref as A
import mem_contract as MC
import stft_cases as SC

pytestmark = pytest.mark.gpu

CAP = A.CEILING["real"]
CODE = {"f64": 0, "f32": 1}
WORST = {}


def _rdt(prec):
    import torch
    return torch.float64 if prec == "f64" else torch.float32


def _cdt(prec):
    import torch
    return torch.complex128 if prec == "f64" else torch.complex64


def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


def _vp(t):
    return C.c_void_p(t.data_ptr())


def _stft_raw(x, out, win, n, m, hop, pad, frames, rows, prec, mode, kind, scale=1.0, stream=None):
    from distributedfft_amd import _lib as L
    L.check(_lib().dfft_stft1d(_vp(x), _vp(out), _vp(win), n, m, hop, pad, frames, rows, CODE[prec], SC.MODE_CODE[mode], SC.KIND_CODE[kind], scale,
                               C.c_void_p(stream) if stream else None), "dfft_stft1d")


def _istft_raw(X, out, win, inv_env, n, m, hop, pad, frames, rows, prec, stream=None):
    from distributedfft_amd import _lib as L
    L.check(_lib().dfft_istft1d(_vp(X), _vp(out), _vp(win), _vp(inv_env), n, m, hop, pad, frames, rows, CODE[prec],
                                C.c_void_p(stream) if stream else None), "dfft_istft1d")


class _env:
    """An environment variable the library reads per call, set for the calls inside"""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.old


def _composed():
    return _env("DFFT_STFT_FUSED", "0")


@pytest.fixture(scope="module", autouse=True)
def _print_the_worst_nu_per_route():
    """After the module's last test, whatever the order: the record DESIGN 7n quotes"""
    yield
    for (route, prec), (value, what) in sorted(WORST.items()):
        print(f"stft worst nu {route} {prec}: {value:.3f}  ({what})")


def _check(value, prec, route, what, factor=1.0):
    print(f"stft {prec} {route} {what}: nu {value:.3f}")
    if value > WORST.get((route, prec), (-1.0, ""))[0]:
        WORST[(route, prec)] = (value, what)
    assert value <= factor * CAP[prec], (prec, route, what, value, factor * CAP[prec])


def _forward(gpu, case, prec, mode, kind, fused_on=True):
    """One call through the C ABI -> (numpy result [rows][frames][M + 1], reference of that kind)"""
    import torch
    M, hop, pad, n, wkind = case
    m = 2 * M
    x, win, frames, ref = SC.forward_case(M, hop, pad, n, wkind, mode)
    rows = x.shape[0]
    xt = torch.from_numpy(x).to(_rdt(prec)).to(gpu)
    wt = torch.from_numpy(win).to(_rdt(prec)).to(gpu)
    out = torch.empty((rows, frames, M + 1), dtype=_rdt(prec) if kind == "power" else _cdt(prec), device=gpu)
    keep = xt.clone()
    if fused_on:
        _stft_raw(xt, out, wt, n, m, hop, pad, frames, rows, prec, mode, kind)
    else:
        with _composed():
            assert _lib().dfft_stft1d_fused_applies(m, CODE[prec]) == 0
            _stft_raw(xt, out, wt, n, m, hop, pad, frames, rows, prec, mode, kind)
    torch.cuda.synchronize()
    assert torch.equal(xt, keep), "in was written"
    return out.cpu().numpy(), (SC.power(ref) if kind == "power" else ref)


# ---- the table --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("case", SC.FORWARD, ids=lambda c: "M{}-hop{}-pad{}-n{}-{}".format(*c))
def test_forward_against_the_longdouble_reference(gpu, case, prec):
    """Both pad modes and both output kinds of the case against the reference, and every fused case once more on the composed route:
    within the cap, and the two routes agree with each other to the same bound."""
    M = case[0]
    m = 2 * M
    fused = SC.fused(M, prec)
    assert _lib().dfft_stft1d_fused_applies(m, CODE[prec]) == int(fused)
    for mode in SC.MODES:
        if not SC.usable(case, mode):
            continue
        for kind in SC.KINDS:
            f = 2.0 if kind == "power" else 1.0
            what = "M={} hop={} pad={} n={} {} {} {}".format(*case, mode, kind)
            got, ref = _forward(gpu, case, prec, mode, kind)
            _check(SC.nu_frames(got, ref, m, prec), prec, ("fused " if fused else "composed ") + kind, what, f)
            if fused:
                comp, _ = _forward(gpu, case, prec, mode, kind, fused_on=False)
                _check(SC.nu_frames(comp, ref, m, prec), prec, "composed " + kind, what, f)
                _check(SC.nu_frames(got, comp.astype(A.CLD if kind == "complex" else A.LD), m, prec), prec, "fused against composed", what, f)


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("case", sorted(SC.LOOP), ids=lambda c: "M{}".format(c[0]))
def test_more_items_than_the_grid_holds(gpu, case, prec):
    """The rows of the case repeated along the batch: more items than resident workgroups x G, so a workgroup takes several item groups
    (and the last one is ragged).  Equal rows give equal results; the reference is the small case's."""
    import torch
    M, hop, pad, n, wkind = case
    m, reps = 2 * M, SC.LOOP[case]
    x, win, frames, ref = SC.forward_case(M, hop, pad, n, wkind, "reflect")
    rows = x.shape[0]
    xt = torch.from_numpy(x).to(_rdt(prec)).to(gpu).repeat(reps, 1).contiguous()
    wt = torch.from_numpy(win).to(_rdt(prec)).to(gpu)
    out = torch.empty((reps, rows, frames, M + 1), dtype=_cdt(prec), device=gpu)
    assert _lib().dfft_stft1d_fused_applies(m, CODE[prec]) == 1
    _stft_raw(xt, out, wt, n, m, hop, pad, frames, reps * rows, prec, "reflect", "complex")
    torch.cuda.synchronize()
    assert bool((torch.view_as_real(out) == torch.view_as_real(out[0])).all()), "equal rows gave different results"
    _check(SC.nu_frames(out[0].cpu().numpy(), ref, m, prec), prec, "fused complex", f"M={M} hop={hop} n={n} rows={reps * rows} looping")


def test_normalized_scale_and_fewer_frames(gpu):
    """scale multiplies the bins (its square the power); a call may ask for fewer frames than the rows give"""
    import torch
    M, hop, pad, n, wkind = 64, 32, 64, 386, "hann"
    x, win, frames, ref = SC.forward_case(M, hop, pad, n, wkind, "zero")
    xt, wt = torch.from_numpy(x).to(gpu), torch.from_numpy(win).to(gpu)
    s = 128 ** -0.5
    for fused_on in (True, False):
        for kind in SC.KINDS:
            out = torch.full((3, frames - 2, M + 1), float("nan"), dtype=torch.float64 if kind == "power" else torch.complex128, device=gpu)
            with _env("DFFT_STFT_FUSED", "1" if fused_on else "0"):
                _stft_raw(xt, out, wt, n, 2 * M, hop, pad, frames - 2, 3, "f64", "zero", kind, scale=s)
            torch.cuda.synchronize()
            want = ref[:, :frames - 2] * A.LD(s)
            _check(SC.nu_frames(out.cpu().numpy(), SC.power(want) if kind == "power" else want, 2 * M, "f64"), "f64",
                   ("fused " if fused_on else "composed ") + kind, "scaled, two frames fewer", 2.0 if kind == "power" else 1.0)


# ---- the inverse ------------------------------------------------------------------------------------------------------------------------
def _inverse(gpu, case, prec):
    import torch
    M, hop, pad, frames, wkind = case
    X, win, inv_env, n, ref = SC.inverse_case(M, hop, pad, frames, wkind)
    Xt = torch.from_numpy(X).to(_cdt(prec)).to(gpu)
    wt = torch.from_numpy(win).to(_rdt(prec)).to(gpu)
    et = torch.from_numpy(inv_env).to(_rdt(prec)).to(gpu)
    out = torch.full((X.shape[0], n), float("nan"), dtype=_rdt(prec), device=gpu)
    keep = Xt.clone()
    _istft_raw(Xt, out, wt, et, n, 2 * M, hop, pad, frames, X.shape[0], prec)
    torch.cuda.synchronize()
    assert MC.bits_equal(Xt, keep), "in was written"
    return out, ref


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("case", SC.INVERSE, ids=lambda c: "M{}-hop{}-pad{}-f{}-{}".format(*c))
def test_inverse_against_the_longdouble_overlap_add(gpu, case, prec):
    out, ref = _inverse(gpu, case, prec)
    _check(SC.nu_rows(out.cpu().numpy(), ref, 2 * case[0], prec), prec, "inverse", "M={} hop={} pad={} frames={} {}".format(*case))


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("case", [(64, 32, 64, 9, "hann"), (64, 37, 0, 9, "rect"), (18, 7, 0, 11, "rect"), (64, 128, 0, 9, "hann")],
                         ids=lambda c: "M{}-hop{}-pad{}".format(*c[:3]))
def test_chunks_do_not_change_the_result(gpu, case, prec):
    """DFFT_STFT_CHUNK_BYTES caps a chunk's scratch: rows cut into several chunks of frames (the cap holds fewer frames than a row has,
    but at least the ceil(m / hop) one sample sums), chunks of one or two whole rows, and the forward composed route in chunks of a few
    items -- each bit for bit what the uncapped call gives, since every sample sums the same frames in the same order."""
    import torch
    M, hop, pad, frames, wkind = case
    m, rs = 2 * M, 8 if prec == "f64" else 4
    whole, ref = _inverse(gpu, case, prec)
    _check(SC.nu_rows(whole.cpu().numpy(), ref, m, prec), prec, "inverse", "M={} hop={} pad={} frames={} {}".format(*case))
    ib = m * rs + (0 if M == 64 else (M + 1) * 2 * rs)
    per = -(-m // hop)
    for items in (max(per, 2), per + 3, frames, 2 * frames + 1):
        with _env("DFFT_STFT_CHUNK_BYTES", str(items * ib)):
            assert _lib().dfft_istft1d_scratch_bytes(m, frames, 3, CODE[prec]) == min(3 * frames, items) * ib
            cut, _ = _inverse(gpu, case, prec)
        assert MC.bits_equal(cut, whole), (case, prec, items)
    with _composed():
        for kind in SC.KINDS:
            a, _ = _forward(gpu, (M, hop, pad, 386, wkind), prec, "zero", kind, fused_on=False)
            with _env("DFFT_STFT_CHUNK_BYTES", str(5 * (m * rs + (M + 1) * 2 * rs))):
                b, _ = _forward(gpu, (M, hop, pad, 386, wkind), prec, "zero", kind, fused_on=False)
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (case, prec, kind)


def test_nola_failure_raises(gpu):
    import torch
    from distributedfft_amd import api
    X = torch.ones((2, 65, 9), dtype=torch.complex128, device=gpu)
    with pytest.raises(ValueError):
        api.istft(X, 128, 32, torch.hann_window(128, dtype=torch.float64, device=gpu), center=False)   # the window starts at zero
    with pytest.raises(ValueError):
        api.istft(X, 128, 200, None, center=False)                                                   # gaps between the frames
    assert api.istft(X, 128, 32, torch.hann_window(128, dtype=torch.float64, device=gpu)).shape == (2, 256)
    with pytest.raises(ValueError):
        api.stft(torch.ones((2, 300), device=gpu), 128, pad_mode="replicate")
    with pytest.raises(ValueError):
        api.stft(torch.ones((2, 300), device=gpu), 128, power=1)
    with pytest.raises(ValueError):
        api.stft(torch.ones((2, 30), device=gpu), 128)                                               # reflect needs n_fft // 2 < n


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("n_fft", [128, 36, 1024])
def test_round_trip(gpu, n_fft, prec):
    """istft(stft(x)) == x for center=True, Hann, hop = n_fft / 4, within twice the cap (two transforms)"""
    import torch
    from distributedfft_amd import api
    n = 5 * n_fft + 6
    x = A.rand_real((3, n), 35000 + n_fft)
    xt = torch.from_numpy(x).to(_rdt(prec)).to(gpu)
    w = torch.hann_window(n_fft, dtype=_rdt(prec), device=gpu)
    X = api.stft(xt, n_fft, window=w)
    assert X.shape == (3, n_fft // 2 + 1, 1 + n // (n_fft // 4)) and X.dtype == _cdt(prec)
    y = api.istft(X, n_fft, window=w, length=n)
    assert y.shape == xt.shape and y.dtype == xt.dtype
    _check(SC.nu_rows(y.cpu().numpy(), x.astype(A.LD), n_fft, prec), prec, "round trip", f"n_fft={n_fft} n={n}", 2.0)


# ---- api.stft / api.istft against torch on the CPU -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", A.PRECS)
def test_api_against_torch_on_the_cpu(gpu, prec):
    """torch.stft / torch.istft in float64 on the CPU copy of the input, held to the same bounds as the longdouble references: the cap,
    and twice the cap for the power spectrogram."""
    import torch
    from distributedfft_amd import api
    rdt = _rdt(prec)
    x = torch.from_numpy(A.rand_real((2, 3, 700), 36000)).to(rdt).to(gpu)
    for n_fft, hop, wl, center, mode, norm in ((128, None, None, True, "reflect", False), (128, 32, 100, True, "constant", True),
                                               (36, 10, None, False, "reflect", False), (256, 64, 256, True, "reflect", True)):
        w = None if wl is None else (torch.hann_window(wl, dtype=rdt, device=gpu) + 0.1)
        wc = None if w is None else w.cpu().double()
        kw = dict(hop_length=hop, win_length=wl, center=center, pad_mode=mode, normalized=norm)
        want = torch.stft(x.cpu().double().reshape(6, 700), n_fft, window=wc, onesided=True, return_complex=True, **kw)   # torch takes two axes
        want = want.reshape(2, 3, *want.shape[1:])
        got = api.stft(x, n_fft, window=w, **kw)
        assert got.shape == want.shape and got.dtype == _cdt(prec) and got.transpose(-1, -2).is_contiguous()
        what = f"n_fft={n_fft} hop={hop} win_length={wl} center={center} {mode} normalized={norm}"
        g = got.transpose(-1, -2).cpu().numpy()
        r = want.transpose(-1, -2).numpy().astype(A.CLD)
        _check(SC.nu_frames(g, r, n_fft, prec), prec, "against torch", "stft " + what)
        flat = api.stft(x, n_fft, window=w, frames_last=False, **kw)
        assert MC.bits_equal(flat, got.transpose(-1, -2))
        pw = api.stft(x, n_fft, window=w, power=2, **kw)
        assert pw.dtype == rdt and pw.shape == want.shape
        _check(SC.nu_frames(pw.transpose(-1, -2).cpu().numpy(), SC.power(r), n_fft, prec), prec, "against torch", "power " + what, 2.0)
        kwi = dict(hop_length=hop, win_length=wl, center=center, normalized=norm)
        for length in (None, 650):
            back = torch.istft(want.reshape(6, *want.shape[2:]), n_fft, window=wc, length=length, **kwi).reshape(2, 3, -1)
            mine = api.istft(want.to(_cdt(prec)).to(gpu), n_fft, window=w, length=length, **kwi)
            assert mine.shape == back.shape and mine.dtype == rdt
            _check(SC.nu_rows(mine.cpu().numpy(), back.numpy().astype(A.LD), n_fft, prec), prec, "against torch", f"istft length={length} " + what)


# ---- the buffer contract ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["fused", "composed"])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("prec", A.PRECS)
def test_buffer_contract(gpu, prec, offset, route):
    """in, out, win and inv_env in guarded buffers, on a 16-byte boundary (n, hop, pad even: whole frames load two reals per access) and
    one element past it (per-real loads), the input's guards filled with NaN: nothing outside out is written, the inputs are untouched,
    no NaN reaches the result and the result is right -- forward on the frame kernel and on the composed route (DFFT_STFT_FUSED=0, and an
    untuned length), inverse on a tuned and an untuned length."""
    import torch
    lib = _lib()
    rdt, cdt = _rdt(prec), _cdt(prec)

    def nan_guards(buf, view):
        start = MC.view_start(buf, view)
        buf[:start] = float("nan")
        buf[start + view.numel():] = float("nan")

    for M, hop, pad, n in ((64, 32, 64, 386), (64, 32, 64, 385), (64, 31, 0, 386), (8, 4, 8, 100), (18, 5, 3, 77)):
        m = 2 * M
        for mode in SC.MODES:
            x, win, frames, ref = SC.forward_case(M, hop, pad, n, "hann", mode)
            rows = x.shape[0]
            for kind in SC.KINDS:
                xb, xv = MC.guarded(rows * n, rdt, gpu, offset, n)
                wb, wv = MC.guarded(m, rdt, gpu, offset, m)
                ob, ov = MC.guarded(rows * frames * (M + 1), rdt if kind == "power" else cdt, gpu, offset, M + 1)
                xv.copy_(torch.from_numpy(x).to(rdt).reshape(-1))
                wv.copy_(torch.from_numpy(win).to(rdt))
                nan_guards(xb, xv)
                nan_guards(wb, wv)
                xkeep, wkeep = xb.clone(), wb.clone()
                what = f"M={M} hop={hop} pad={pad} n={n} {mode} {kind} offset={offset} {route}"
                with _env("DFFT_STFT_FUSED", "0" if route == "composed" else "1"):
                    assert lib.dfft_stft1d_fused_applies(m, CODE[prec]) == int(route == "fused" and M != 18)
                    _stft_raw(xv, ov, wv, n, m, hop, pad, frames, rows, prec, mode, kind)
                torch.cuda.synchronize()
                MC.guards_intact(ob, ov, what + " out")
                assert MC.bits_equal(xb, xkeep), what + ": in (or its guards) was written"
                assert MC.bits_equal(wb, wkeep), what + ": win (or its guards) was written"
                got = (torch.view_as_real(ov) if kind == "complex" else ov)
                assert not bool(torch.isnan(got).any()), what + ": a read outside the rows reached the result"
                g = ov.cpu().numpy().reshape(rows, frames, M + 1)
                _check(SC.nu_frames(g, SC.power(ref) if kind == "power" else ref, m, prec), prec,
                       ("fused " if route == "fused" and M != 18 else "composed ") + kind, what, 2.0 if kind == "power" else 1.0)
    if route == "composed":
        return
    for case in ((64, 32, 64, 9, "hann"), (64, 37, 0, 9, "rect"), (18, 7, 0, 11, "rect")):
        M, hop, pad, frames, wkind = case
        m = 2 * M
        X, win, inv_env, n, ref = SC.inverse_case(*case)
        rows = X.shape[0]
        Xb, Xv = MC.guarded(rows * frames * (M + 1), cdt, gpu, offset, M + 1)
        wb, wv = MC.guarded(m, rdt, gpu, offset, m)
        eb, ev = MC.guarded(n, rdt, gpu, offset, n)
        ob, ov = MC.guarded(rows * n, rdt, gpu, offset, n)
        Xv.copy_(torch.from_numpy(X).to(cdt).reshape(-1))
        wv.copy_(torch.from_numpy(win).to(rdt))
        ev.copy_(torch.from_numpy(inv_env).to(rdt))
        for b, v in ((wb, wv), (eb, ev)):
            nan_guards(b, v)
        keeps = [(b, b.clone()) for b in (Xb, wb, eb)]
        what = "inverse M={} hop={} pad={} frames={} {} offset={}".format(*case, offset)
        _istft_raw(Xv, ov, wv, ev, n, m, hop, pad, frames, rows, prec)
        torch.cuda.synchronize()
        MC.guards_intact(ob, ov, what + " out")
        for b, k in keeps:
            assert MC.bits_equal(b, k), what + ": an input (or its guards) was written"
        assert not bool(torch.isnan(ov).any()), what
        _check(SC.nu_rows(ov.cpu().numpy().reshape(rows, n), ref, m, prec), prec, "inverse", what)


# ---- a call sequence --------------------------------------------------------------------------------------------------------------------
def test_call_sequence_with_trim(gpu):
    """Forward and inverse calls on one stream with m, hop, precision, kind and route changing between them, dfft_trim, and one more
    call of each direction on the composed routes (whose scratch the trim freed): every result is right."""
    import torch
    lib = _lib()
    st = torch.cuda.Stream(gpu)
    # forward: (M, hop, pad, n, window), mode, kind, prec, composed by the switch; inverse: (M, hop, pad, frames, window), prec
    seq = [("f", (64, 32, 64, 386, "hann"), "reflect", "complex", "f64", False), ("i", (64, 32, 64, 9, "hann"), "f64"),
           ("f", (18, 5, 3, 77, "rect"), "zero", "power", "f32", False), ("f", (512, 256, 512, 3074, "hann"), "reflect", "power", "f32", False),
           ("i", (18, 7, 0, 11, "rect"), "f32"), ("f", (64, 7, 64, 386, "hann"), "zero", "complex", "f64", True), ("f", (8, 4, 8, 9, "rect"), "reflect", "complex", "f32", False)]
    last = [("f", (18, 9, 18, 110, "hann"), "reflect", "complex", "f64", False), ("i", (64, 64, 0, 9, "hann"), "f32")]

    def enqueue(step):
        if step[0] == "f":
            _, case, mode, kind, prec, off = step
            M, hop, pad, n, wkind = case
            x, win, frames, ref = SC.forward_case(M, hop, pad, n, wkind, mode)
            xt = torch.from_numpy(x).to(_rdt(prec)).to(gpu)
            wt = torch.from_numpy(win).to(_rdt(prec)).to(gpu)
            o = torch.empty((x.shape[0], frames, M + 1), dtype=_rdt(prec) if kind == "power" else _cdt(prec), device=gpu)
            st.wait_stream(torch.cuda.current_stream(gpu))
            with _env("DFFT_STFT_FUSED", "0" if off else "1"):
                assert lib.dfft_stft1d_fused_applies(2 * M, CODE[prec]) == int(SC.fused(M, prec) and not off)
                _stft_raw(xt, o, wt, n, 2 * M, hop, pad, frames, x.shape[0], prec, mode, kind, stream=st.cuda_stream)
            route = ("fused " if SC.fused(M, prec) and not off else "composed ") + kind
            return (xt, wt), o, (SC.power(ref) if kind == "power" else ref), 2 * M, prec, route, f"sequence {case} {mode}", 2.0 if kind == "power" else 1.0
        _, case, prec = step
        M, hop, pad, frames, wkind = case
        X, win, inv_env, n, ref = SC.inverse_case(*case)
        ts = [torch.from_numpy(np.ascontiguousarray(a)).to(d).to(gpu) for a, d in ((X, _cdt(prec)), (win, _rdt(prec)), (inv_env, _rdt(prec)))]
        o = torch.empty((X.shape[0], n), dtype=_rdt(prec), device=gpu)
        st.wait_stream(torch.cuda.current_stream(gpu))
        _istft_raw(ts[0], o, ts[1], ts[2], n, 2 * M, hop, pad, frames, X.shape[0], prec, stream=st.cuda_stream)
        return ts, o, ref, 2 * M, prec, "inverse", f"sequence {case}", 1.0

    runs = [enqueue(s) for s in seq]
    st.synchronize()
    for _, o, ref, m, prec, route, what, f in runs:
        _check(A.nu(o.cpu().numpy(), ref, m, prec, (-1,)), prec, route, what, f)
    assert lib.dfft_trim() == 0
    runs = [enqueue(s) for s in last]
    st.synchronize()
    for _, o, ref, m, prec, route, what, f in runs:
        _check(A.nu(o.cpu().numpy(), ref, m, prec, (-1,)), prec, route, what + " after dfft_trim", f)
