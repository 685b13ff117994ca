"""-m gpu: the chunk seams of every composed route at small shapes (tests/chunk_seams.py).

Every plan-less route that works through scratch cuts its batch into chunks of at most max(cap, one unit) bytes; the cap is 256 MiB unless
DFFT_SCRATCH_CHUNK_BYTES says otherwise (read once per call).  Each seam runs one small problem with the cap unset -- one chunk -- and
under caps that cut it into three chunks or more (two for the four-pair seams under their two-pair cap), and checks per run
  (a) the result against the family's longdouble reference under the family's existing bound (the op's of tests/call_mix.py);
  (b, c) the chunked result against the one-chunk result, bit for bit, wherever the cut cannot change a bit (below);
  (d) stale reads and the lease: the scratch buffer holds exactly the announced lease, every byte 0xFF (NaN patterns), before the call,
      and has the same capacity afterwards; `out` lies between guard regions that stay intact; no input is written;
  (e) the number of chunks the mirror computes.

Which results are bit-identical to the one-chunk call, and why:
  * rconv1d, rconv1d_os, rconv1d_long (both routes), the paired real rows, the strided real columns, r2r, Bluestein: units are
    independent -- a row, an overlap-save block, a row pair, a batch item is transformed by the same launches on its own scratch
    rows wherever the cut falls.
  * rxspec1d composed (rxspec_mac_kernel) and rxspec1d_long composed (lxspec_mac_kernel): a thread owns one bin of one channel and adds
    the channel's rows of the chunk IN ROW ORDER onto `out` (zero for the first chunk, else what the chunks before left there).  The
    additions of a bin are the same sequence whatever the cut; storing the running sum to memory between two of them changes no bit.
    So: bit equality with the one-chunk call.
  * rxspec1d_long fused: the Mid kernel sums a channel's rows of one chunk (one slice here: fewer than eight rows per channel) into a
    partial sum that starts at zero, and lxspec_reduce_kernel writes (first chunk) or ADDS (later chunks) that partial sum to `out`:
    (r0 + r1 + r2) + (r3 + ...) is another sequence of roundings than the one-chunk call's r0 + r1 + r2 + r3 + ...  The order does depend
    on the cut.  So, as test_gpu_rxspec1d_long.py::test_several_chunks: bit equality with the chunks' own sums (one-chunk calls on the
    rows of each channel in the chunk) added in chunk order.

(h) pins that a plan reads the cap when it is created: created under a two-unit cap and executed with none, and the reverse, an
any-length R2C plan gives the bits of the plan that never saw a cap."""
import numpy as np
import pytest

import call_mix as CM
import chunk_seams as S
import mem_contract as MC
import test_gpu_real_any as RA

pytestmark = pytest.mark.gpu

_DEV = {}
WORST = {}    # family -> (nu / bound, nu, seam) of this process


def _L():
    from distributedfft_amd import _lib
    return _lib


def _lib():
    return _L().load()


def _tdtype(np_dtype):
    import torch
    return {"float32": torch.float32, "float64": torch.float64, "complex64": torch.complex64, "complex128": torch.complex128}[np.dtype(np_dtype).name]


def _dev(op, gpu):
    """The op's inputs on the device (once per op), a copy to compare them with afterwards, their pointers"""
    st = _DEV.get(op.name)
    if st is None:
        import torch
        inputs = {k: torch.from_numpy(np.array(v)).to(gpu) for k, v in op.case[0].items()}
        st = _DEV[op.name] = (inputs, {k: t.clone() for k, t in inputs.items()}, {k: t.data_ptr() for k, t in inputs.items()})
        torch.cuda.synchronize()
    return st


def _wait(stream):
    try:
        stream.synchronize()
    except RuntimeError as e:     # a HIP error is sticky: nothing more is started on this device
        pytest.exit(f"the device reported an error while waiting for a stream, the session ends here: {e}", returncode=3)


def _run(seam, gpu, cap):
    """One call of the seam under `cap` bytes (None: unset) on a stream of its own, from dfft_trim(), on a scratch buffer of exactly the
    announced lease filled with 0xFF.  Checks (a) and (d); -> the output view (a device tensor between its guards)."""
    import torch
    L, lib, op = _L(), _lib(), seam.op
    inputs, keep, ptr = _dev(op, gpu)
    _, shape, dtype, _ = op.case
    count = int(np.prod(shape))
    what = (seam, "no cap" if cap is None else f"cap {cap}")
    with CM.env(dict(seam.switches(cap), **({} if cap is not None else {S.ENV: ""}))):
        need = int(op._need(lib))
        assert need == seam.lease(cap) > 0, (what, need, seam.lease(cap))
        L.check(lib.dfft_trim(), "dfft_trim")
        stream = torch.cuda.Stream(gpu)
        h = stream.cuda_stream
        L.check(lib.dfft_debug_scratch_fill(need, 0xFF, h), "dfft_debug_scratch_fill")
        assert int(lib.dfft_debug_scratch_capacity(h)) == need and int(lib.dfft_debug_scratch_count(0xFF, h)) == need, what
        buf, out = MC.guarded(count, _tdtype(dtype), gpu)
        pointers = dict(ptr)
        if seam.inplace:
            assert inputs["x"].numel() == count and inputs["x"].dtype == out.dtype, what
            out.copy_(inputs["x"].reshape(-1))
            pointers["x"] = out.data_ptr()
        stream.wait_stream(torch.cuda.current_stream())
        rc = op._call(lib, pointers, out.data_ptr(), h)
        if rc == L.EHIP:
            pytest.exit(f"{what}: the HIP runtime reported an error, the session ends here: {lib.dfft_last_error().decode()}", returncode=3)
        assert rc == 0, (what, rc, lib.dfft_last_error().decode())
        _wait(stream)
        assert int(lib.dfft_debug_scratch_capacity(h)) == need, (what, "the call did not run on the lease its query announced")
        assert int(lib.dfft_debug_scratch_count(0xFF, h)) < need, (what, "a leasing call wrote nothing into the buffer")
    assert MC.guards_intact(buf, out, str(what))
    assert all(MC.bits_equal(inputs[k], keep[k]) for k in inputs), (what, "an input was written")
    value = op.measure(out.cpu().numpy().reshape(shape))
    print(f"chunk seam {seam} {what[1]}: nu {value:.3f} (bound {op.bound}: {op.bound_name})")
    if value / op.bound > WORST.get(seam.family, (-1.0,))[0]:
        WORST[seam.family] = (value / op.bound, value, f"{seam} {what[1]}")
        print(f"chunk seam worst so far {seam.family}: nu {value:.3f} of {op.bound} ({seam} {what[1]})")
    assert value <= op.bound, (what, value, op.bound)
    return out


def _chunk_sums(seam, gpu, cap):
    """dfft_rxspec1d_long, fused: per chunk and channel the one-chunk call on the channel's rows of that chunk (channels = 1, no cap),
    a channel without a row in the chunk adding zero, the chunks added in order -- the first is written, the others are added"""
    import torch
    L, lib = _L(), _lib()
    m, n, channels, batch, order, autos = seam.sums
    code = CM.CODE[seam.op.prec]
    inputs, _, _ = _dev(seam.op, gpu)
    x = inputs["x"].reshape(batch * channels, n)
    g = x if autos else inputs["g"].reshape(batch * channels, n)
    total, r0 = None, 0
    with CM.env(dict(seam.op.switches, **{S.ENV: ""})):
        for k in seam.chunks(cap):
            part = torch.zeros(channels, m // 2 + 1, dtype=_tdtype(seam.op.case[2]), device=gpu)
            for c in range(channels):
                rows = [r for r in range(r0, r0 + k) if r % channels == c]
                if not rows:
                    continue
                xs = x[rows].contiguous()
                gs = xs if autos else g[rows].contiguous()
                torch.cuda.synchronize()
                assert lib.dfft_rxspec1d_long_slices(m, 1, len(rows), code) == 1
                L.check(lib.dfft_rxspec1d_long(xs.data_ptr(), gs.data_ptr(), part[c].data_ptr(), n, m, 1, len(rows), code, order, None), "dfft_rxspec1d_long")
                torch.cuda.synchronize()
            total = part if total is None else total + part
            r0 += k
    return total.reshape(-1)


@pytest.mark.parametrize("seam", S.SEAMS, ids=repr)
def test_seam(gpu, seam):
    one = _run(seam, gpu, None)
    assert seam.chunks() == [seam.units]
    for label in seam.caps:
        cap = seam.cap_bytes(label)
        chunks = seam.chunks(cap)
        assert sum(chunks) == seam.units and (len(chunks) >= 3 or (seam.units == 4 and chunks == [2, 2])), (seam, label, chunks)
        got = _run(seam, gpu, cap)
        if seam.exact:
            assert MC.bits_equal(got, one), (seam, label, chunks, "the chunked result differs from the one-chunk result")
        else:
            assert MC.bits_equal(got, _chunk_sums(seam, gpu, cap)), (seam, label, chunks, "differs from the chunks' own sums added in chunk order")


def test_worst_figures_per_family():
    """The worst nu of this process per family, as a share of the family's bound (printed for DESIGN; every run asserted its own)"""
    for family in S.FAMILIES:
        if family in WORST:
            share, value, what = WORST[family]
            print(f"chunk seams worst {family}: nu {value:.3f} = {share:.2f} of its bound ({what})")
            assert share <= 1.0


# ---- (h) plan scratch under a changed cap ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n2, switches", [(375, {}), (1009, {"DFFT_BLUESTEIN_FUSED": 0})], ids=["pairs-375", "bluestein-1009-multi-pass"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_plan_reads_the_cap_when_it_is_created(gpu, n2, switches, prec):
    """An any-length R2C plan on (8, 12, n2) at P = 1, forward and backward: its paired real rows (96 rows, 48 pairs; n2 = 1009 with the
    multi-pass Bluestein inside) size the plan's scratch at creation under the cap read THERE, and every execute cuts by that scratch.
    Created under a two-pair cap and executed with none, created with none and executed under the cap, and created and executed under
    it: all three give the bits of the plan that never saw a cap."""
    import torch
    from distributedfft_amd import api
    N = (8, 12, n2)
    rdt, cdt = (torch.float64, torch.complex128) if prec == "f64" else (torch.float32, torch.complex64)
    rc, cc = api.r2c_counts(*N, 1, 0)
    x = torch.from_numpy(np.random.default_rng(n2).standard_normal(rc)).to(gpu).to(rdt)
    cap = {S.ENV: 2 * n2 * CM.ESIZE[prec]}
    none = {S.ENV: ""}

    def run(at_create, at_execute):
        a, b, c = x.clone(), torch.zeros(cc, dtype=cdt, device=gpu), torch.zeros(rc, dtype=rdt, device=gpu)
        torch.cuda.synchronize()
        out = []
        for src, dst, direction in ((a, b, api.FORWARD), (b, c, api.BACKWARD)):     # (a plan captures its input when it is created)
            with CM.env(dict(switches, **at_create)):
                p = api.PlanR2C(*N, src, dst, None, 0, 1, direction, any_length=True)
            with CM.env(dict(switches, **at_execute)):
                p.execute()
                p.sync()
            p.destroy()
            out.append(dst.clone())
        assert MC.bits_equal(a, x), "the forward plan wrote its input"
        return out

    base = run(none, none)
    got = base[0].cpu().numpy().reshape(N[1], N[2] // 2 + 1, N[0])
    ref = np.fft.rfftn(x.cpu().numpy().astype(np.float64).reshape(N)).transpose(1, 2, 0)
    assert RA._rel(got, ref) < RA.TOL[prec], (N, prec, "the plan that never saw a cap is wrong itself")
    for name, at_create, at_execute in (("created under the cap", cap, none), ("executed under the cap", none, cap), ("both", cap, cap)):
        spectrum, back = run(at_create, at_execute)
        assert MC.bits_equal(spectrum, base[0]), (name, "forward")
        assert MC.bits_equal(back, base[1]), (name, "backward")
