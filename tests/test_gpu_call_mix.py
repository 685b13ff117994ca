"""-m gpu: the plan-less entry points against the state EARLIER calls left behind -- the library's promise of bit-identical results from
call to call, held across history.

All of them share one grow-only scratch buffer per (device, stream) (dfft_long.hip, leased through ScratchLease while a call is being
enqueued), the table caches keyed by device (twiddles, four-step twiddles, Bluestein chirps, r2r quarter waves, the long convolution's
tables; dfft_trim() drops some of them) and routes chosen per call from environment switches.  tests/call_mix.py registers one small op per
entry point and scratch layout; here every op's *baseline* -- its output right after dfft_trim(), within its family's bound of the
longdouble reference and bit-equal to a second solo call -- must come out again, bit for bit,
  (a) when the scratch buffer holds NaN bit patterns (0xFF) or zeros instead of an earlier call's leftovers,
  (b) after every other op, enqueued back to back on one stream with a single wait at the end,
  (c) while the buffer grows call by call, and shrinking leases reuse it behind a long call that is still running,
  (d) with dfft_trim() in the middle, from the same host thread and from a second one,
  (e) from two host threads that share a stream, or race on building the tables from two streams,
  (f) on a second stream that finds the tables another stream has just built.
The C entry points are called directly on a torch stream of the test's own (or the NULL stream); the wrappers of api.py end in a
device-wide wait, behind which none of this can show.  Every comparison is bit-equality (mem_contract.bits_equal) or the family's existing
bound; nothing here sets a tolerance.  Nothing is provoked either: no faults on purpose, no repetition to catch a flake, two threads at most.

Output buffers start as 0xFF bytes (NaN patterns), so a result that was not written differs from its baseline."""
import threading
from types import SimpleNamespace

import numpy as np
import pytest

import accuracy_ref as A
import call_mix as CM
import mem_contract as MC
from test_gpu_call_sequences import _in_threads

pytestmark = pytest.mark.gpu

MIB = 1 << 20
OUT_CAP = 1 << 30          # output bytes of one tour segment
_DEV, _BASE = {}, {}


def _L():
    from distributedfft_amd import _lib
    return _lib


def _lib():
    return _L().load()


def _handle(stream):
    return stream.cuda_stream if stream is not None else 0


def _wait(stream):
    import torch
    try:
        if stream is None:
            torch.cuda.synchronize()
        else:
            stream.synchronize()
    except RuntimeError as e:     # a HIP error is sticky: nothing more is started on this device
        pytest.exit(f"the device reported an error while waiting for a stream, the session ends here: {e}", returncode=3)
    _L().check(_lib().dfft_fft2d_batch_status(_handle(stream) or None), "dfft_fft2d_batch_status")


def _own_stream(gpu):
    """A stream of the test's own that waits for what the current stream has queued (inputs, output fills)"""
    import torch
    s = torch.cuda.Stream(gpu)
    s.wait_stream(torch.cuda.current_stream())
    return s


def _dev(op, gpu):
    """The op's inputs on the device (once), a copy to compare them with afterwards, and their pointers"""
    st = _DEV.get(op.name)
    if st is None:
        import torch
        inputs = {k: torch.from_numpy(np.array(v)).to(gpu) for k, v in op.case[0].items()}
        st = _DEV[op.name] = SimpleNamespace(inputs=inputs, keep={k: t.clone() for k, t in inputs.items()},
                                             ptr={k: t.data_ptr() for k, t in inputs.items()})
        torch.cuda.synchronize()
    return st


def _inputs_intact(op, gpu):
    st = _dev(op, gpu)
    return all(MC.bits_equal(st.inputs[k], st.keep[k]) for k in st.inputs)


def _out(op, gpu):
    """An output buffer of the op's size as bytes, every one 0xFF"""
    import torch
    return torch.full((op.out_bytes(),), 0xFF, dtype=torch.uint8, device=gpu)


def _enqueue(op, gpu, stream, out, as_is=False):
    call = op.call_as_is if as_is else op.call
    rc = call(_lib(), _dev(op, gpu).ptr, out.data_ptr(), _handle(stream))
    if rc == _L().EHIP:           # a HIP error is sticky: nothing more is started on this device
        pytest.exit(f"{op}: the HIP runtime reported an error, the session ends here: {_lib().dfft_last_error().decode()}", returncode=3)
    assert rc == 0, (op, rc, _lib().dfft_last_error().decode())
    return out


def _same(op, a, b):
    """Two output buffers of the op hold the same bits (compared as the op's element type: mem_contract.bits_equal)"""
    import torch
    t = {"float32": torch.float32, "float64": torch.float64, "complex64": torch.complex64, "complex128": torch.complex128}[op.case[2].name]
    return MC.bits_equal(a.view(t), b.view(t))


def _numpy(op, out):
    _, shape, dtype, _ = op.case
    return out.cpu().numpy().view(dtype).reshape(shape)


def _solo(op, gpu, as_is=False):
    """One call on a fresh stream, waited for"""
    out = _out(op, gpu)
    s = _own_stream(gpu)
    _enqueue(op, gpu, s, out, as_is)
    _wait(s)
    return out


def _baseline(op, gpu):
    """The op's output after dfft_trim(): once per op and session"""
    if op.name not in _BASE:
        _dev(op, gpu)
        _L().check(_lib().dfft_trim(), "dfft_trim")
        _BASE[op.name] = _solo(op, gpu)
    return _BASE[op.name]


def _baselines(ops, gpu):
    return {op.name: _baseline(op, gpu) for op in ops}


def _fill(nbytes, byte, h):
    _L().check(_lib().dfft_debug_scratch_fill(nbytes, byte, h or None), "dfft_debug_scratch_fill")


def _capacity(h):
    return int(_lib().dfft_debug_scratch_capacity(h or None))


def _count(byte, h):
    n = int(_lib().dfft_debug_scratch_count(byte, h or None))
    assert n >= 0, (n, _lib().dfft_last_error().decode())
    return n


# ---- the baseline -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", CM.REGISTRY + [CM.long_op("f64")], ids=repr)
def test_baseline_is_within_the_bound_and_bit_stable(gpu, op):
    base = _baseline(op, gpu)
    value = op.measure(_numpy(op, base))
    print(f"call mix {op}: nu {value:.3f} (bound {op.bound}: {op.bound_name})")
    assert value <= op.bound, (op, value, op.bound)
    assert _same(op, _solo(op, gpu), base), (op, "a second solo call differs")
    assert _inputs_intact(op, gpu), (op, "an input was written")


# ---- (a) poisoned scratch -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["own-stream", "null-stream"])
@pytest.mark.parametrize("op", CM.REGISTRY, ids=repr)
def test_poisoned_scratch(gpu, op, where):
    """The buffer holds 0xFF throughout (every fp32 / fp64 word a NaN), then 0x00: the result is the baseline's, bit for bit; the call ran
    on THAT buffer (the capacity did not change) and, if it leases, wrote into it; if it does not, it left every byte alone."""
    base = _baseline(op, gpu)
    stream = _own_stream(gpu) if where == "own-stream" else None
    h, need = _handle(stream), op.need(_lib())
    assert (need > 0) == (op.flag == CM.LEASES)
    for byte in (0xFF, 0x00):
        _fill(max(need, MIB), byte, h)
        cap = _capacity(h)
        assert cap >= max(need, MIB)
        assert _count(byte, h) == cap, (op, byte, "the fill did not reach the whole buffer")
        out = _out(op, gpu)
        if stream is not None:
            import torch
            stream.wait_stream(torch.cuda.current_stream())
        _enqueue(op, gpu, stream, out)
        _wait(stream)
        assert _same(op, out, base), (op, hex(byte), "the result depends on what the scratch buffer held")
        assert _capacity(h) == cap, (op, hex(byte), "the call did not run on the poisoned buffer", need, cap, _capacity(h))
        left = _count(byte, h)
        if op.flag == CM.LEASES:
            assert left < cap, (op, hex(byte), "a leasing call wrote nothing into the buffer")
        else:
            assert left == cap, (op, hex(byte), "a call that leases nothing wrote into the buffer", cap - left)
    assert _inputs_intact(op, gpu), (op, "an input was written")


# ---- (b) every op after every other, with no host wait ------------------------------------------------------------------------------------
def _run_tour(gpu, ops, stream):
    """CM.tour over `ops` on `stream`, every call into a buffer of its own, one wait per segment of at most OUT_CAP output bytes (segments
    overlap by one call, so every ordered pair stays a pair of neighbours inside a segment)"""
    import torch
    base = _baselines(ops, gpu)
    walk = CM.tour(len(ops))
    size = [(op.out_bytes() + 255) // 256 * 256 for op in ops]
    wrong, a = [], 0
    while True:
        b, total = a, 0
        while b < len(walk) and (b < a + 2 or total + size[walk[b]] <= OUT_CAP):
            total += size[walk[b]]
            b += 1
        pool = torch.full((total,), 0xFF, dtype=torch.uint8, device=gpu)
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        outs, off = [], 0
        for i in walk[a:b]:
            outs.append(pool[off:off + ops[i].out_bytes()])
            off += size[i]
            _enqueue(ops[i], gpu, stream, outs[-1])
        _wait(stream)
        for pos, (i, out) in enumerate(zip(walk[a:b], outs)):
            if not _same(ops[i], out, base[ops[i].name]):
                wrong.append((a + pos, ops[walk[a + pos - 1]].name if a + pos else None, ops[i].name))
        del pool, outs
        if b == len(walk):
            break
        a = b - 1
    assert not wrong, (len(wrong), "calls differ from their baselines; (position, the call before, the call):", wrong[:12])
    for op in ops:
        assert _inputs_intact(op, gpu), (op, "an input was written")


def test_tour_fp64(gpu):
    import torch
    _run_tour(gpu, CM.ops("f64"), torch.cuda.Stream(gpu))


def test_tour_fp32_on_the_null_stream(gpu):
    _run_tour(gpu, CM.ops("f32"), None)


def _mixed_ops():
    """Both precisions in turn: per entry point its first leasing op and, where it has one, its first op that leases nothing"""
    out = []
    for entry in CM.ENTRY_POINTS:
        for flag in (CM.LEASES, CM.NO_LEASE):
            for prec in A.PRECS:
                out += [op for op in CM.ops(prec) if op.entry == entry and op.flag == flag][:1]
    return out


def test_tour_of_both_precisions(gpu):
    import torch
    ops = _mixed_ops()
    assert {op.prec for op in ops} == set(A.PRECS) and all(a.prec != b.prec for a, b in zip(ops[0::2], ops[1::2]))
    _run_tour(gpu, ops, torch.cuda.Stream(gpu))


# ---- (c) growth while work is queued ------------------------------------------------------------------------------------------------------
def _growing_ops():
    """Leasing fp64 ops whose leases grow by at least a half from one to the next, and the long op (64 MiB) last"""
    lib, out, last = _lib(), [], 0
    for op in sorted((op for op in CM.ops("f64") if op.flag == CM.LEASES), key=lambda op: (op.need(lib), op.name)):
        if op.need(lib) >= last + last // 2 + 1:
            out.append(op)
            last = op.need(lib)
    long = CM.long_op("f64")
    assert long.need(lib) == 64 * MIB > last and len(out) >= 6
    return out + [long]


def test_growth_while_work_is_queued(gpu):
    """From dfft_trim(), in order of increasing lease on one stream: every call finds the buffer too small and regrows it behind the calls
    queued before it.  The largest lease is the long call's (four-step rows, n = 65536, 64 rows, fp64: 64 MiB), so that one closes the way
    up and opens the way down, where it is still running when the calls behind it are enqueued on the buffer it uses.  One wait at the
    end; the buffer then holds the largest lease."""
    import torch
    lib, order = _lib(), _growing_ops()
    base = _baselines(order, gpu)
    _L().check(lib.dfft_trim(), "dfft_trim")
    up, down = [_out(op, gpu) for op in order], [_out(op, gpu) for op in order]
    stream = _own_stream(gpu)
    h = _handle(stream)
    assert _capacity(h) == 0
    cap = 0
    for op, out in zip(order, up):
        _enqueue(op, gpu, stream, out)
        assert _capacity(h) == op.need(lib) > cap, (op, _capacity(h), op.need(lib), cap)
        cap = _capacity(h)
    for op, out in zip(reversed(order), reversed(down)):
        _enqueue(op, gpu, stream, out)
        assert _capacity(h) == cap, (op, "a smaller lease changed the buffer")
    _wait(stream)
    for op, a, b in zip(order, up, down):
        assert _same(op, a, base[op.name]), (op, "on the way up")
        assert _same(op, b, base[op.name]), (op, "on the way down")
    assert _capacity(h) == max(op.need(lib) for op in order) == 64 * MIB
    del up, down
    _L().check(lib.dfft_trim(), "dfft_trim")     # the 64 MiB go back
    torch.cuda.empty_cache()


# ---- (d) dfft_trim() in the middle --------------------------------------------------------------------------------------------------------
def _trim_ops():
    by = CM.BY_NAME
    return [CM.long_op("f64"), by["any-2053-f64"], by["dct2-97-f64"], by["rconv-64-composed-f64"]]


def test_trim_right_behind_a_long_call(gpu):
    """The long call is enqueued, dfft_trim() follows at once from the host, then a Bluestein op, an r2r op and a leasing op rebuild what
    it dropped: all four results are the baselines taken BEFORE the trim."""
    ops = _trim_ops()
    base = _baselines(ops, gpu)
    outs = [_out(op, gpu) for op in ops]
    stream = _own_stream(gpu)
    _enqueue(ops[0], gpu, stream, outs[0])
    _L().check(_lib().dfft_trim(), "dfft_trim")
    for op, out in zip(ops[1:], outs[1:]):
        _enqueue(op, gpu, stream, out)
    _wait(stream)
    for op, out in zip(ops, outs):
        assert _same(op, out, base[op.name]), (op, "differs after a dfft_trim() in the middle")


def test_trim_from_a_second_thread(gpu):
    """One thread loops over a Bluestein op, an r2r op and a leasing op (none of them behind a switch) on one stream; a second thread
    issues dfft_trim() once the first call has been enqueued."""
    import torch
    by = CM.BY_NAME
    ops = [by["any-2053-f64"], by["dct2-97-f64"], by["lconv-16384-f64"]]
    assert not any(op.switches for op in ops)
    base = _baselines(ops, gpu)
    rounds = 8
    outs = [[_out(op, gpu) for op in ops] for _ in range(rounds)]
    stream = _own_stream(gpu)
    started = threading.Event()

    def work():
        torch.cuda.set_device(gpu)
        for r in range(rounds):
            for op, out in zip(ops, outs[r]):
                _enqueue(op, gpu, stream, out, as_is=True)
                started.set()

    def trim():
        torch.cuda.set_device(gpu)
        assert started.wait(timeout=600)
        _L().check(_lib().dfft_trim(), "dfft_trim")

    _in_threads([work, trim])
    _wait(stream)
    for r in range(rounds):
        for op, out in zip(ops, outs[r]):
            assert _same(op, out, base[op.name]), (op, r, "differs with a dfft_trim() from a second thread")


# ---- (e) host threads ---------------------------------------------------------------------------------------------------------------------
def test_two_threads_on_one_stream(gpu):
    """One thread loops a several-chunk composed rcsd1d and rconv1d, the other a several-chunk composed stft1d / istft1d pair, a composed
    rconv1d_long and a several-chunk composed rconv1d_os and rxspec1d, all on ONE stream: a lease has to cover every launch of its call.  The switches of all four are set once around the
    whole test (host threads must not change the environment under each other) and the solo results are taken under the same switches:
    the composed rcsd1d runs its frames through the composed stft route then."""
    import torch
    by = CM.BY_NAME
    first = [by["rcsd-cross-chunks-f64"], by["rconv-36-chunks-f64"]]
    second = [by["stft-64-chunks-f64"], by["istft-64-chunks-f64"], by["lconv-16384-composed-f64"], by["osconv-36-chunks-f64"],
              by["rxspec-cross-chunks-f64"]]
    switches = {}
    for op in first + second:
        for k, v in op.switches.items():
            assert switches.setdefault(k, v) == v, (op, k)
    lib = _lib()
    with CM.env(switches):
        assert all(op.need(lib) > 0 for op in first + second)
        assert lib.dfft_rcsd1d_fused_applies(128, 0, 0) == 0 == lib.dfft_stft1d_fused_applies(128, 0) == lib.dfft_rconv1d_long_fused_applies(CM.LONG_M, 0)
        solo = {op.name: _solo(op, gpu, as_is=True) for op in first + second}
        for op in first + second:
            assert op.measure(_numpy(op, solo[op.name])) <= op.bound, op
        a_outs = [[_out(op, gpu) for op in first] for _ in range(20)]
        b_outs = [[_out(op, gpu) for op in second] for _ in range(7)]
        stream = _own_stream(gpu)

        def job(ops, outs):
            def run():
                torch.cuda.set_device(gpu)
                for row in outs:
                    for op, out in zip(ops, row):
                        _enqueue(op, gpu, stream, out, as_is=True)
            return run

        _in_threads([job(first, a_outs), job(second, b_outs)])
        _wait(stream)
    for ops, outs in ((first, a_outs), (second, b_outs)):
        for r, row in enumerate(outs):
            for op, out in zip(ops, row):
                assert _same(op, out, solo[op.name]), (op, r, "differs when two host threads share the stream")


def test_two_threads_race_on_building_the_tables(gpu):
    """From dfft_trim(), two threads on two streams both start with the same Bluestein op and the same long convolution: whichever
    builds the tables, both results are the baseline's."""
    import torch
    by = CM.BY_NAME
    ops = [by["any-2053-f64"], by["lconv-16384-f64"], by["dct2-97-f64"]]
    assert not any(op.switches for op in ops)
    base = _baselines(ops, gpu)
    outs = [[_out(op, gpu) for op in ops] for _ in range(2)]
    streams = [_own_stream(gpu), _own_stream(gpu)]
    _L().check(_lib().dfft_trim(), "dfft_trim")
    gate = threading.Barrier(2, timeout=600)

    def job(k):
        def run():
            torch.cuda.set_device(gpu)
            gate.wait()
            for op, out in zip(ops, outs[k]):
                _enqueue(op, gpu, streams[k], out, as_is=True)
        return run

    _in_threads([job(0), job(1)])
    for k in range(2):
        _wait(streams[k])
        for op, out in zip(ops, outs[k]):
            assert _same(op, out, base[op.name]), (op, k, "differs when two threads race on the tables")


# ---- (f) one table set, two streams -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["any-2053", "any-10007", "irfft-1009", "dct2-97", "dst3-375-rows", "lconv-16384", "lxspec-cross-slices",
                                  "rows-8192"])
@pytest.mark.parametrize("prec", A.PRECS)
def test_tables_built_on_one_stream_serve_another(gpu, name, prec):
    """After dfft_trim() the op builds its tables on stream S1; with no wait in between, the same op runs on other inputs (the batch in
    reverse order) on S2.  Both results are what the calls give alone."""
    import torch
    op = CM.BY_NAME[f"{name}-{prec}"]
    assert op.tables and set(op.case[0]) - {"x", "g"} <= {"hp", "h"}
    st = _dev(op, gpu)
    other = dict(st.ptr)
    flipped = {k: torch.flip(st.inputs[k], [0]).contiguous() for k in ("x", "g") if k in st.inputs}
    other.update({k: t.data_ptr() for k, t in flipped.items()})
    lib = _lib()

    def enqueue(ptr, stream, out):
        rc = op.call(lib, ptr, out.data_ptr(), _handle(stream))
        assert rc == 0, (op, rc, lib.dfft_last_error().decode())

    alone = _out(op, gpu)                      # the other inputs, alone
    s0 = _own_stream(gpu)
    enqueue(other, s0, alone)
    _wait(s0)
    base = _baseline(op, gpu)                  # (cached, or a trim and a solo call)
    out1, out2 = _out(op, gpu), _out(op, gpu)
    s1, s2 = _own_stream(gpu), _own_stream(gpu)
    _L().check(lib.dfft_trim(), "dfft_trim")
    enqueue(st.ptr, s1, out1)
    enqueue(other, s2, out2)
    _wait(s1)
    _wait(s2)
    assert _same(op, out1, base), (op, "the stream that built the tables")
    assert _same(op, out2, alone), (op, "the stream that found them")
    assert not _same(op, alone, base), (op, "the other inputs are not other")
