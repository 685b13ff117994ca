"""The buffer contract of the complex entry points, host side (no GPU): the guarded-buffer helper of the GPU tests checked on CPU tensors
(tests/mem_contract.py), the refusal of partly overlapping in / out by dfft_fft1d_rows, dfft_fft1d_cols, dfft_fft1d_any,
dfft_fft2d_batch, dfft_plan_create and dfft_plan_create_conv -- made before the device is queried, so fake addresses do --, and the
admission rule of the fused X stage of the spectral-filter plans for fp32 buffers that are only 8-byte aligned."""
import ctypes as C
from pathlib import Path

import pytest

import mem_contract as M

ROOT = Path(__file__).resolve().parent.parent
A, B = 0x10000000, 0x20000000


# ---- the helper ------------------------------------------------------------------------------------------------------------------------
def _dtypes():
    import torch
    return [(torch.complex64, 8), (torch.complex128, 16), (torch.float32, 4), (torch.float64, 8)]


def test_offset_views_have_the_advertised_misalignment():
    for dtype, size in _dtypes():
        for pitch in (1, 21, 33, 100):
            buf0, v0 = M.guarded(40, dtype, "cpu", 0, pitch)
            buf1, v1 = M.guarded(40, dtype, "cpu", 1, pitch)
            assert v0.data_ptr() % 16 == 0
            assert v1.data_ptr() % 16 == size % 16          # one ELEMENT past a 16-byte boundary (complex128 stays aligned)
            assert (v1.data_ptr() - size) % 16 == 0
            for buf, v in ((buf0, v0), (buf1, v1)):
                g = M.guard_elems(pitch)
                start = M.view_start(buf, v)
                assert v.numel() == 40 and g >= 64 and g >= 2 * pitch
                assert start >= g and buf.numel() - (start + 40) >= g        # guards on both sides
                assert (v.data_ptr() - buf.data_ptr()) == start * size


def test_guards_intact_passes_an_untouched_buffer_and_names_each_spoiled_edge():
    import torch
    for dtype, _ in _dtypes():
        for off in (0, 1):
            buf, v = M.guarded(24, dtype, "cpu", off, 7)
            v.copy_(torch.arange(24).to(dtype))                               # writing the view itself is fine
            assert M.guards_intact(buf, v)
            start = M.view_start(buf, v)
            for rel in (-start, -1, 24, buf.numel() - start - 1):             # first and last element of either guard
                spoiled = buf.clone()
                sv = spoiled[start:start + 24]
                spoiled[start + rel] = 1.0
                with pytest.raises(AssertionError, match=rf"index {rel} relative"):
                    M.guards_intact(spoiled, sv, "case")
            # one bit is enough: the sentinel's neighbour in the last place (an integer view compares, not a float tolerance)
            spoiled = buf.clone()
            M._bits(spoiled)[(start - 3) * M._parts(buf)] += 1
            with pytest.raises(AssertionError, match=r"index -3 relative"):
                M.guards_intact(spoiled, spoiled[start:start + 24])


def test_bits_equal_is_bitwise():
    import torch
    a = torch.zeros(4, dtype=torch.complex64)
    b = a.clone()
    assert M.bits_equal(a, b)
    b[2] = complex(-0.0, 0.0)
    assert bool(torch.equal(a, b)) and not M.bits_equal(a, b)


def test_an_empty_view_keeps_its_place():
    import torch
    buf, v = M.guarded(0, torch.complex64, "cpu", 1, 5)
    assert v.numel() == 0 and M.view_start(buf, v) == M.guard_elems(5) + 1 and M.guards_intact(buf, v)


# ---- overlap refusals through the C ABI ------------------------------------------------------------------------------------------------
def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


def _p(v):
    return C.c_void_p(v) if v else None


def _calls(n=16, s=4, batch=2):
    """name -> (call(in, out, batch, dtype), bytes per batch item in fp64) for a transform of `batch` x n x s elements"""
    lib = _lib()
    return {
        "dfft_fft1d_rows": (lambda i, o, b, dt: lib.dfft_fft1d_rows(_p(i), _p(o), n * s, b, dt, 1, None), n * s * 16),
        "dfft_fft1d_cols": (lambda i, o, b, dt: lib.dfft_fft1d_cols(_p(i), _p(o), n, s, b, dt, 1, None), n * s * 16),
        "dfft_fft1d_any": (lambda i, o, b, dt: lib.dfft_fft1d_any(_p(i), _p(o), n, s, b, dt, -1, None), n * s * 16),
        "dfft_fft1d_any (Bluestein)": (lambda i, o, b, dt: lib.dfft_fft1d_any(_p(i), _p(o), 11, s, b, dt, 1, None), 11 * s * 16),
        "dfft_fft1d_any (rows)": (lambda i, o, b, dt: lib.dfft_fft1d_any(_p(i), _p(o), n, 1, b, dt, 1, None), n * 16),
        "dfft_fft1d_cols (four-step)": (lambda i, o, b, dt: lib.dfft_fft1d_cols(_p(i), _p(o), 8192, s, b, dt, 1, None), 8192 * s * 16),
        "dfft_fft2d_batch": (lambda i, o, b, dt: lib.dfft_fft2d_batch(_p(i), _p(o), n, s, b, dt, 1, None), n * s * 16),
        "dfft_fft2d_batch (four-step axis)": (lambda i, o, b, dt: lib.dfft_fft2d_batch(_p(i), _p(o), 8192, s, b, dt, -1, None), 8192 * s * 16),
    }


def test_partly_overlapping_in_and_out_are_refused():
    from distributedfft_amd import _lib as L
    lib = _lib()
    for name, (call, item) in _calls().items():
        for dt, size in ((L.F64, item), (L.F32, item // 2)):
            total = 2 * size
            for delta in (64, 8 if dt == L.F32 else 16, total - (8 if dt == L.F32 else 16)):     # 64 bytes, one element, all but one element
                assert call(A, A + delta, 2, dt) == L.EINVAL, (name, dt, delta)
                assert "overlap" in lib.dfft_last_error().decode(), name
                assert call(A + delta, A, 2, dt) == L.EINVAL, (name, dt, delta)


def test_in_place_touching_ranges_and_empty_batches_are_accepted():
    """... as far as the device query on a machine without a GPU (with one, fake addresses must not reach a kernel)."""
    from distributedfft_amd import _lib as L
    if _lib().dfft_device_count() > 0:
        return
    for name, (call, item) in _calls().items():
        for dt, size in ((L.F64, item), (L.F32, item // 2)):
            total = 2 * size
            assert call(A, A, 2, dt) == L.ENOGPU, name                      # exactly in place
            assert call(A, A + total, 2, dt) == L.ENOGPU, name              # the ranges merely touch
            assert call(A + total, A, 2, dt) == L.ENOGPU, name
            assert call(A, B, 2, dt) == L.ENOGPU, name
            # batch == 0 transforms nothing: no range to overlap, whatever the pointers
            assert call(A, A + 8, 0, dt) in (L.OK, L.ENOGPU), name
            assert call(A, A, 0, dt) in (L.OK, L.ENOGPU), name


def _plan(inp, out, N=(16, 12, 10), dtype=0, P=1, flags=0):
    h = C.c_void_p()
    rc = _lib().dfft_plan_create(C.byref(h), N[0], N[1], N[2], dtype, 1, _p(inp), _p(out), None, 0, P, flags)
    return rc, _lib().dfft_last_error().decode()


def _conv(inp, out, N=(16, 12, 10), dtype=0):
    h = C.c_void_p()
    rc = _lib().dfft_plan_create_conv(C.byref(h), N[0], N[1], N[2], dtype, _p(inp), _p(out), None, 0, 1, 0)
    return rc, _lib().dfft_last_error().decode()


def test_plans_refuse_partly_overlapping_buffers():
    from distributedfft_amd import _lib as L
    lib = _lib()
    N = (16, 12, 10)
    mc = lib.dfft_max_count(*N, 1, 1)
    for create in (_plan, _conv):
        for dt, size in ((L.F64, 16), (L.F32, 8)):
            total = mc * size
            for delta in (64, size, total - size):
                for i, o in ((A, A + delta), (A + delta, A)):
                    rc, msg = create(i, o, N, dt)
                    assert rc == L.EINVAL and "overlap" in msg, (create.__name__, dt, delta, msg)
            if lib.dfft_device_count() > 0:
                continue
            for i, o in ((A, A), (A, 0), (A, A + total), (A + total, A), (A, B)):   # in place (out == in or NULL), touching, apart
                assert create(i, o, N, dt)[0] == L.ENOGPU, (create.__name__, dt, i, o)
    # the other argument checks keep their order: a bad size is reported as such, not as an overlap
    rc, msg = _plan(A, A + 64, (0, 12, 10))
    assert rc == L.EINVAL and "overlap" not in msg


# ---- the fused X stage of the spectral-filter plans ------------------------------------------------------------------------------------
def test_fused_x_stage_refuses_fp32_buffers_that_are_only_8_byte_aligned():
    """dfft_conv_fused_applies: the one-kernel X stage moves fp32 column PAIRS (16 bytes): P = 1 plans in the natural layout store
    straight into the caller's `out`, so an `out` one element past a 16-byte boundary must send the plan to the three-launch stage, whose
    column launches fall back per base.  fp64 elements are 16 bytes: element alignment is all it needs."""
    from distributedfft_amd import _lib as L
    lib = _lib()

    def applies(dt, i, o, n0=64, rows=8, ncols=16, plane=128, pitch=16, rot=0):
        return lib.dfft_conv_fused_applies(dt, n0, rows, ncols, plane, pitch, rot, _p(i), _p(o))

    assert applies(L.F32, A, B) == 1 and applies(L.F64, A, B) == 1
    assert applies(L.F32, A, A) == 1
    assert applies(L.F32, A, B + 8) == 0                 # out one complex64 past the boundary
    assert applies(L.F32, A + 8, B) == 0                 # in
    assert applies(L.F32, A + 8, A + 8) == 0
    assert applies(L.F64, A + 16, B + 16) == 1           # one complex128 past: still aligned
    assert applies(L.F32, A, B, n0=128, rows=6, ncols=8, plane=48, pitch=8) == 1
    assert applies(L.F32, A, B + 8, n0=128, rows=6, ncols=8, plane=48, pitch=8) == 0
    # the rules it had before hold unchanged
    assert applies(L.F32, A, B, ncols=15, plane=120, pitch=15) == 0    # odd columns: no pairs
    assert applies(L.F64, A, B, ncols=15, plane=120, pitch=15) == 1
    assert applies(L.F64, A, B, n0=60) == 0                            # not a fused length
    assert applies(7, A, B) == 0


def test_the_header_states_the_contract_and_declares_the_query():
    from distributedfft_amd import _lib as L
    text = (ROOT / "include" / "dfft.h").read_text()
    assert "dfft_conv_fused_applies" in L.SIGNATURES and "int dfft_conv_fused_applies(" in text
    flat = " ".join(text.replace("*", " ").split())
    for phrase in ("any element-aligned pointers", "byte ranges that overlap only partly: DFFT_EINVAL", "`in` is never written",
                   "nothing outside"):
        assert flat.count(phrase) >= 2, phrase
