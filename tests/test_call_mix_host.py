"""The registry of tests/call_mix.py, checked without a GPU: every op's lease flag against the entry point's own scratch query, the
registry against _lib.SIGNATURES, the tour against all ordered pairs, every reference against a same-precision CPU model under the op's
bound (so the reference alone does not eat the margin the GPU test relies on), and the three test hooks where there is no device."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import accuracy_ref as A
import call_mix as CM

ROOT = Path(__file__).resolve().parent.parent
HOOKS = ("dfft_debug_scratch_fill", "dfft_debug_scratch_capacity", "dfft_debug_scratch_count")
QUERIES = ("dfft_rfft1d_scratch_bytes", "dfft_rfft2d_batch_scratch_bytes", "dfft_fft2d_batch_scratch_bytes")


def _lib():
    from distributedfft_amd import _lib as L
    return L.load()


# ---- lease flags --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", CM.REGISTRY, ids=repr)
def test_lease_flag_matches_the_scratch_query(op):
    need = op.need(_lib())
    assert op.flag in (CM.LEASES, CM.NO_LEASE)
    if op.flag == CM.LEASES:
        assert 0 < need <= CM.MEMORY_CAP, (op, need)
    else:
        assert need == 0, (op, need)
    assert op.out_bytes() <= CM.MEMORY_CAP


def test_every_entry_point_that_can_lease_has_a_leasing_op():
    for entry in CM.ENTRY_POINTS:
        mine = [op for op in CM.REGISTRY if op.entry == entry]
        assert mine, entry
        for prec in A.PRECS:
            assert any(op.flag == CM.LEASES and op.prec == prec for op in mine), (entry, prec)
    assert {op.entry for op in CM.REGISTRY} == set(CM.ENTRY_POINTS)


def test_routes_are_the_ones_the_names_claim():
    """The route queries under each op's switches: fused where the op says one launch, composed where it says so, several slices and
    several chunks where it says so."""
    lib = _lib()
    by = CM.BY_NAME
    for prec in A.PRECS:
        code = CM.CODE[prec]
        assert lib.dfft_bluestein_fused_applies(97, 3) == 1 and lib.dfft_bluestein_fused_applies(2053, 1) == 0
        assert lib.dfft_length_kind(8192) == 2 and lib.dfft_length_kind(10007) == 3 and lib.dfft_length_kind(375) == 1
        assert lib.dfft_real_form(512) == 1 and lib.dfft_real_form(72) == 1 and lib.dfft_real_form(243) != 1 and lib.dfft_real_form(CM.LONG_M) != 1
        assert lib.dfft_rfft_cols_fused_applies(243, 6, code) == 1 and lib.dfft_rfft_cols_fused_applies(375, 7, code) == 0
        for kind in range(4):
            assert lib.dfft_r2r_fused_applies(243, 6, code, kind, 1) == 1
            with CM.env({"DFFT_R2R_FUSED": 0}):
                assert lib.dfft_r2r_fused_applies(243, 6, code, kind, 1) == 0
        for name, query in (("rconv-64", lambda: lib.dfft_rconv1d_fused_applies(128, 128, code, 0, 1)),
                            ("osconv-64", lambda: lib.dfft_rconv1d_os_fused_applies(128, code)),
                            ("stft-64", lambda: lib.dfft_stft1d_fused_applies(128, code)),
                            ("rcsd-cross-slices", lambda: lib.dfft_rcsd1d_fused_applies(128, code, 0)),
                            ("rcsd-auto-slices", lambda: lib.dfft_rcsd1d_fused_applies(128, code, 1)),
                            ("rxspec-cross-slices", lambda: lib.dfft_rxspec1d_fused_applies(63, 128, code, 0)),
                            ("lxspec-cross-slices", lambda: lib.dfft_rxspec1d_long_fused_applies(CM.LONG_M, code)),
                            ("lconv-16384", lambda: lib.dfft_rconv1d_long_fused_applies(CM.LONG_M, code))):
            assert query() == 1, (name, prec)
            composed = by[f"{name.replace('-slices', '')}-composed-{prec}"] if name != "lconv-16384" else by[f"lconv-16384-composed-{prec}"]
            assert composed.switches
            with CM.env(composed.switches):
                assert query() == 0, (composed, prec)
        assert lib.dfft_rconv1d_fused_applies(72, 72, code, 0, 1) == 0 and lib.dfft_stft1d_fused_applies(36, code) == 0
        # several slices: the partial sums are what the fused cross-spectra lease
        frames = CM.WC.frame_counts(CM.RCSD_M, CM.RCSD_ROWS)[1]
        assert lib.dfft_rcsd1d_slices(2 * CM.RCSD_M, CM.RCSD_ROWS, frames, code) >= 2
        assert lib.dfft_rcsd1d_slices(2 * CM.RCSD_M, CM.RCSD_ROWS, 1, code) == 1
        batch = CM.XC.batches(CM.RXSPEC_M, CM.RXSPEC_CHANNELS)[1]
        assert lib.dfft_rxspec1d_slices(2 * CM.RXSPEC_M, CM.RXSPEC_CHANNELS, batch, code) >= 2
        assert lib.dfft_rxspec1d_slices(2 * CM.RXSPEC_M, CM.RXSPEC_CHANNELS, 1, code) == 1
        assert lib.dfft_rxspec1d_long_slices(CM.LONG_M, 1, CM.XL.ragged_batch(CM.LONG_M), code) >= 2
        # several chunks: the capped lease is five items, fewer than the call has
        M, hop, pad, n, _ = CM.STFT_BASE
        stft_items = CM.SC.ROWS * CM.SC.frames_of(n, 2 * M, hop, pad)
        for name, whole_name, item, items in (
                (f"stft-64-chunks-{prec}", f"stft-64-composed-{prec}", CM.stft_item_bytes(128, prec, "complex"), stft_items),
                (f"stft-64-chunks-power-{prec}", f"stft-64-composed-power-{prec}", CM.stft_item_bytes(128, prec, "power"), stft_items),
                (f"istft-64-chunks-{prec}", f"istft-64-{prec}", CM.istft_item_bytes(128, prec, True), CM.SC.ROWS * CM.ISTFT_BASE[3]),
                (f"rcsd-cross-chunks-{prec}", f"rcsd-cross-composed-{prec}", CM.rcsd_item_bytes(128, prec), CM.RCSD_ROWS * frames),
                (f"rcsd-auto-chunks-{prec}", f"rcsd-auto-composed-{prec}", CM.rcsd_item_bytes(128, prec), CM.RCSD_ROWS * frames)):
            assert items > 5 and by[name].need(lib) == 5 * item < by[whole_name].need(lib), (name, by[name].need(lib), item, by[whole_name].need(lib))
    assert lib.dfft_rxspec1d_long_fused_applies(CM.LONG_SPILL_M, 0) == 0 and lib.dfft_rxspec1d_long_fused_applies(CM.LONG_SPILL_M, 1) == 1


def test_the_new_lease_queries_follow_the_routines_rules():
    """dfft_rfft1d / dfft_rfft2d_batch / dfft_fft2d_batch: nothing for the one-launch forms, the documented sizes elsewhere, 0 for refusals"""
    lib = _lib()
    for prec in A.PRECS:
        code, cs = CM.CODE[prec], CM.ESIZE[prec]
        assert lib.dfft_rfft1d_scratch_bytes(512, 3, code, +1) == 0 == lib.dfft_rfft1d_scratch_bytes(512, 3, code, -1)
        assert lib.dfft_rfft1d_scratch_bytes(72, 3, code, +1) == 0 and lib.dfft_rfft1d_scratch_bytes(72, 3, code, -1) == 3 * 37 * cs   # the copied bins
        assert lib.dfft_rfft1d_scratch_bytes(243, 3, code, +1) == 0 and lib.dfft_rfft1d_scratch_bytes(1009, 3, code, +1) > 0
        assert lib.dfft_rfft1d_scratch_bytes(512, 0, code, +1) == 0 == lib.dfft_rfft1d_scratch_bytes(512, 3, 7, +1) == lib.dfft_rfft1d_scratch_bytes(512, 3, code, 0)
        assert lib.dfft_fft2d_batch_scratch_bytes(256, 256, 2, code) == 0 == lib.dfft_fft2d_batch_scratch_bytes(4096, 4096, 1, code)
        assert lib.dfft_fft2d_batch_scratch_bytes(8192, 8, 2, code) == 2 * 8192 * 8 * cs == lib.dfft_fft2d_batch_scratch_bytes(8, 8192, 2, code)
        assert lib.dfft_fft2d_batch_scratch_bytes(97, 8, 2, code) == 0      # a Bluestein axis is refused
        assert lib.dfft_rfft2d_batch_scratch_bytes(64, 96, 3, code, +1) == 0
        assert lib.dfft_rfft2d_batch_scratch_bytes(64, 96, 3, code, -1) == 3 * 64 * 49 * cs                  # the bins of the plane group
        assert lib.dfft_rfft2d_batch_scratch_bytes(8192, 96, 2, code, +1) == lib.dfft_fft1d_any_scratch_bytes(8192, 49, 2, code) > 0
        assert lib.dfft_rfft2d_batch_scratch_bytes(8192, 96, 2, code, -1) == 2 * (2 * 8192 * 49 * cs)        # the bins and the four-step scratch
        assert lib.dfft_rfft2d_batch_scratch_bytes(64, 0, 3, code, +1) == 0


# ---- completeness -------------------------------------------------------------------------------------------------------------------------
def test_the_registry_is_complete():
    """Every symbol of _lib.SIGNATURES is an op's entry point or excluded with a reason -- never both, never neither -- and every entry
    point whose last argument is a caller's stream and that is not excluded for a stated reason is registered."""
    from distributedfft_amd import _lib as L
    registered = {op.entry for op in CM.REGISTRY}
    for name in L.SIGNATURES:
        reason = CM.exclusion(name)
        assert (name in registered) != (reason is not None), (name, reason)
    assert registered <= set(L.SIGNATURES)
    header = (ROOT / "include" / "dfft.h").read_text()
    takes_stream = set(re.findall(r"^\w[\w ]*?\b(dfft_\w+)\([^;]*?void\* stream\);", header, re.M | re.S))
    assert registered <= takes_stream, registered - takes_stream
    for name in takes_stream - registered:
        assert CM.exclusion(name), name
    for pattern, reason in CM.EXCLUDED:
        assert reason and any(re.fullmatch(pattern, n) for n in L.SIGNATURES), pattern


def test_every_op_has_both_precisions_and_a_named_bound():
    names = {op.name.rsplit("-", 1)[0] for op in CM.REGISTRY}
    for base in names:
        assert f"{base}-f64" in CM.BY_NAME, base
        assert f"{base}-f32" in CM.BY_NAME or base == "lxspec-cross-spilling-split", base     # that split spills in fp64 only
    for op in CM.REGISTRY:
        assert op.bound_name and op.bound > 0, op


# ---- the tour -----------------------------------------------------------------------------------------------------------------------------
def test_tour_covers_every_ordered_pair():
    for k in range(2, max(len(CM.ops(p)) for p in A.PRECS) + 1):
        walk = CM.tour(k)
        assert len(walk) == k * (k - 1) + 1 and walk[0] == walk[-1] == 0
        pairs = set(zip(walk, walk[1:]))
        assert pairs == {(a, b) for a in range(k) for b in range(k) if a != b}, k
        assert CM.tour(k) == walk                       # deterministic
    k = len(CM.REGISTRY)                                # the mixed tour walks the whole registry
    walk = CM.tour(k)
    assert len(set(zip(walk, walk[1:]))) == k * (k - 1) == len(walk) - 1


# ---- the references -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", CM.REGISTRY + [CM.long_op("f64")], ids=repr)
def test_cpu_model_of_the_reference_is_under_the_bound(op):
    inputs, shape, dtype, ref = op.case
    got = op.model()
    assert got.shape == shape == ref.shape and got.dtype == dtype, (op, got.shape, shape, ref.shape, got.dtype, dtype)
    value = op.measure(got)
    print(f"call mix {op}: CPU model nu {value:.3f} (bound {op.bound}: {op.bound_name})")
    assert value <= op.bound, (op, value, op.bound)
    for a in inputs.values():
        assert a.dtype in (A.RDT[op.prec], A.CDT[op.prec]) and a.flags.c_contiguous and not a.flags.writeable


# ---- the hooks ----------------------------------------------------------------------------------------------------------------------------
def test_hooks_and_queries_are_declared_and_bound():
    from distributedfft_amd import _lib as L
    header = (ROOT / "include" / "dfft.h").read_text()
    lib = _lib()
    for name in HOOKS + QUERIES:
        assert name in L.SIGNATURES and re.search(r"\b" + name + r"\(", header), name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert L.SIGNATURES["dfft_debug_scratch_fill"] == (C.c_int, [C.c_ulonglong, C.c_int, C.c_void_p])
    assert L.SIGNATURES["dfft_debug_scratch_capacity"] == (C.c_ulonglong, [C.c_void_p])
    assert L.SIGNATURES["dfft_debug_scratch_count"] == (C.c_longlong, [C.c_int, C.c_void_p])
    design = (ROOT / "DESIGN.md").read_text()
    assert all(name in design for name in HOOKS), "DESIGN.md documents the test hooks"


def test_hooks_without_a_device_fail_cleanly():
    """Where no device is visible: an error code, 0 bytes and an error code, with a message; nothing is touched.  (Where one is visible
    this is tests/test_gpu_call_mix.py's business.)"""
    from distributedfft_amd import _lib as L
    lib = _lib()
    if lib.dfft_device_count() > 0:
        assert lib.dfft_debug_scratch_capacity(None) >= 0
        return
    assert lib.dfft_debug_scratch_fill(1 << 20, 0xFF, None) == L.ENOGPU and b"no HIP device" in lib.dfft_last_error()
    assert lib.dfft_debug_scratch_capacity(None) == 0
    assert lib.dfft_debug_scratch_count(0xFF, None) == L.ENOGPU
    assert lib.dfft_debug_scratch_fill(0, 0, C.c_void_p(1234)) == L.ENOGPU and lib.dfft_debug_scratch_capacity(C.c_void_p(1234)) == 0
