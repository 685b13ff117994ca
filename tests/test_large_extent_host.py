"""No GPU: the helper of the large-extent tests (tests/large_extent.py) at small shapes on CPU tensors, numpy standing in for the transform.

A correct output passes; an unwritten line, a line written at its offset modulo a small power of two (the stand-in for 2^32), a swapped
column pair, a chunk shifted by one unit and a changed input element are each rejected, and the report names the line.  The wrap assertion
is held for every tensor of tests/test_gpu_large_extent.py's case tables and against a brute-force count at small shapes; the mirrors of
the library's chunk rules are held against its dfft_*_scratch_bytes exports; the extent rule of dfft_fft1d_cols and the one-launch
predicates are pinned on both sides of every switch, at the shapes no test can allocate as well.

The second half does the same for rows whose neighbouring lines interact (large_extent.Band: overlap-save, STFT, inverse STFT, one row
and many) and for the tables of tests/test_gpu_large_extent_rows.py: a correct output passes; an unwritten line, a line written at its
offset modulo 1024, a chunk shifted by one item, a wrong filter row for rows past an index, a changed input sample and an edge line
treated as an interior line are rejected with the line named; the wrap assertion holds for every tensor and every Band; the routes and
scratch sizes the cases rely on are pinned on both sides, and so is every 2^31 refusal that a run case sits just under."""
import itertools

import numpy as np
import pytest

import large_extent as LE
import rconv1d_os_cases as OC
import stft_cases as SC
import test_gpu_large_extent as G
import test_gpu_large_extent_rows as GR

F64, F32 = 0, 1
K = LE.K_DEFAULT
N, S, BATCH = 16, 11, 13          # 143 lines of 16 points: every base line at least twice


@pytest.fixture
def small_slices(monkeypatch):
    """slices of a few items, so that both block forms and many blocks are walked"""
    monkeypatch.setattr(LE, "SLICE_BYTES", 3 * N * S * 16)


def _cpu():
    import torch
    return torch.device("cpu")


def _fft(spoil=None):
    def call(x, out):
        import torch
        out.copy_(torch.from_numpy(np.fft.fft(x.numpy(), axis=1)))
        if spoil:
            spoil(x, out)
    return call


def _case(call, inplace, K_=K):
    x, ref = LE.complex_base(N, K_, +1)
    return LE.run_case(_cpu(), "host stand-in", "tuned", "f64", N, x, ref, BATCH, S, call, inplace, K=K_)


@pytest.mark.parametrize("inplace", [True, False], ids=["in-place", "out-of-place"])
def test_a_correct_output_passes(small_slices, inplace):
    dt, peak = _case(_fft(), inplace)
    assert peak == BATCH * N * S * 16 * (1 if inplace else 2) + LE.GIB


def test_column_slices_of_one_item_pass_too(monkeypatch):
    monkeypatch.setattr(LE, "SLICE_BYTES", N * 16 * 4)      # less than one item: column ranges of 4 (2 in the fp64 comparison)
    assert len(list(LE.blocks(BATCH, N, S, 16))) == BATCH * 3
    _case(_fft(), False)


def _rejected(spoil, inplace, *lines):
    """the case fails and its report names one of `lines` ((b, c) pairs)"""
    with pytest.raises(AssertionError) as e:
        _case(_fft(spoil), inplace)
    text = str(e.value)
    assert any(f"({b}, {c})" in text for b, c in lines), (text, lines)


def test_an_unwritten_line_is_rejected(small_slices):
    def unwritten_out_of_place(x, out):
        out[7, :, 4] = float("nan")               # what the NaN pre-fill leaves
    _rejected(unwritten_out_of_place, False, (7, 4))

    def unwritten_in_place(x, out):
        out[7, :, 4] = LE.base_tensor(LE.complex_base(N, K, +1)[0], "f64", _cpu())[:, (7 * S + 4) % K]   # still its input
    _rejected(unwritten_in_place, True, (7, 4))


def test_a_line_written_at_its_offset_modulo_a_power_of_two_is_rejected(small_slices):
    """Line (9, 3) lands at flat offsets modulo 1024 elements, over earlier lines, and its own place keeps the pre-fill."""
    W, b, c = 1024, 9, 3

    def wrapped(x, out):
        flat = out.view(-1)
        line = out[b, :, c].clone()
        out[b, :, c] = float("nan")
        for k in range(N):
            flat[((b * N + k) * S + c) % W] = line[k]
    landed = [((b * N + k) * S + c) % W for k in range(N)]
    hit = {(b, c)} | {(f // S // N, f % S) for f in landed}
    _rejected(wrapped, False, *hit)


def test_a_swapped_column_pair_is_rejected(small_slices):
    def swapped(x, out):
        a = out[5, :, 6].clone()
        out[5, :, 6] = out[5, :, 7]
        out[5, :, 7] = a
    _rejected(swapped, True, (5, 6), (5, 7))


def test_a_chunk_shifted_by_one_unit_is_rejected(small_slices):
    def shifted(x, out):
        out[4:8] = out[5:9].clone()               # items 4 ... 7 hold their successors' lines
    _rejected(shifted, True, *[(b, c) for b in range(4, 8) for c in range(S)])


def test_a_changed_input_element_is_rejected(small_slices):
    def touched(x, out):
        x[6, 9, 2] += 1
    with pytest.raises(AssertionError) as e:
        _case(_fft(touched), False)
    assert "(6, 9, 2)" in str(e.value) and "input" in str(e.value)


# ---- the wrap assertion ------------------------------------------------------------------------------------------------------------------
def test_wrap_hits_agrees_with_brute_force():
    for batch, m, s, K_, shift in itertools.product((3, 8), (4, 6), (1, 5, 7), (3, 5, 7), (1, 5, 7, 20, 24, 35, 64, 105)):
        total = batch * m * s
        e = np.arange(max(0, total - shift))
        if not len(e):
            assert LE.wrap_hits(batch, m, s, K_, shift) == []
            continue

        def ident(f):
            row, c = np.divmod(f, s)
            b, k = np.divmod(row, m)
            return (b * s + c) % K_, k
        (l0, k0), (l1, k1) = ident(e), ident(e + shift)
        same = bool(np.any((l0 == l1) & (k0 == k1)))
        # the closed form looks at shifts as if the tensor went on for ever: it may reject a shift whose only hits lie past the end
        assert same <= bool(LE.wrap_hits(batch, m, s, K_, shift)), (batch, m, s, K_, shift)
        if total >= 4 * shift + 4 * m * s:
            assert same == bool(LE.wrap_hits(batch, m, s, K_, shift)), (batch, m, s, K_, shift)


def test_wrapped_accesses_land_on_other_values_for_every_case_shape():
    shapes = G.all_shapes()
    assert len(shapes) >= 25
    for what, batch, m, s, eb in shapes:
        assert batch * s >= K, what
        assert LE.pick_k([(batch, m, s, eb)]) in LE.K_CANDIDATES, what
        assert batch * m * s * eb <= 36 << 30, (what, "a tensor of more than 36 GiB")
    picked = {what: LE.pick_k([(b, m, s, eb)]) for what, b, m, s, eb in shapes}
    print("K per tensor other than 61:", {w: k for w, k in picked.items() if k != K})
    # a K that divides the line shift of a wrap is rejected: 160 elements of [100][4][8] are 5 items, i.e. 40 lines
    assert LE.wrap_hits(100, 4, 8, 5, 160) == [(0, 40)] and LE.wrap_hits(100, 4, 8, 7, 160) == []


# ---- the mirrors of the chunk rules ----------------------------------------------------------------------------------------------------------
def test_chunk_rule_mirrors_match_the_library(native_lib, monkeypatch):
    lib = native_lib
    for fused_env in ("1", "0"):
        monkeypatch.setenv("DFFT_BLUESTEIN_FUSED", fused_env)
        for prec, code in (("f64", F64), ("f32", F32)):
            for n, s, batch in [(4099, 5, 466), (4099, 1, 100000), (1009, 3, 40000), (2039, 1053226, 1), (2039, 7, 3), (65537, 2, 900), (11, 1, 5)]:
                M = lib.dfft_bluestein_length(n)
                fused = bool(lib.dfft_bluestein_fused_applies(n, s))
                assert fused == (fused_env == "1" and n <= 2048 and (s == 1 or n * s < 2 ** 31)), (n, s)
                served = lib.dfft_fft1d_any_extent_supported(n, s, code, 1, 1)
                assert served == (0 if (n, s, prec) == (2039, 1053226, "f64") else 1)
                want = LE.bluestein_scratch(M, s, batch, prec, fused) if served else 0      # a refused call leases nothing
                assert lib.dfft_fft1d_any_scratch_bytes(n, s, batch, code) == want, (n, s, batch, prec)
            assert lib.dfft_fft1d_any_scratch_bytes(8192, 3, 7, code) == 7 * 8192 * 3 * LE.CBYTES[prec] and lib.dfft_fft1d_any_scratch_bytes(512, 3, 7, code) == 0
            for n, s, batch in [(375, 1000, 207), (375, 1, 208781), (16384, 6, 795), (1009, 7, 9000), (512, 64, 3000), (512, 4194304, 1), (512, 4194305, 2)]:
                M = lib.dfft_bluestein_length(n)
                sp = 1 if s == 1 else (s + 1) // 2
                bs_fused = bool(M) and bool(lib.dfft_bluestein_fused_applies(n, sp))
                for kind in range(4):
                    vec = int(s > 1 and s % 2 == 0)
                    want = 0 if lib.dfft_r2r_fused_applies(n, s, code, kind, vec) else LE.composed_scratch(n, s, batch, prec, M, bs_fused)
                    assert lib.dfft_r2r1d_strided_scratch_bytes(n, s, batch, code, kind, vec) == want, (n, s, batch, prec, kind)
                if s > 1:
                    want = 0 if lib.dfft_rfft_cols_fused_applies(n, s, code) else LE.composed_scratch(n, s, batch, prec, M, bs_fused, rows_pair=False)
                    assert lib.dfft_rfft1d_strided_scratch_bytes(n, s, batch, code) == want, (n, s, batch, prec)
    # under DFFT_R2R_FUSED=0 every length takes the composed route
    monkeypatch.setenv("DFFT_R2R_FUSED", "0")
    assert lib.dfft_r2r_fused_applies(512, 64, F32, 0, 1) == 0
    assert lib.dfft_r2r1d_strided_scratch_bytes(512, 64, 3000, F32, 0, 1) == LE.composed_scratch(512, 64, 3000, "f32", 0, False)


def test_ragged_batch_is_two_chunks_and_a_third():
    for cu in (1, 2, 3, 89, 44739):
        b = LE.ragged_batch(cu)
        assert 2 * cu < b <= 3 * cu and (b - 2 * cu) in (1, cu // 3)


# ---- the extent rule of dfft_fft1d_cols and the one-launch predicates --------------------------------------------------------------------------
def test_cols_extent_rule(native_lib):
    ok = native_lib.dfft_cols_extent_supported
    for n, width, prec in G.COLS_REFUSED:
        assert ok(n, width, G.CODE[prec], 0) == 0
        assert ok(n, width, G.CODE[prec], 1) == (1 if n == 8192 else 0)   # 128 * width is even: an aligned pass A runs on pairs
    for cid, n, width, _, prec, _ in G.COLS:
        assert ok(n, width, G.CODE[prec], 0 if cid in G.OFFSET else 1) == 1
    # the rule itself, in the kernel's units: (n - 1) * w + 63 < 2^32
    edge = (2 ** 32 - 64) // 4095                 # the widest w of 4096-point columns
    assert (ok(4096, edge, F64, 0), ok(4096, edge + 1, F64, 0)) == (1, 0)                  # fp64: elements of 16 bytes
    assert (ok(4096, edge, F32, 0), ok(4096, edge + 1, F32, 0)) == (1, 0)                  # scalar fp32 (odd width or unaligned)
    assert (ok(4096, 2 * edge, F32, 1), ok(4096, 2 * edge + 2, F32, 1)) == (1, 0)          # fp32 column pairs: twice the width
    assert ok(4096, 2 * edge, F32, 0) == 0                                                 # ... the same width on 8-byte-aligned pointers
    assert ok(4096, 2 * edge, F64, 1) == 0                                                 # `pairs` means nothing to fp64
    assert (ok(2048, (2 ** 32 - 64) // 2047, F64, 0), ok(2048, (2 ** 32 - 64) // 2047 + 1, F64, 0)) == (1, 0)   # the split-line lengths
    assert (ok(1024, (2 ** 32 - 64) // 1023, F32, 0), ok(1024, (2 ** 32 - 64) // 1023 + 1, F32, 0)) == (1, 0)
    # column indices are ints: width <= 2^31 - 64 for every length, and no other limit for the run-time-scheduled and four-step lengths
    assert (ok(2, 2 ** 31 - 64, F32, 0), ok(2, 2 ** 31 - 63, F32, 0), ok(2, 2 ** 31, F64, 0)) == (1, 0, 0)
    assert ok(3600, 2 ** 31 - 64, F64, 0) == 1 and ok(3600, 2 ** 31 - 63, F64, 0) == 0
    # four-step 8192 = 64 * 128: pass A runs 64 points over 128 * width columns (pairs iff `in` is aligned), pass B 128 points over width
    edge = (2 ** 32 - 64) // (63 * 128)
    assert edge == 532610
    assert (ok(8192, edge, F64, 1), ok(8192, edge + 1, F64, 1)) == (1, 0)
    assert (ok(8192, edge, F32, 0), ok(8192, edge + 1, F32, 0)) == (1, 0)
    assert (ok(8192, 2 * edge, F32, 1), ok(8192, 2 * edge + 1, F32, 1)) == (1, 0)
    assert ok(8192, 2 ** 30, F64, 0) == 0 and ok(8192, 2 ** 31, F64, 0) == 0
    # 6561 = 81 * 81 (odd factors): an odd width leaves both passes on scalar fp32, whatever the alignment
    edge = (2 ** 32 - 64) // (80 * 81)
    assert (ok(6561, edge, F64, 1), ok(6561, edge + 1, F64, 1)) == (1, 0)
    odd = edge if edge % 2 else edge - 1
    assert (ok(6561, odd, F32, 1), ok(6561, odd + 2, F32, 1)) == (1, 0)
    # dfft_fft1d_any is the same rule for kinds 1 and 2, with the two pointers told apart: pass A of a four-step length reads `in` only
    any_ok = native_lib.dfft_fft1d_any_extent_supported
    e8 = 532610
    assert (any_ok(8192, 2 * e8, F32, 1, 0), any_ok(8192, 2 * e8, F32, 0, 1)) == (1, 0)
    assert (any_ok(4096, 2 * 1048832, F32, 1, 1), any_ok(4096, 2 * 1048832, F32, 1, 0), any_ok(4096, 2 * 1048832, F32, 0, 1)) == (1, 0, 0)
    assert any_ok(8192, 1, F64, 0, 0) == 1 and any_ok(4096, 1, F32, 0, 0) == 1           # rows: no such limit
    assert ok(0, 8, F64, 0) == 0 and ok(8, 0, F64, 0) == 0 and ok(8, 8, 2, 0) == 0


def test_cols_over_the_extent_are_refused_before_the_device_is_queried(native_lib):
    """DFFT_EUNSUPPORTED with or without a GPU: the pointers (a small host array) are never used."""
    from distributedfft_amd import _lib
    buf = np.zeros(64, dtype=np.complex64)
    for n, width, prec in G.COLS_REFUSED + [(4096, 2 ** 31, "f64"), (2, 2 ** 31 - 63, "f32")]:
        p = buf.ctypes.data + (8 if n == 8192 else 0)        # the four-step shape is over the rule of an 8-byte-aligned `in`
        assert p % 16 == (8 if n == 8192 else 0)
        rc = native_lib.dfft_fft1d_cols(p, p, n, width, 1, G.CODE[prec], 1, None)
        assert rc == _lib.EUNSUPPORTED, (n, width, prec, rc, native_lib.dfft_last_error())
        assert b"dfft_fft1d_cols" in native_lib.dfft_last_error()
    assert not buf.any()


def test_bluestein_extent_past_the_one_launch_form(native_lib, monkeypatch):
    """n * s >= 2^31 runs the M-point passes on the 16-byte-aligned scratch: (M - 1) * w + 63 < 2^32 with w = s / 2 for fp32 with even s,
    w = s otherwise -- and M >= 2n - 1, so fp64 and odd s are never served there.  Refused before the device is queried."""
    from distributedfft_amd import _lib
    monkeypatch.delenv("DFFT_BLUESTEIN_FUSED", raising=False)
    lib, any_ok = native_lib, native_lib.dfft_fft1d_any_extent_supported
    assert lib.dfft_bluestein_length(2039) == 4096
    for al in (0, 1):                                         # the caller's alignment does not matter: the passes run on the scratch
        assert [any_ok(2039, s, F32, al, al) for s in (1053204, 1053226, 1053227, 1053228)] == [1, 1, 0, 1]
        assert [any_ok(2039, s, F64, al, al) for s in (1053204, 1053226, 1053228)] == [1, 0, 0]
    top = 2 * ((2 ** 32 - 64) // 4095)                        # the widest even s of fp32: 34 GB of data, 69 GB of scratch
    assert (any_ok(2039, top, F32, 1, 1), any_ok(2039, top + 2, F32, 1, 1)) == (1, 0)
    # n > 2048: always multi-pass, M = 8232 is a four-step length, whose pass A is the limit
    M = lib.dfft_bluestein_length(4099)
    assert M > 4096 and any_ok(4099, 5, F64, 1, 1) == 1 and any_ok(4099, 1, F64, 0, 0) == 1 and any_ok(4099, 2 ** 22, F64, 1, 1) == 0
    # under DFFT_BLUESTEIN_FUSED=0 the same rule holds below n * s = 2^31 (everything there fits)
    monkeypatch.setenv("DFFT_BLUESTEIN_FUSED", "0")
    assert any_ok(2039, 1053204, F64, 1, 1) == 0 and any_ok(2039, 1000, F64, 1, 1) == 1
    monkeypatch.delenv("DFFT_BLUESTEIN_FUSED")
    buf = np.zeros(64, dtype=np.complex128)
    for n, s, prec in G.ANY_REFUSED:
        assert any_ok(n, s, G.CODE[prec], 1, 1) == 0 and lib.dfft_fft1d_any_scratch_bytes(n, s, 1, G.CODE[prec]) == 0
        rc = lib.dfft_fft1d_any(buf.ctypes.data, buf.ctypes.data, n, s, 1, G.CODE[prec], 1, None)
        assert rc == _lib.EUNSUPPORTED and b"dfft_fft1d_any" in lib.dfft_last_error(), (n, s, prec, rc)
    assert not buf.any()
    # the composed routes refuse the same way: packed pairs of an r2r / real-column call whose inner columns pass the rule
    sp_over = (2 ** 32 - 64) // 511 + 2                       # 512-point columns over sp scalar units (odd sp)
    sp_over += 1 - sp_over % 2
    s_over = 2 * sp_over - 1
    rbuf = np.zeros(64, dtype=np.float32)
    assert lib.dfft_r2r1d_strided(rbuf.ctypes.data, rbuf.ctypes.data, 512, s_over, 1, F32, 0, None) == _lib.EUNSUPPORTED
    assert not rbuf.any()
    if lib.dfft_device_count() == 0:
        # out of place, so two disjoint ranges of 34 GB each: made-up addresses, which only a machine without a device may be handed
        assert lib.dfft_rfft1d_strided(1 << 44, 1 << 46, 512, s_over, 1, F32, 1, None) == _lib.EUNSUPPORTED
        assert lib.dfft_rfft1d_strided(1 << 46, 1 << 44, 512, s_over, 1, F32, -1, None) == _lib.EUNSUPPORTED
        assert lib.dfft_rfft1d_strided(1 << 44, 1 << 46, 512, s_over - 2, 1, F32, 1, None) == _lib.ENOGPU   # just under: accepted


def test_one_launch_predicates_switch_at_2_pow_31(native_lib, monkeypatch):
    lib = native_lib
    monkeypatch.delenv("DFFT_BLUESTEIN_FUSED", raising=False)
    monkeypatch.delenv("DFFT_R2R_FUSED", raising=False)
    # Bluestein columns: n * s < 2^31; rows (s = 1) always; never above 2048 points or for another kind of length
    for cid, n, s, batch, prec, fused in G.ANY:
        assert bool(lib.dfft_bluestein_fused_applies(n, s)) == fused, cid
    s_edge = (2 ** 31 - 1) // 2039
    assert (lib.dfft_bluestein_fused_applies(2039, s_edge), lib.dfft_bluestein_fused_applies(2039, s_edge + 1)) == (1, 0)
    assert lib.dfft_bluestein_fused_applies(2039, 1) == 1 and lib.dfft_bluestein_fused_applies(2053, 3) == 0
    assert lib.dfft_bluestein_fused_applies(2048, 3) == 0 and lib.dfft_bluestein_fused_applies(11, (2 ** 31) // 11 + 1) == 0
    # the multi-pass form of such a call: one padded item of M * s elements
    assert lib.dfft_fft1d_any_scratch_bytes(2039, 1053226, 1, F32) == 4096 * 1053226 * 8
    for cid, n, s, batch, prec, fused in G.REAL:
        if fused is not None:
            assert bool(lib.dfft_rfft_cols_fused_applies(n, s, G.CODE[prec])) == fused, cid
    for cid, n, s, batch, prec, kinds, places, fused in G.R2R:
        for kind in kinds:
            from distributedfft_amd import api
            assert bool(lib.dfft_r2r_fused_applies(n, s, G.CODE[prec], api.R2R_KINDS[kind], int(s > 1 and s % 2 == 0))) == fused, (cid, kind)
    # fp64 at the same switch (17 GB and more per tensor: pinned here only)
    assert (lib.dfft_rfft_cols_fused_applies(512, 4194303, F64), lib.dfft_rfft_cols_fused_applies(512, 4194304, F64)) == (1, 0)
    assert (lib.dfft_r2r_fused_applies(512, 4194302, F64, 0, 1), lib.dfft_r2r_fused_applies(512, 4194304, F64, 0, 1)) == (1, 0)
    assert lib.dfft_r2r_fused_applies(512, 1, F32, 1, 0) == 1     # rows have no such limit


# ---- rows whose neighbouring lines interact: the Band helper on CPU tensors --------------------------------------------------------------------
@pytest.fixture
def band_slices(monkeypatch):
    """slices of a few dozen lines, so that many blocks are walked"""
    monkeypatch.setattr(LE, "SLICE_BYTES", 1 << 13)
    GR.register_bounds()


def _os_host():
    """overlap-save, one row: m = 16, d = 6, lines of S = 10 samples"""
    M, d, lines = 8, 6, 200
    band = LE.Band(1, lines, lines, 1, 0)
    base, H, small = GR.os_band_base(M, d, "complex", K)

    def call(x, out):
        import torch
        out.copy_(torch.from_numpy(OC.reference(x.numpy().reshape(1, -1), H, 2 * M, d, lines * 10).astype(np.float64).reshape(lines, 10)))
    return "rconv1d_os", 2 * M, base, small, band, 10, False, call


def _stft_host(kind="complex"):
    """STFT, one row: m = 16, hop = 4 (every frame spans four lines), no edge line"""
    M, hop, lines = 8, 4, 300
    band = LE.Band(1, lines, lines - 3, 0, 3)
    base, win, small = GR.stft_base(M, hop, kind, K)

    def call(x, out):
        import torch
        X = SC.reference(x.numpy().reshape(1, -1), win, 2 * M, hop, 0, lines - 3, "zero")[0]
        out.copy_(torch.from_numpy((SC.power(X).astype(np.float64) if kind == "power" else X.astype(np.complex128))))
    return "stft" if kind == "complex" else "stft-power", 2 * M, base, small, band, M + 1, kind == "complex", call


def _istft_host(rows=1, frames=200):
    """inverse STFT: m = 16, hop = 4: three head and three tail lines per row"""
    M, hop = 8, 4
    band = LE.Band(rows, frames, frames + 3, 3, 0)
    base, win, small = GR.istft_base(M, hop, K)
    inv = GR.istft_envelope_lines(win, 2 * M, hop, frames).reshape(-1)

    def call(x, out):
        import torch
        y = SC.inverse_reference(x.numpy().reshape(rows, frames, M + 1), win, inv, (frames + 3) * hop, 2 * M, hop, 0)
        out.copy_(torch.from_numpy(y.astype(np.float64).reshape(-1, hop)))
    return "istft", 2 * M, base, small, band, hop, False, call


BAND_HOSTS = {"os": _os_host, "stft": _stft_host, "stft-power": lambda: _stft_host("power"), "istft": _istft_host,
              "istft-rows": lambda: _istft_host(70, 130)}


def _band_case(host, spoil=None):
    family, m, base, small, band, p_out, cplx, call = host

    def spoiled(x, out):
        call(x, out)
        if spoil:
            spoil(x, out)
    return LE.run_band_case(_cpu(), "host stand-in", family, "f64", m, base, small, band, p_out, cplx, spoiled, K=K)


def _band_rejected(host, spoil, *lines):
    with pytest.raises(AssertionError) as e:
        _band_case(host, spoil)
    text = str(e.value)
    assert any(f"({r}, {t})" in text for r, t in lines), (text, lines)


@pytest.mark.parametrize("name", sorted(BAND_HOSTS))
def test_band_a_correct_output_passes(band_slices, name):
    host = BAND_HOSTS[name]()
    dt, peak = _band_case(host)
    band = host[4]
    assert band.tail == {"os": 0, "stft": 0, "stft-power": 0, "istft": 3, "istft-rows": 3}[name]
    assert peak > LE.GIB


def test_band_inverse_envelope_of_a_long_row_is_its_head_interior_and_tail(band_slices):
    win = SC.window(16, "hann")
    want = GR.istft_envelope_lines(win, 16, 4, 200).reshape(-1)
    got = GR.istft_inv_env(win, 16, 4, 200, "f64", _cpu()).numpy()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", ["os", "stft", "istft", "istft-rows"])
def test_band_an_unwritten_line_is_rejected(band_slices, name):
    host = BAND_HOSTS[name]()
    band = host[4]
    r, t = band.rows - 1, band.lout // 2 + 7

    def unwritten(x, out):
        out[r * band.lout + t] = float("nan")
    _band_rejected(host, unwritten, (r, t))


@pytest.mark.parametrize("name", ["os", "stft", "istft-rows"])
def test_band_a_line_written_at_its_offset_modulo_a_power_of_two_is_rejected(band_slices, name):
    host = BAND_HOSTS[name]()
    band, p = host[4], host[5]
    g, W = band.rows * band.lout - 9, 1024

    def wrapped(x, out):
        flat = out.view(-1)
        line = out[g].clone()
        out[g] = float("nan")
        for k in range(p):
            flat[(g * p + k) % W] = line[k]
    hit = {divmod(g, band.lout)} | {divmod(((g * p + k) % W) // p, band.lout) for k in range(p)}
    _band_rejected(host, wrapped, *hit)


@pytest.mark.parametrize("name", ["os", "stft", "istft", "istft-rows"])
def test_band_a_chunk_shifted_by_one_item_is_rejected(band_slices, name):
    host = BAND_HOSTS[name]()
    band = host[4]
    g0 = (band.rows - 1) * band.lout + 140 if band.rows == 1 else 5 * band.lout + 40

    def shifted(x, out):
        out[g0:g0 + 16] = out[g0 + 1:g0 + 17].clone()
    _band_rejected(host, shifted, *[divmod(g, band.lout) for g in range(g0, g0 + 16)])


@pytest.mark.parametrize("name", ["os", "stft", "istft-rows"])
def test_band_a_changed_input_sample_is_rejected(band_slices, name):
    host = BAND_HOSTS[name]()

    def touched(x, out):
        x[150, 2] += 1
    with pytest.raises(AssertionError) as e:
        _band_case(host, touched)
    assert "(150, 2, 0)" in str(e.value) and "input" in str(e.value)


@pytest.mark.parametrize("name,edge", [("os", "head"), ("istft", "head"), ("istft", "tail"), ("istft-rows", "head"), ("istft-rows", "tail")])
def test_band_an_edge_line_treated_as_an_interior_line_is_rejected(band_slices, name, edge):
    """The edge line holds what an interior line of its class holds (a window that wrapped round the row's end instead of being cut)."""
    host = BAND_HOSTS[name]()
    band = host[4]
    r = band.rows - 1
    t = 0 if edge == "head" else band.lout - 1
    cls = (r * band.lin + t) % K

    def as_interior(x, out):
        out[r * band.lout + t] = out[K + cls]     # line K + cls of row 0 is the interior line of that class
    _band_rejected(host, as_interior, (r, t))


def test_band_rows_past_the_first_K_have_their_edges_compared(band_slices):
    """Row 69 of 70: a head line that holds row 9's head line is rejected although its own reference is never computed (it is held against
    the head line of row 69 mod 61 = 8, which starts with the same base lines)."""
    host = BAND_HOSTS["istft-rows"]()
    band = host[4]

    def spoil(x, out):
        out[69 * band.lout + 1] = out[9 * band.lout + 1]
    _band_rejected(host, spoil, (69, 1))


def test_band_wrap_hits_agrees_with_brute_force():
    for rows, lin, lout, p, K_, dq in itertools.product((1, 4, 9), (11, 13), (0, 2), (1, 3), (3, 5, 7), (1, 5, 7, 12, 15, 26, 35)):
        band = LE.Band(rows, lin, lin + lout, lout, 0)
        shift = dq * p
        g = np.arange(rows * band.lout)
        r, t = np.divmod(g, band.lout)
        cls = (r * lin + t) % K_
        ok = g + dq < rows * band.lout
        same = bool(np.any(cls[g[ok]] == cls[(g + dq)[ok]]))
        assert same <= bool(LE.band_wrap_hits(band, p, K_, shift)), (rows, lin, lout, p, K_, dq)
        assert LE.band_wrap_hits(band, p, K_, shift + 1) == [] or p == 1
    assert not LE.band_wrap_hits(LE.Band(1, 500, 500, 1, 0), 4, 61, 4 * 60) and LE.band_wrap_hits(LE.Band(1, 500, 500, 1, 0), 4, 61, 4 * 122)


# ---- rows with one filter row each: a wrong filter row shows ----------------------------------------------------------------------------------
def test_a_wrong_filter_row_for_rows_past_an_index_is_rejected(small_slices):
    GR.register_bounds()
    M, n, rows = 8, 12, 3 * K + 5
    x, H, ref = GR.rconv_base(M, n, "complex", K)

    def conv(first_wrong):
        def call(t, out):
            import torch
            xs = t.numpy().reshape(rows, n)
            r = np.arange(rows)
            Hr = H[np.where(r >= first_wrong, (r + 1) % K, r % K)]          # rows past first_wrong take their neighbour's filter
            out.copy_(torch.from_numpy(np.fft.irfft(np.fft.rfft(xs, 2 * M, axis=1) * Hr, 2 * M, axis=1)[:, :n].reshape(rows, n, 1)))
        return call
    LE.run_case(_cpu(), "host stand-in", "rconv1d", "f64", 2 * M, x, ref, rows, 1, conv(rows), False, K=K)
    with pytest.raises(AssertionError) as e:
        LE.run_case(_cpu(), "host stand-in", "rconv1d", "f64", 2 * M, x, ref, rows, 1, conv(2 * K + 3), False, K=K)
    assert any(f"({b}, 0)" in str(e.value) for b in range(2 * K + 3, rows)), str(e.value)


# ---- the tables of tests/test_gpu_large_extent_rows.py ---------------------------------------------------------------------------------------
def test_wrapped_accesses_land_on_other_values_for_every_band():
    assert {s[0] for s in GR.shapes()} <= {s[0] for s in G.all_shapes()}        # all_shapes() covers the sibling module
    bands = GR.band_shapes()
    assert len(bands) == len(GR.OS_BAND) + len(GR.STFT) + len(GR.ISTFT)
    for what, band, p_in, p_out, eb_in, eb_out in bands:
        assert LE.band_pick_k(band, p_in, p_out, eb_in, eb_out) in LE.K_CANDIDATES, what
        peak = band.rows * (band.lin * p_in * eb_in + band.lout * p_out * eb_out)
        assert peak + 10 * LE.GIB <= LE.CAP_80, what
    # a K that divides the class shift of a wrap is rejected: rows of 9 lines from 7 frames, 15 lines on are one row and 6 lines, class + 13,
    # or two rows less 3 lines, class + 11
    b = LE.Band(40, 7, 9, 2, 0)
    assert LE.band_wrap_hits(b, 4, 13, 60) == [(0, 13)] and LE.band_wrap_hits(b, 4, 11, 60) == [(1, 11)] and LE.band_wrap_hits(b, 4, 17, 60) == []


def test_row_cases_sit_where_the_table_says():
    """rows * n, items and offsets of every case against the powers of two they are there for"""
    P31, P32 = 2 ** 31, 2 ** 32
    plans = {c[0][:2]: GR.rconv_plan(c) for c in GR.RCONV}
    assert plans["R1"][1] * 1000 > P32 and plans["R1"][2] == plans["R1"][0] and plans["R1"][1] % plans["R1"][0] == 0
    assert plans["R2"][1:] == (P31 - 1, P31 - 1, 1)
    assert plans["R3"][1] * 70 > P32 and plans["R4"][1] * 512 > P31
    assert GR.os_rows_plan(GR.OS_ROWS[0])[1] * 65538 > P32
    for c in GR.LONG:
        assert GR.long_plan(c)[1] * c[2] > P32 and c[2] < c[1] and c[2] % 2 == 0
    o1, o2, o4 = [GR.os_band(c) for c in GR.OS_BAND]
    assert o1[0].lin * o1[1] > P32 and o2[0].lin == P31 - 1 and o2[1] == 3 and o4[0].lin * o4[1] > P31
    s1, s2, s3, s4 = [GR.stft_band(c)[0] for c in GR.STFT]
    assert s1.lin * 1024 > P32 and s2.lin * 256 > P32 and s2.qa == 3 and s3.lout == P31 - 1 and s3.lout * 3 > P32 and s4.lin * 1024 > P32
    i1a, i1b, i2 = [GR.istft_band(c)[0] for c in GR.ISTFT]
    assert i1a.lout * 256 == 2 ** 20 == i1b.lout * 512 and i1a.rows * 2 ** 20 > P31 and i1a.rows * i1a.lin * 513 > P32
    assert i1b.rows * 2 ** 20 > P32 and i2.rows == 1 and i2.lout * 512 > P31 and i1a.lin % K and i1b.lin % K


def test_row_case_routes_and_the_refusals_just_over_their_guards(native_lib, monkeypatch):
    """Both sides of every switch the cases rely on, and every refusal a run case sits just under: through the entry points, which answer
    DFFT_EUNSUPPORTED before asking for a device (the pointers, a small host array, are never used)."""
    from distributedfft_amd import _lib
    lib = native_lib
    for name in ("DFFT_RCONV_FUSED", "DFFT_STFT_FUSED", "DFFT_RCONV_LONG_FUSED", "DFFT_STFT_CHUNK_BYTES", "DFFT_SCRATCH_CHUNK_BYTES"):
        monkeypatch.delenv(name, raising=False)
    P31 = 2 ** 31
    # dfft_rconv1d: a tuned half runs fused and leases nothing, M = 36 and DFFT_RCONV_FUSED=0 run composed on a 256 MiB chunk
    for cid, M, n, kind, prec, _, _, composed, _ in GR.RCONV:
        assert bool(lib.dfft_rconv1d_fused_applies(n, 2 * M, G.CODE[prec], GR.KIND[kind], 1)) == (not composed), cid
    rb = 37 * 8 + 72 * 4
    assert lib.dfft_rconv1d_scratch_bytes(70, 72, 61, 10 ** 6, F32) == (256 << 20) // rb * rb and lib.dfft_rconv1d_scratch_bytes(2, 4, P31 - 1, 1, F32) == 0
    monkeypatch.setenv("DFFT_RCONV_FUSED", "0")
    assert lib.dfft_rconv1d_fused_applies(1000, 1024, F32, 0, 1) == 0 and lib.dfft_rconv1d_scratch_bytes(1000, 1024, 61, 1000, F32) > 0
    assert lib.dfft_rconv1d_os_fused_applies(1024, F32) == 0 and lib.dfft_rconv1d_os_scratch_bytes(7680, 1024, 256, 1, 1, F32) == 10 * (513 * 8 + 1024 * 4)
    monkeypatch.delenv("DFFT_RCONV_FUSED")
    # dfft_rconv1d_os: M = 1536 is routed to the composed form in fp64 only
    assert [lib.dfft_rconv1d_os_fused_applies(m, p) for m, p in ((1024, F32), (4, F32), (3072, F32), (3072, F64), (72, F32))] == [1, 1, 1, 0, 0]
    ib = 1537 * 16 + 3072 * 8
    assert lib.dfft_rconv1d_os_scratch_bytes(2 ** 31 + 2048, 3072, 1024, 1, 1, F64) == (256 << 20) // ib * ib
    assert lib.dfft_rconv1d_os_scratch_bytes(3 * (P31 - 1), 4, 1, 1, 1, F32) == 0
    # dfft_stft1d / dfft_istft1d
    assert lib.dfft_stft1d_fused_applies(1024, F32) == 1 and lib.dfft_stft1d_fused_applies(4, F32) == 1
    assert lib.dfft_stft1d_scratch_bytes(1024, 2 ** 22 + 1, 1, F32, 0) == 0
    monkeypatch.setenv("DFFT_STFT_FUSED", "0")
    assert lib.dfft_stft1d_fused_applies(1024, F32) == 0 and lib.dfft_stft1d_scratch_bytes(1024, 2 ** 22 + 1, 1, F32, 0) == 256 << 20
    monkeypatch.delenv("DFFT_STFT_FUSED")
    assert lib.dfft_istft1d_scratch_bytes(1024, 2 ** 22, 1, F32) == 256 << 20 == lib.dfft_istft1d_scratch_bytes(1024, 4093, 2049, F32)
    # dfft_rconv1d_long
    assert lib.dfft_rconv1d_long_fused_applies(16384, F32) == 1 and lib.dfft_rconv1d_long_scratch_bytes(16000, 16384, 61, 4401, F32) == 256 << 20
    monkeypatch.setenv("DFFT_RCONV_LONG_FUSED", "0")
    assert lib.dfft_rconv1d_long_fused_applies(16384, F32) == 0
    monkeypatch.delenv("DFFT_RCONV_LONG_FUSED")
    # the refusals: 2^31 rows (R2 runs 2^31 - 1), 2^31 blocks (O2 runs 2^31 - 1), 2^31 frames (S3 runs 2^31 - 1)
    buf = np.zeros(64, dtype=np.float32)
    p, q = buf.ctypes.data, buf.ctypes.data + 128
    h = np.zeros(8, dtype=np.float32).ctypes.data
    for channels, batch in ((P31, 1), (1, P31), (2 ** 16, 2 ** 15), (3, 715827883)):
        assert lib.dfft_rconv1d(p, p, h, 2, 4, channels, batch, F32, 1, None) == _lib.EUNSUPPORTED and b"2^31 or more rows" in lib.dfft_last_error()
        assert lib.dfft_rconv1d_long(p, p, h, 16000, 16384, channels, batch, F32, 1, None) == _lib.EUNSUPPORTED
        assert lib.dfft_rconv1d_scratch_bytes(2, 4, channels, batch, F32) == 0 == lib.dfft_rconv1d_long_scratch_bytes(16000, 16384, channels, batch, F32)
    assert lib.dfft_rconv1d_os(p, q, h, 3 * P31, 3 * P31, 4, 1, 1, 1, F32, 0, None) == _lib.EUNSUPPORTED
    assert b"2^31 or more items" in lib.dfft_last_error()
    assert lib.dfft_rconv1d_os(p, q, h, 3 * P31 - 2, 3 * P31 - 2, 4, 1, 1, 1, F32, 0, None) == _lib.EUNSUPPORTED       # a ragged last block counts
    assert lib.dfft_rconv1d_os(p, q, h, 768 * 2 ** 20, 768 * 2 ** 20, 1024, 256, 2 ** 6, 2 ** 5, F32, 0, None) == _lib.EUNSUPPORTED
    assert lib.dfft_stft1d(p, q, h, 2 * P31 + 2, 4, 2, 0, P31, 1, F32, 0, 1, 1.0, None) == _lib.EUNSUPPORTED
    assert b"2^31 or more items" in lib.dfft_last_error()
    assert lib.dfft_stft1d(p, q, h, 2 ** 20, 1024, 256, 0, 4093, 524689, F32, 0, 0, 1.0, None) == _lib.EUNSUPPORTED   # 4093 * 524 689 = 2^31 + 429
    assert lib.dfft_istft1d(q, p, h, h + 16, 2 * P31 + 2, 4, 2, 0, P31, 1, F32, None) == _lib.EUNSUPPORTED
    assert lib.dfft_stft1d_scratch_bytes(4, P31, 1, F32, 1) == 0 == lib.dfft_istft1d_scratch_bytes(4, P31, 1, F32)
    assert not buf.any()
    if lib.dfft_device_count() == 0:
        # just under each guard the call is accepted: made-up, disjoint addresses, which only a machine without a device may be handed
        a, b, c = 1 << 44, 1 << 46, 1 << 42
        assert lib.dfft_rconv1d(a, a, c, 2, 4, P31 - 1, 1, F32, 1, None) == _lib.ENOGPU
        assert lib.dfft_rconv1d_os(a, b, c, 3 * (P31 - 1), 3 * (P31 - 1), 4, 1, 1, 1, F32, 0, None) == _lib.ENOGPU
        assert lib.dfft_stft1d(a, b, c, 2 * P31, 4, 2, 0, P31 - 1, 1, F32, 0, 1, 1.0, None) == _lib.ENOGPU
        assert lib.dfft_istft1d(b, a, c, c + 4096, 2 * P31, 4, 2, 0, P31 - 1, 1, F32, None) == _lib.ENOGPU
