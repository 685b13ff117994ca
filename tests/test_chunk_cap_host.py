"""No GPU: the chunk cap DFFT_SCRATCH_CHUNK_BYTES through the C ABI.  Every dfft_*_scratch_bytes query of a composed route equals the
Python mirror of its chunk rule (tests/chunk_seams.py, tests/large_extent.py, tests/rxspec1d_long_cases.py) under a cap of one unit, 2.5
units, exactly three units, one byte and more than the whole problem; unset answers like 268435456; the family names of the STFT and
of the cross-spectral density win over the general one, which now moves them too; the fused routes' leases do not follow the cap except
where the long fused routes chunk their pass-A rows; and the table of tests/test_gpu_chunk_seams.py covers what it claims."""
import pytest

import accuracy_ref as A
import call_mix as CM
import chunk_seams as S
import large_extent as LE
import rxspec1d_long_cases as XL

ENV = S.ENV
F64, F32 = 0, 1
FAMILY_ENVS = ("DFFT_STFT_CHUNK_BYTES", "DFFT_RCSD_CHUNK_BYTES")


def _lib():
    from distributedfft_amd import _lib as L
    return L.load()


@pytest.fixture(autouse=True)
def _clean(monkeypatch):
    for name in (ENV,) + FAMILY_ENVS:
        monkeypatch.delenv(name, raising=False)


# ---- the queries against the mirrors -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seam", S.SEAMS, ids=repr)
def test_query_equals_the_mirror_under_every_cap(seam):
    lib = _lib()
    u, units = seam.unit_bytes, seam.units
    assert seam.need(lib) == seam.lease() > 0, (seam, "no cap")
    assert seam.chunks() == [units], (seam, "the problem is one chunk at 256 MiB")
    caps = dict(seam.host_caps(), **{label: seam.cap_bytes(label) for label in seam.caps})
    for label, cap in caps.items():
        assert seam.need(lib, cap) == seam.lease(cap) > 0, (seam, label, cap)
    # what the caps mean, by the rule "never fewer than one unit"
    if seam.whole_pairs:    # never fewer than a pair of rows, and whole pairs
        assert seam.per_chunk(u) == seam.per_chunk(1) == seam.per_chunk(5 * u // 2) == seam.per_chunk(3 * u) == 2 and seam.per_chunk(4 * u) == 4
        assert seam.per_chunk(caps["whole"]) == units and seam.lease(caps["whole"]) == seam.lease() and seam.lease(u) < seam.lease(4 * u) < seam.lease()
        return
    assert seam.per_chunk(u) == seam.per_chunk(1) == 1 and seam.per_chunk(5 * u // 2) == min(2, units) and seam.per_chunk(3 * u) == min(3, units)
    assert seam.per_chunk(caps["whole"]) == units and seam.lease(caps["whole"]) == seam.lease() and caps["whole"] > units * u
    assert seam.per_chunk(3 * u - 1) == min(2, units)
    if units > 3:
        assert seam.lease(u) < seam.lease(3 * u) < seam.lease()


@pytest.mark.parametrize("seam", S.SEAMS, ids=repr)
def test_unset_empty_and_non_positive_mean_256_mib(seam, monkeypatch):
    lib = _lib()
    want = seam.need(lib)
    for text in ("268435456", "", "0", "-5", "x"):
        monkeypatch.setenv(ENV, text)
        with CM.env(seam.op.switches):
            assert seam.op._need(lib) == want, (seam, text)


def test_a_cap_between_unit_counts_rounds_down_and_a_large_problem_follows_it(monkeypatch):
    """The cap in bytes on problems that do fill it: rows of dfft_rconv1d (m = 72, untuned half) under 1 MiB and under the default"""
    lib = _lib()
    for code, cs in ((F64, 16), (F32, 8)):
        rb = 37 * cs + 72 * cs // 2
        monkeypatch.delenv(ENV, raising=False)
        assert lib.dfft_rconv1d_scratch_bytes(70, 72, 61, 10 ** 6, code) == (256 << 20) // rb * rb
        monkeypatch.setenv(ENV, str(1 << 20))
        assert lib.dfft_rconv1d_scratch_bytes(70, 72, 61, 10 ** 6, code) == (1 << 20) // rb * rb
        assert lib.dfft_rconv1d_scratch_bytes(70, 72, 3, 5, code) == 15 * rb        # fewer rows than fit


# ---- precedence ------------------------------------------------------------------------------------------------------------------------------
def test_family_names_win_and_the_general_name_moves_stft_and_rcsd(monkeypatch):
    lib = _lib()
    monkeypatch.setenv("DFFT_STFT_FUSED", "0")
    monkeypatch.setenv("DFFT_RCSD_FUSED", "0")
    for prec in A.PRECS:
        code = CM.CODE[prec]
        m, frames, rows = 128, 13, 3
        queries = (
            ("DFFT_STFT_CHUNK_BYTES", CM.stft_item_bytes(m, prec, "complex"), lambda: lib.dfft_stft1d_scratch_bytes(m, frames, rows, code, 0)),
            ("DFFT_STFT_CHUNK_BYTES", CM.stft_item_bytes(m, prec, "power"), lambda: lib.dfft_stft1d_scratch_bytes(m, frames, rows, code, 1)),
            ("DFFT_RCSD_CHUNK_BYTES", CM.rcsd_item_bytes(m, prec), lambda: lib.dfft_rcsd1d_scratch_bytes(m, frames, rows, code, 0)),
        )
        for family, ib, query in queries:
            items = frames * rows
            for name in (ENV, family):
                monkeypatch.delenv(name, raising=False)
            assert query() == items * ib
            monkeypatch.setenv(ENV, str(5 * ib))                 # the general name alone
            assert query() == 5 * ib
            monkeypatch.setenv(family, str(2 * ib))              # the family's own name wins, smaller ...
            assert query() == 2 * ib
            monkeypatch.setenv(family, str(7 * ib))              # ... or larger
            assert query() == 7 * ib
            monkeypatch.setenv(family, "0")                      # not positive: as if unset, so the general name again
            assert query() == 5 * ib
            monkeypatch.delenv(ENV)
            assert query() == items * ib
            monkeypatch.setenv(family, str(2 * ib))
            assert query() == 2 * ib
            monkeypatch.delenv(family)
        # a family name does not reach the other routes
        monkeypatch.setenv("DFFT_STFT_CHUNK_BYTES", "1")
        monkeypatch.setenv("DFFT_RCSD_CHUNK_BYTES", "1")
        seam = next(s for s in S.SEAMS if s.family == "rconv1d" and s.op.prec == prec)
        with CM.env(seam.op.switches):
            assert seam.op._need(lib) == seam.lease()
        monkeypatch.delenv("DFFT_STFT_CHUNK_BYTES")
        monkeypatch.delenv("DFFT_RCSD_CHUNK_BYTES")
    # the inverse STFT keeps its own minimum (a chunk never holds fewer frames than overlap one sample) under either name
    monkeypatch.setenv("DFFT_STFT_CHUNK_BYTES", "1")
    floor = lib.dfft_istft1d_scratch_bytes(128, 9, 3, F64)
    monkeypatch.delenv("DFFT_STFT_CHUNK_BYTES")
    whole = lib.dfft_istft1d_scratch_bytes(128, 9, 3, F64)
    monkeypatch.setenv(ENV, "1")
    assert 0 < floor == lib.dfft_istft1d_scratch_bytes(128, 9, 3, F64) < whole and floor % CM.istft_item_bytes(128, "f64", True) == 0


# ---- fused routes ----------------------------------------------------------------------------------------------------------------------------
def test_fused_leases_do_not_follow_the_cap_except_the_long_pass_a_rows(monkeypatch):
    lib = _lib()
    for prec in A.PRECS:
        code, cs = CM.CODE[prec], CM.ESIZE[prec]
        batch = CM.XC.batches(CM.RXSPEC_M, CM.RXSPEC_CHANNELS)[1]
        frames = CM.WC.frame_counts(CM.RCSD_M, CM.RCSD_ROWS)[1]
        short = (lambda: lib.dfft_rconv1d_scratch_bytes(128, 128, 3, 40, code),                       # one launch: nothing
                 lambda: lib.dfft_rconv1d_os_scratch_bytes(272, 128, 32, 3, 2, code),
                 lambda: lib.dfft_rxspec1d_scratch_bytes(63, 128, CM.RXSPEC_CHANNELS, batch, code),   # the slices' partial sums
                 lambda: lib.dfft_rxspec1d_slices(128, CM.RXSPEC_CHANNELS, batch, code),
                 lambda: lib.dfft_rcsd1d_scratch_bytes(128, frames, CM.RCSD_ROWS, code, 0),
                 lambda: lib.dfft_stft1d_scratch_bytes(128, 13, 3, code, 0),
                 lambda: lib.dfft_rfft1d_scratch_bytes(243, 7, code, +1),                             # the one-launch pairs
                 lambda: lib.dfft_rfft1d_strided_scratch_bytes(243, 6, 5, code),
                 lambda: lib.dfft_r2r1d_strided_scratch_bytes(243, 6, 5, code, 0, 1),
                 lambda: lib.dfft_fft1d_any_scratch_bytes(97, 3, 5, code),
                 lambda: lib.dfft_fft1d_any_scratch_bytes(8192, 3, 5, code))                          # four-step: as much as its data
        monkeypatch.delenv(ENV, raising=False)
        base = [q() for q in short]
        assert base[0] == base[1] == base[5] == base[6] == base[7] == base[8] == base[9] == 0 and base[2] > 0 and base[3] >= 2 and base[4] > 0
        assert base[10] == 5 * 8192 * 3 * cs
        monkeypatch.setenv(ENV, "1")
        assert [q() for q in short] == base
        # the long fused routes chunk their pass-A rows by the cap, and the slice count follows the chunk's rows
        m, channels = 16384, 1
        lb = XL.ragged_batch(m)
        assert lib.dfft_rconv1d_long_fused_applies(m, code) == 1 == lib.dfft_rxspec1d_long_fused_applies(m, code)
        monkeypatch.delenv(ENV)
        assert lib.dfft_rxspec1d_long_slices(m, channels, lb, code) == XL.call_slices(m, channels, lb, prec) >= 2
        assert lib.dfft_rconv1d_long_scratch_bytes(m, m, channels, lb, code) == lb * (m // 2) * cs
        for rows in (1, 9, lb - 1):
            cap = rows * 2 * (m // 2) * cs
            monkeypatch.setenv(ENV, str(cap))
            assert XL.chunk_rows(m, prec, lb, cap) == rows
            assert lib.dfft_rxspec1d_long_slices(m, channels, lb, code) == XL.slices_rule(m, channels, rows) == XL.call_slices(m, channels, lb, prec, cap)
            assert lib.dfft_rxspec1d_long_scratch_bytes(m, m, channels, lb, code) == XL.scratch_bytes(m, channels, lb, prec, cap)
            assert lib.dfft_rconv1d_long_scratch_bytes(m, m, channels, lb, code) == min(lb, 2 * rows) * (m // 2) * cs
            monkeypatch.delenv(ENV)
        assert XL.slices_rule(m, channels, 1) == 1 < XL.slices_rule(m, channels, lb)


# ---- the table --------------------------------------------------------------------------------------------------------------------------------
def test_the_table_covers_what_it_claims():
    lib = _lib()
    by_family = {f: [s for s in S.SEAMS if s.family == f] for f in S.FAMILIES}
    for family, seams in by_family.items():
        assert {s.op.prec for s in seams} == set(A.PRECS), family
    for s in S.SEAMS:
        with CM.env(s.op.switches):
            assert s.op._need(lib) > 0, (s, "the seam does not take a leasing route")
        runs = [s.chunks(s.cap_bytes(label)) for label in s.caps]
        # three chunks or more under every cap -- but for the seams of four pairs, which the two-pair cap cuts in two (three whole
        # pairs and a half-empty one are four units); their one-pair cap gives four
        for label, chunks in zip(s.caps, runs):
            assert len(chunks) >= 3 or (s.units == 4 and s.caps[label] == 2 and chunks == [2, 2]), (s, label, chunks)
        assert max(len(c) for c in runs) >= 3 and any(c[-1] < c[0] or len(c) == s.units for c in runs), (s, runs)
        assert s.op.out_bytes() <= 2 << 20 and s.lease() <= 8 << 20, (s, "a few MiB at the most (the largest: n = 4099, s = 5, batch 5 in fp64)")
        assert s.exact == (s.sums is None)
    n, channels, batch = S.SHAPE
    rows = n and channels * batch
    four = LE.chunk_sizes(rows, 4)
    assert four == [4, 4, 4, 4, 4, 1] and {(4 * i) % channels for i in range(len(four))} == {0, 1, 2}      # every phase of row0 % channels
    os_items = [s for s in by_family["rconv1d_os"]][0]
    starts = [5 * i for i in range(len(os_items.chunks(os_items.cap_bytes("5-items"))))]
    assert any(i % 4 for i in starts) and any(i // 4 % S.OS_SHAPE[0] for i in starts)                     # inside a row, across channels
    fused_long = [s for s in by_family["rxspec1d_long"] if not s.exact]
    assert fused_long and all(s.chunks(s.cap_bytes("3-rows")) == [3, 3, 3] and s.chunks(s.cap_bytes("4-rows")) == [4, 4, 1] for s in fused_long)
    assert all(lib.dfft_rxspec1d_long_fused_applies(S.LONG_M, c) == 1 == lib.dfft_rconv1d_long_fused_applies(S.LONG_M, c) for c in (F64, F32))
    assert S.bluestein_M(1009) == 2048 and S.bluestein_M(4099) > 4096 and S.bluestein_M(375) == 0
    # Bluestein chunks nest inside a pair / r2r chunk: one padded transform is larger than one unit of the outer rule
    for s in S.SEAMS:
        if s.family in ("real-rows", "r2r") and "1009" in s.name and s.op.switches:
            inner = LE.bluestein_per_transform_bytes(2048, 1, s.op.prec)
            assert inner > s.unit_bytes and LE.bluestein_chunk(2048, 1, 2, s.op.prec, 2 * s.unit_bytes) == 1


@pytest.mark.parametrize("seam", [s for s in S.SEAMS if s.op.name not in CM.BY_NAME], ids=repr)
def test_cpu_model_of_the_reference_is_under_the_bound(seam):
    """As tests/test_call_mix_host.py holds its registry: the same-precision CPU model of each seam's reference is within the family's
    bound, so the reference does not eat the margin the GPU test relies on"""
    if seam.inplace:
        return      # the same op as its out-of-place twin
    op = seam.op
    inputs, shape, dtype, ref = op.case
    got = op.model()
    assert got.shape == shape == ref.shape and got.dtype == dtype
    value = op.measure(got)
    print(f"chunk seam {seam}: CPU model nu {value:.3f} (bound {op.bound}: {op.bound_name})")
    assert value <= op.bound, (seam, value, op.bound)
