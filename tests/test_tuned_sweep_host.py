"""The tuned-length sweep, host side (no GPU): tests/tuned_sweep.py against the source and the cross-compiled library.

  * coverage: per family, the swept lengths are exactly the entries of DFFT_PLAN_TABLE that the family's source instantiates -- the gate is
    read from the instantiation macro itself (kFusedMinM, odd n for the pair kernels, conv_fused_n), so a new X(...) line, a new gate or
    a new family cannot land without the sweep following;
  * routes: for every swept (family, length, precision, variant) the library's route predicate and its scratch-size query say what
    tuned_sweep.ROUTED says, and every half-length reaches both access widths of its kernels;
  * references: every longdouble reference of the sweep, against numpy's / scipy's float64 transform of the same input, stays under the cap
    the GPU result is held to (the float64 CPU transform is one more implementation of the same operation: a few eps, where a wrong
    reference is off by its whole norm), no reference line is identically zero, reflect padding has pad < n;
  * the whole case generation takes well under a minute (printed)."""
import time

import numpy as np
import pytest
import scipy.fft as sf

import accuracy_ref as A
import rconv1d_cases as RC
import rconv1d_os_cases as RCO
import stft_cases as SC
import tuned_sweep as TS

F64 = "f64"
# The caps of tests/test_gpu_tuned_sweep.py in fp64 (rconv1d / overlap-save: the BOUND of test_gpu_rconv1d.py / test_gpu_rconv1d_os.py,
# restated here because importing a GPU module from a host test would drag torch in; test_caps_are_the_gpu_modules_own compares them)
RCONV_BOUND = {"f64": 16.0, "f32": 26.0}
OSCONV_BOUND = {"f64": 5.5, "f32": 95.0}

# Entries of DFFT_PLAN_TABLE per family when the sweep was last reviewed: a new X(...) line fails here until whoever adds it has looked at
# the family's ROUTED table, its geometry exceptions and DESIGN.md's coverage table, and raised the count.
REVIEWED = {"real_rows": 49, "real_pair": 16, "real_cols": 49, "r2r": 49, "bluestein": 37, "rconv": 49, "osconv": 49, "stft": 49}


def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def _no_route_switch(monkeypatch):
    for name in ("DFFT_R2R_FUSED", "DFFT_RCONV_FUSED", "DFFT_STFT_FUSED", "DFFT_BLUESTEIN_FUSED"):
        monkeypatch.delenv(name, raising=False)


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------
def coverage_problems(lengths):
    """What separates the sweep tables from the instantiations of a plan table with these lengths (empty: nothing)"""
    problems = []
    for family in TS.FAMILIES:
        swept = set(TS.LENGTHS[family]) | (set(TS.BLUESTEIN_UNREACHABLE) if family == "bluestein" else set())
        built = set(TS.instantiated(family, lengths))
        if swept != built:
            problems.append((family, "instantiated but not swept", sorted(built - swept), "swept but not instantiated", sorted(swept - built)))
        if len(built) != REVIEWED[family]:
            problems.append((family, "entries", len(built), "reviewed", REVIEWED[family]))
    return problems


def test_every_instantiated_length_is_swept():
    assert len(TS.PLAN) == len(set(TS.PLAN)) == 49
    assert coverage_problems(TS.PLAN) == []
    for family in TS.FAMILIES:
        assert len(TS.LENGTHS[family]) == len(set(TS.LENGTHS[family]))
    # the gates as the sweep states them
    assert TS.source_constant("kFusedMinM", "dfft_bluestein.hip") == TS.BLUESTEIN_MIN_M
    assert TS.source_constant("kBluesteinFusedMaxLength", "dfft_bluestein.h") == TS.BLUESTEIN_MAX_N
    assert TS.instantiation_gate("real_pair") == "N % 2 == 1" and TS.instantiation_gate("bluestein") == "N >= kFusedMinM"
    # the fused X stage of the filter plans is not swept here (the conv modules run every one of its lengths), but its gate reads the same way
    assert TS.instantiated("conv_x") == TS.instantiated("conv_x_multi") == TS.conv_fused_lengths()
    assert set(TS.conv_fused_lengths()) <= set(TS.PLAN) and len(TS.conv_fused_lengths()) == 7


def test_a_plan_entry_without_a_sweep_entry_is_caught():
    """A plan table with one more line than the sweep's: every family that would instantiate it reports it."""
    text = (TS.CSRC / "dfft_plans.h").read_text().replace("    X(2401, 11, 7, 7, 7, 7, 7)", "    X(2401, 11, 7, 7, 7, 7, 7) \\\n    X(3087, 11, 7, 7, 7, 7, 3, 3)")
    lengths = TS.plan_lengths(text)
    assert lengths == sorted(TS.PLAN + [3087])
    problems = coverage_problems(lengths)
    named = {p[0] for p in problems if p[1] == "instantiated but not swept" and p[2] == [3087]}
    assert named == set(TS.FAMILIES), problems


def test_bluestein_lengths_against_the_library():
    lib = _lib()
    reach = {}
    for n in range(2, TS.BLUESTEIN_MAX_N + 1):
        kind3 = lib.dfft_length_kind(n) == 3
        assert kind3 == (not TS.seven_smooth(n)), n
        if kind3:
            assert lib.dfft_bluestein_length(n) == TS.bluestein_padded(n), n
            reach[int(lib.dfft_bluestein_length(n))] = n
    assert reach == TS.BLUESTEIN_N
    assert lib.dfft_bluestein_fused_applies(TS.BLUESTEIN_MAX_N + 5, 1) == 0 and lib.dfft_length_kind(TS.BLUESTEIN_MAX_N + 5) == 3   # 2053
    tuned = [m for m in TS.PLAN if m >= TS.BLUESTEIN_MIN_M]
    assert sorted(set(reach) | set(TS.BLUESTEIN_UNREACHABLE)) == tuned and not set(reach) & set(TS.BLUESTEIN_UNREACHABLE)
    assert len(reach) == 32


# ---- routes -----------------------------------------------------------------------------------------------------------------------------
def _swept_variants():
    """Every (family, length, prec, variant...) the GPU module runs -> (predicate value, scratch bytes) of the library"""
    lib = _lib()
    for prec in TS.PRECS:
        code = TS.CODE[prec]
        for M in TS.LENGTHS["real_rows"]:
            yield ("real_rows", M, prec), (lib.dfft_real_form(2 * M) == 1, 0)
        for n in TS.LENGTHS["real_pair"]:
            yield ("real_pair", n, prec), (lib.dfft_real_form(n) == 2, 0)
        for n in TS.LENGTHS["real_cols"]:
            for s in TS.real_cols_s(n):
                yield ("real_cols", n, prec, s), (lib.dfft_rfft_cols_fused_applies(n, s, code), lib.dfft_rfft1d_strided_scratch_bytes(n, s, 2, code))
        for n in TS.LENGTHS["r2r"]:
            for kind, three in TS.R2R_THREE.items():
                for form, s in TS.R2R_FORMS.items():
                    vec = int(form == "cols_vec")
                    got = (lib.dfft_r2r_fused_applies(n, s, code, TS.R2R_CODE[kind], vec),
                           lib.dfft_r2r1d_strided_scratch_bytes(n, s, 2, code, TS.R2R_CODE[kind], vec))
                    yield ("r2r", n, prec, three, form), got
        for M in TS.LENGTHS["bluestein"]:
            n = TS.BLUESTEIN_N[M]
            for s, batch in ((1, 3), (3, 2)):
                assert lib.dfft_bluestein_fused_applies(n, s) == 1 and lib.dfft_fft1d_any_scratch_bytes(n, s, batch, code) == 0, (M, n, s)
            yield ("bluestein", M, prec), (1, 0)
        for M in TS.LENGTHS["rconv"]:
            for n, kind, batch in TS.rconv_cases(M):
                got = (lib.dfft_rconv1d_fused_applies(n, 2 * M, code, TS.FILTER_CODE[kind], int(n % 2 == 0)),
                       lib.dfft_rconv1d_scratch_bytes(n, 2 * M, TS.RCONV_CHANNELS, batch, code))
                yield ("rconv", M, prec), got
        for M in TS.LENGTHS["osconv"]:
            for d, n, n_out, channels, batch, kind in TS.osconv_cases(M):
                yield ("osconv", M, prec), (lib.dfft_rconv1d_os_fused_applies(2 * M, code), lib.dfft_rconv1d_os_scratch_bytes(n_out, 2 * M, d, channels, batch, code))
        for M in TS.LENGTHS["stft"]:
            for (_, hop, pad, n, _), mode, kind in TS.stft_cases(M):
                frames = SC.frames_of(n, 2 * M, hop, pad)
                assert frames == lib.dfft_stft1d_frames(n, 2 * M, hop, pad) >= 1
                yield ("stft", M, prec), (lib.dfft_stft1d_fused_applies(2 * M, code), lib.dfft_stft1d_scratch_bytes(2 * M, frames, SC.ROWS, code, SC.KIND_CODE[kind]))


def test_routes_and_scratch_agree_with_the_library():
    from distributedfft_amd import _lib as L
    assert (L.R2R_DCT2, L.R2R_DCT3, L.R2R_DST2, L.R2R_DST3) == tuple(TS.R2R_CODE[k] for k in A.R2R_KINDS)
    assert (L.F64, L.F32) == (TS.CODE["f64"], TS.CODE["f32"]) and (L.FILTER_COMPLEX, L.FILTER_REAL) == (TS.FILTER_CODE["complex"], TS.FILTER_CODE["real"])
    seen = {f: set() for f in TS.FAMILIES}
    count = 0
    for key, (applies, scratch) in _swept_variants():
        family, length, prec = key[:3]
        fused = TS.route(family, length, prec, *key[3:]) == "fused"
        assert bool(applies) == fused, (key, applies)
        if family not in ("real_rows", "real_pair"):       # their entry point has no scratch query: one launch at every tuned length
            assert (scratch == 0) == fused, (key, scratch)
        seen[family].add((length, prec) + tuple(key[3:]))
        count += 1
    print(f"tuned sweep: {count} (family, length, precision, variant, shape) route checks")
    for family in TS.FAMILIES:
        assert TS.ROUTED[family] <= seen[family], (family, "ROUTED names what the sweep does not run", TS.ROUTED[family] - seen[family])
    # multi_pass_faster at fp32 n = 2048: both sides are run
    assert TS.route("real_cols", 2048, "f32", 40) == "fused" and TS.route("real_cols", 2048, "f32", 24) == "composed"
    # a neighbouring fused length for the composed route under the switch
    for family, (_, n) in TS.COMPOSED_NEIGHBOUR.items():
        assert n in TS.LENGTHS[family] and not any(r[0] == n for r in TS.ROUTED[family]), (family, n)


def test_every_half_length_reaches_both_access_widths():
    for M in TS.PLAN:
        ns = TS.rconv_n_values(M)
        assert ns[0] == 2 * M and ns[1] == (M - 1 if M > 2 else 1) and any(n % 2 for n in ns) and any(n % 2 == 0 for n in ns), (M, ns)
        assert all(1 <= n <= 2 * M for n in ns) and (1 not in ns or M <= 3)
        shapes = TS.osconv_shapes(M)
        assert shapes[0] == (M, 2 * M + M // 2), (M, shapes)
        assert any(TS.osconv_vec(d, n) for d, n in shapes) and any(d % 2 for d, n in shapes), (M, shapes)
        for d, n in shapes:
            S = 2 * M - d
            assert 0 <= d < 2 * M and n >= 1 and RCO.blocks(n, 2 * M, d) >= 2 and (M == 2 or n % S), (M, d, n)   # a ragged last block
        st = TS.stft_shapes(M)
        assert st[0] == SC._base(M)
        assert any(TS.stft_vec(c) for c in st) and any(c[1] % 2 for c in st), (M, st)
        for c in st:
            assert all(SC.usable(c, mode) for mode in SC.MODES) and c[1] >= 1 and 0 <= c[2] < 2 * M, c
    G = [RC.rows_per_group(M) for M in TS.PLAN]
    assert max(G) > TS.ROWS and min(G) == 1          # five rows: ragged thread groups and one-row workgroups both occur


def test_caps_are_the_gpu_modules_own():
    """BOUND of test_gpu_rconv1d.py / test_gpu_rconv1d_os.py, read from their source (importing them needs nothing but would run their
    module code; the text is enough)"""
    import re
    here = TS.ROOT / "tests"
    for file, want in (("test_gpu_rconv1d.py", RCONV_BOUND), ("test_gpu_rconv1d_os.py", OSCONV_BOUND)):
        m = re.search(r'^BOUND = \{"f64": ([\d.]+), "f32": ([\d.]+)\}', (here / file).read_text(), re.M)
        assert {"f64": float(m.group(1)), "f32": float(m.group(2))} == want, file


# ---- references -------------------------------------------------------------------------------------------------------------------------
WORST = {}


def _hold(family, value, cap, what):
    if value > WORST.get(family, (-1.0, ""))[0]:
        WORST[family] = (value, what)
    assert value <= cap, (family, what, value, cap)


def _r2r_f64(x, kind):
    return {"dct2": lambda v: sf.dct(v, 2, axis=1), "dct3": lambda v: sf.dct(v, 3, axis=1), "dst2": lambda v: sf.dst(v, 2, axis=1),
            "dst3": lambda v: sf.dst(v, 3, axis=1)}[kind](x)


def _real_refs(family, n, x, F, X, b, axis=1):
    cap = A.CEILING["real"][F64]
    _hold(family, A.nu(np.fft.rfft(x, axis=axis), F, n, F64, (axis,)), cap, f"rfft n={n}")
    _hold(family, A.nu(np.fft.irfft(X, n, axis=axis) * n, b, n, F64, (axis,)), cap, f"irfft n={n}")


def test_references_against_float64_transforms_and_generation_time():
    t0 = time.perf_counter()
    cases = 0
    for M in TS.LENGTHS["real_rows"]:
        _real_refs("real_rows", 2 * M, *TS.real_rows_case(2 * M, True))
        cases += 1
    for n in TS.LENGTHS["real_pair"]:
        _real_refs("real_pair", n, *TS.real_rows_case(n, False))
        cases += 1
    for n in TS.LENGTHS["real_cols"]:
        for s in TS.real_cols_s(n):
            _real_refs("real_cols", n, *TS.real_cols_case(n, s))
            cases += 1
    for n in TS.LENGTHS["r2r"]:
        for s in TS.R2R_FORMS.values():
            case = TS.r2r_case(n, s)
            for kind, ref in zip(A.R2R_KINDS, case[1:]):
                _hold("r2r", A.nu(_r2r_f64(case[0], kind), ref, n, F64, (1,)), A.CEILING["r2r"][F64], f"{kind} n={n} s={s}")
            cases += 1
    for M in TS.LENGTHS["bluestein"]:
        n, both = TS.bluestein_cases(M)
        for shape, axis, x, F in both:
            cap = A.CEILING["bluestein"][F64]
            _hold("bluestein", A.nu(np.fft.fft(x, axis=axis), F, n, F64, (axis,)), cap, f"fwd n={n} {shape}")
            _hold("bluestein", A.nu(np.fft.ifft(x, axis=axis) * n, A.reverse_bins(F, [axis]), n, F64, (axis,)), cap, f"bwd n={n} {shape}")
            cases += 1
    for M in TS.LENGTHS["rconv"]:
        m = 2 * M
        for n, kind, batch in TS.rconv_cases(M):
            x, H, ref = RC.case(M, n, TS.RCONV_CHANNELS, batch, kind)
            Hr = H[np.arange(x.shape[0]) % TS.RCONV_CHANNELS]
            got = np.fft.irfft(np.fft.rfft(x, m, axis=1) * Hr, m, axis=1)[:, :n]
            _hold("rconv", RC.nu_rows(got, ref, m, F64), RCONV_BOUND[F64], f"M={M} n={n} {kind}")
            cases += 1
    for M in TS.LENGTHS["osconv"]:
        m = 2 * M
        for d, n, n_out, channels, batch, kind in TS.osconv_cases(M):
            x, H, ref = RCO.case(M, d, n, n_out, channels, batch, kind)
            Hr = H[np.arange(x.shape[0]) % channels][:, None, :]
            cb = np.fft.irfft(np.fft.rfft(RCO.gather(x, m, d, n_out), axis=2) * Hr, m, axis=2)
            got = cb[:, :, d:].reshape(x.shape[0], -1)[:, :n_out]
            _hold("osconv", RCO.nu_rows(got, ref, m, F64), OSCONV_BOUND[F64], f"M={M} d={d} n={n} {kind}")
            cases += 1
    for M in TS.LENGTHS["stft"]:
        m = 2 * M
        for shape in TS.stft_shapes(M):
            _, hop, pad, n, wkind = shape
            for mode in SC.MODES:
                assert SC.usable(shape, mode)
                x, win, frames, ref = SC.forward_case(M, hop, pad, n, wkind, mode)
                got = np.fft.rfft(SC.gather(x, m, hop, pad, frames, mode) * win, axis=2)
                cap = A.CEILING["real"][F64]
                _hold("stft", SC.nu_frames(got, ref, m, F64), cap, f"M={M} hop={hop} pad={pad} {mode} complex")
                _hold("stft", SC.nu_frames(SC.power(got), SC.power(ref), m, F64), 2 * cap, f"M={M} hop={hop} pad={pad} {mode} power")
                cases += 1
    elapsed = time.perf_counter() - t0
    for family, (value, what) in sorted(WORST.items()):
        print(f"tuned sweep reference check, float64 CPU transform against longdouble, worst {family}: nu {value:.3f}  ({what})")
    print(f"tuned sweep: {cases} cases generated and checked in {elapsed:.1f} s")
    assert elapsed < 40.0, elapsed
