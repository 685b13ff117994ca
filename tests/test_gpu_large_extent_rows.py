"""-m gpu: the 1-D real convolution and STFT entry points (dfft_rconv1d, dfft_rconv1d_os, dfft_stft1d, dfft_istft1d, dfft_rconv1d_long) at
extents whose element offsets pass 2^31 and 2^32 and whose item counts sit just under the 2^31 refusals -- the sibling of
tests/test_gpu_large_extent.py, whose all_shapes() covers the tensors of this module and whose rules it follows: tiled inputs, every line
checked on the device, the base lines against longdouble references under the bound the family's own GPU module asserts, a skip only
where the peak exceeds the free HBM.

Many independent rows (R, O3, L) are tensors [rows][n][1] of large_extent.run_case, row L holding base row L mod K and filtered by filter
row L mod K (channels = K; R2: channels = rows, filter row c = base filter c mod K).  A single long row (O1, O2, O4, S, I2) and the rows
of frames of I1 are large_extent.Band cases: lines of S = m - d samples (overlap-save), of hop samples and of m/2 + 1 bins (STFT and its
inverse), whose neighbours interact.  DESIGN.md section 7k lists the guard each case brackets."""
import numpy as np
import pytest

import accuracy_ref as A
import large_extent as LE
import rconv1d_cases as RC
import rconv1d_long_cases as LC
import rconv1d_os_cases as OC
import stft_cases as SC

pytestmark = pytest.mark.gpu
CODE = {"f64": 0, "f32": 1}
KIND = {"complex": 0, "real": 1}
RB = {"f64": 8, "f32": 4}                       # one real
P31, P32 = 1 << 31, 1 << 32


def register_bounds():
    """The bounds the families' own GPU modules assert (no new tolerance): nu per line with n_eff = m"""
    import test_gpu_rconv1d as TR
    import test_gpu_rconv1d_os as TO
    import test_gpu_stft as TS
    LE.EXTRA_BOUND.update({"rconv1d": TR.BOUND, "rconv1d_os": TO.BOUND, "rconv1d_long": LC.BOUND, "stft": TS.CAP, "istft": TS.CAP,
                           "stft-power": {p: 2.0 * TS.CAP[p] for p in TS.CAP}})   # the power spectrogram: twice the cap (test_gpu_stft.py)


# ---- the case tables -----------------------------------------------------------------------------------------------------------------------
# dfft_rconv1d: (id, M, n, filter kind, prec, fewest rows, in place, composed?, channels = rows?).  rows = the next multiple of K (channels = K).
#   R1 row bases past 2^32 reals; R2 the last iterations of the unsigned row loop, 2^31 - 1 rows, one under the refusal (2^31 - 1 is
#   prime, so no K divides it: channels = rows, batch = 1, and filter row c holds base filter c mod K); R3 row0 * n across 134 scratch
#   chunks of the composed route (M = 36 has no plan); R4 fp64 byte offsets past 2^34
RCONV = [
    ("R1-fused-rows*n-over-2^32", 512, 1000, "complex", "f32", P32 // 1000 + 1, False, False, False),
    ("R2-fused-2^31-1-rows", 2, 2, "real", "f32", P31 - 1, True, False, True),
    ("R3-composed-rows*n-over-2^32", 36, 70, "complex", "f32", P32 // 70 + 1, True, True, False),
    ("R4-fused-f64-rows*n-over-2^31", 256, 512, "real", "f64", P31 // 512 + 1, False, False, False),
]
# dfft_rconv1d_os, many rows: (id, M, d, n, filter kind, prec, fewest rows).  O3: row * n + s0 and row * n_out + t0 past 2^32
OS_ROWS = [("O3-rows*n-over-2^32", 512, 256, 65538, "complex", "f32", P32 // 65538 + 1)]
# dfft_rconv1d_long: (id, m, n, filter kind, prec, fewest rows, in place, composed?)
LONG = [
    ("L1-fused-rows*n-over-2^32", 16384, 16000, "complex", "f32", P32 // 16000 + 1, False, False),
    ("L2-composed-rows*n-over-2^32", 16384, 16000, "real", "f32", P32 // 16000 + 1, True, True),
]
# dfft_rconv1d_os, one row of `lines` lines of S = m - d samples (n = n_out = lines * S): (id, M, d, lines, filter kind, prec, fused?)
#   O1 two-real accesses, b * S past 2^32; O2 per-real accesses, 2^31 - 1 items: AT the largest accepted count (one more block is refused);
#   O4 the routed pair (M = 1536 in fp64 runs composed): gather and scatter across 193 chunks, past 2^31 fp64 reals
OS_BAND = [
    ("O1-one-row-n-over-2^32", 512, 256, P32 // 768 + 1, "complex", "f32", True),
    ("O2-one-row-2^31-1-items", 2, 1, P31 - 1, "complex", "f32", True),
    ("O4-one-row-f64-composed-n-over-2^31", 1536, 1024, P31 // 2048 + 1, "real", "f64", False),
]
# dfft_stft1d, one row of `lines` lines of hop samples, no centring: (id, M, hop, lines, output, prec, DFFT_STFT_FUSED=0?)
#   S1 frame bases past 2^32; S2 the overlapped window decode, 2^24 frames; S3 2^31 - 1 frames, AT the largest accepted count, and
#   it * (M + 1) past 2^32; S4 the composed route: it0 * (M + 1) past 2^31 over 65 536-frame chunks
STFT = [
    ("S1-fused-n-over-2^32", 512, 1024, P32 // 1024 + 1, "complex", "f32", False),
    ("S2-fused-hop-m/4-power", 512, 256, P32 // 256 + 4, "power", "f32", False),
    ("S3-fused-2^31-1-frames", 2, 2, P31, "power", "f32", False),
    ("S4-composed-n-over-2^32", 512, 1024, P32 // 1024 + 1, "complex", "f32", True),
]
# dfft_istft1d: (id, M, hop, rows, frames per row, prec); n = (frames - 1) hop + m per row.
#   I1: rows of 2^20 samples.  With hop = m / 4 the bins are 8 bytes for every output byte doubled: rows * n past 2^32 needs 64 GiB of bins
#   and 16 GiB of samples, over the cap of a case; so I1a keeps hop = m / 4 with rows * n past 2^31 (its bins pass 2^32 complex
#   elements) and I1b reaches rows * n past 2^32 with hop = m / 2.  I2: one row past 2^31 samples, cut into 65 536-frame chunks [t0, t1)
ISTFT = [
    ("I1a-rows-hop-m/4-bins-over-2^32", 512, 256, 2049, 4093, "f32"),
    ("I1b-rows-hop-m/2-rows*n-over-2^32", 512, 512, 4097, 2047, "f32"),
    ("I2-one-row-n-over-2^31", 512, 512, 1, P31 // 512, "f32"),
]


def _rows_k(fewest, shapes_of):
    """(K, rows): the first K whose multiple rows = ceil(fewest / K) K gives tensors that wrap_distinct accepts"""
    for K in LE.K_CANDIDATES:
        rows = -(-fewest // K) * K
        if all(LE.wrap_distinct(b, m, s, K, eb) for b, m, s, eb in shapes_of(rows)):
            return K, rows
    raise AssertionError("no K")


def rconv_plan(case):
    """-> (K, rows, channels, batch)"""
    _, M, n, kind, prec, fewest, _, _, per_row = case
    if per_row:      # channels = rows: the filter is a tiled tensor [rows][M + 1] as well
        hb = RB[prec] * (1 if kind == "real" else 2)
        K = LE.pick_k([(fewest, n, 1, RB[prec]), (fewest, M + 1, 1, hb)])
        return K, fewest, fewest, 1
    K, rows = _rows_k(fewest, lambda r: [(r, n, 1, RB[prec])])
    return K, rows, K, rows // K


def os_rows_plan(case):
    _, M, d, n, kind, prec, fewest = case
    K, rows = _rows_k(fewest, lambda r: [(r, n, 1, RB[prec])])
    return K, rows


def long_plan(case):
    _, m, n, kind, prec, fewest, _, _ = case
    K, rows = _rows_k(fewest, lambda r: [(r, n, 1, RB[prec])])
    return K, rows


def os_band(case):
    """-> (Band, lines of S samples in and out)"""
    _, M, d, lines, _, _, _ = case
    S = 2 * M - d
    return LE.Band(1, lines, lines, -(-d // S), 0), S


def stft_band(case):
    """-> (Band, p_in = hop, p_out = M + 1)"""
    _, M, hop, lines, _, _, _ = case
    qa = 2 * M // hop - 1
    return LE.Band(1, lines, lines - qa, 0, qa), hop, M + 1


def istft_band(case):
    """-> (Band, p_in = M + 1, p_out = hop)"""
    _, M, hop, rows, frames, _ = case
    qb = 2 * M // hop - 1
    return LE.Band(rows, frames, frames + qb, qb, 0), M + 1, hop


def shapes():
    """(what, batch, m, s, elem_bytes) of every tensor of this module in the tiled form of large_extent.wrap_distinct (line L = base
    line L mod K), for test_gpu_large_extent.all_shapes()"""
    out = []
    for case in RCONV:
        K, rows, channels, batch = rconv_plan(case)
        out.append((case[0], rows, case[2], 1, RB[case[4]]))
        if case[8]:
            out.append((case[0] + " filter", rows, case[1] + 1, 1, RB[case[4]] * (1 if case[3] == "real" else 2)))
    for case in OS_ROWS:
        out.append((case[0], os_rows_plan(case)[1], case[3], 1, RB[case[5]]))
    for case in LONG:
        out.append((case[0], long_plan(case)[1], case[2], 1, RB[case[4]]))
    for case in OS_BAND:
        band, S = os_band(case)
        out.append((case[0], band.lin, S, 1, RB[case[5]]))
    for case in STFT:
        band, hop, bins = stft_band(case)
        out += [(case[0] + " samples", band.lin, hop, 1, RB[case[5]]),
                (case[0] + " bins", band.lout, bins, 1, RB[case[5]] * (1 if case[4] == "power" else 2))]
    for case in ISTFT:
        band, bins, hop = istft_band(case)
        out.append((case[0] + " bins", band.rows * band.lin, bins, 1, 2 * RB[case[5]]))
        if band.rows == 1:
            out.append((case[0] + " samples", band.lout, hop, 1, RB[case[5]]))
    return out


def band_shapes():
    """(what, Band, p_in, p_out, input element bytes, output element bytes) of every Band case: large_extent.band_wrap_distinct covers the
    outputs whose rows interact (I1: the class of a line is not its index modulo K)"""
    out = []
    for case in OS_BAND:
        band, S = os_band(case)
        out.append((case[0], band, S, S, RB[case[5]], RB[case[5]]))
    for case in STFT:
        band, hop, bins = stft_band(case)
        out.append((case[0], band, hop, bins, RB[case[5]], RB[case[5]] * (1 if case[4] == "power" else 2)))
    for case in ISTFT:
        band, bins, hop = istft_band(case)
        out.append((case[0], band, bins, hop, 2 * RB[case[5]], RB[case[5]]))
    return out


# ---- base lines and references -----------------------------------------------------------------------------------------------------------------
def rconv_base(M, n, kind, K):
    """-> (x [K][n], H [K][M + 1], longdouble reference [K][n]): row j filtered by filter row j"""
    x = A.rand_real((K, n), 41000 + 16 * M + n)
    H = RC.make_filter(K, 2 * M, kind, 41001 + 16 * M + n)
    return x, H, RC.reference(x, H, 2 * M)


def os_rows_base(M, d, n, kind, K):
    x = A.rand_real((K, n), 42000 + 16 * M + d)
    H = RC.make_filter(K, 2 * M, kind, 42001 + 16 * M + d)
    return x, H, OC.reference(x, H, 2 * M, d, n)


def os_band_base(M, d, kind, K):
    """-> (lines [K][S], H [1][M + 1], small)"""
    m, S = 2 * M, 2 * M - d
    base = A.rand_real((K, S), 43000 + 16 * M + d)
    H = RC.make_filter(1, m, kind, 43001 + 16 * M + d)

    def small(ids):
        x = base[ids].reshape(1, -1)
        return OC.reference(x, H, m, d, x.shape[1]).reshape(-1, S)
    return base, H, small


def stft_base(M, hop, kind, K):
    """-> (lines [K][hop], window [m], small)"""
    m = 2 * M
    base = A.rand_real((K, hop), 44000 + 16 * M + hop)
    win = SC.window(m, "hann")

    def small(ids):
        x = base[ids].reshape(1, -1)
        X = SC.reference(x, win, m, hop, 0, SC.frames_of(x.shape[1], m, hop, 0), "zero")[0]
        return SC.power(X) if kind == "power" else X
    return base, win, small


def istft_envelope_lines(win, m, hop, frames):
    """1 / envelope of a row of `frames` frames as float32 values, in lines of hop samples [frames + m / hop - 1][hop]"""
    env = SC.envelope(win, m, hop, frames)
    assert env.min() > 0.009
    return (1 / env).astype(np.float32).astype(np.float64).reshape(-1, hop)


def istft_base(M, hop, K):
    """-> (frames [K][M + 1], window [m], small)"""
    m = 2 * M
    base = A.rand_complex((K, M + 1), 45000 + 16 * M + hop)
    win = SC.window(m, "hann")

    def small(ids):
        X = base[ids][None]
        n = (len(ids) - 1) * hop + m
        inv = istft_envelope_lines(win, m, hop, len(ids)).reshape(-1)
        return SC.inverse_reference(X, win, inv, n, m, hop, 0)[0].reshape(-1, hop)
    return base, win, small


def istft_inv_env(win, m, hop, frames, prec, device):
    """The inverse envelope of a row of `frames` frames on the device, built from its head lines, its one interior line and its tail
    lines (the envelope of a short row has the same ones: sums of the same squares in the same order)."""
    import torch
    q = m // hop - 1
    lines = istft_envelope_lines(win, m, hop, 2 * q + 2)                 # q head lines, q + 2 interior lines, q tail lines
    assert np.array_equal(lines[q], lines[q + 1])
    t = torch.from_numpy(lines).to(LE.torch_dtype(prec, False)).to(device)
    env = torch.empty((frames + q, hop), dtype=t.dtype, device=device)
    env[:q], env[q:frames], env[frames:] = t[:q], t[q], t[2 * q + 2:]
    return env.view(-1)


# ---- running a case --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def _bounds_and_worst_per_family():
    """The families' bounds before the first case; after the last one the worst line difference per family and precision"""
    import torch
    register_bounds()
    yield
    for (family, prec), (value, what) in sorted(LE.WORST_LINES.items()):
        print(f"large-extent worst {family} {prec}: {value:.3f} eps sqrt(log2 n) (limit {2 * LE.family_bound(family, prec)})  {what}")
    torch.cuda.empty_cache()   # the last case's filter, window and envelope (up to 8.6 GB) go back to the device, not into torch's cache


def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


def _skip_unless_it_fits(peak):
    """The module's rule: the case's peak against the free HBM, before anything is allocated"""
    import torch
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if peak > free:
        pytest.skip(f"needs {peak / 2**30:.0f} GiB of HBM, {free / 2**30:.0f} free")


def _filter(H, prec, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(H)).to(LE.torch_dtype(prec, np.iscomplexobj(H))).to(device)


def _run_rows(gpu, what, family, prec, m, x, ref, rows, call, inplace, K, extra):
    """rows as lines of large_extent.run_case; `extra`: the library's scratch and the filter, both part of the peak"""
    _, peak, _, _ = LE.case_plan(prec, x, ref, rows, 1, inplace, extra, K)
    _skip_unless_it_fits(peak)
    LE.run_case(gpu, what, family, prec, m, x, ref, rows, 1, call, inplace, K=K, scratch=extra)


@pytest.mark.parametrize("case", RCONV, ids=[c[0] for c in RCONV])
def test_rconv1d(gpu, monkeypatch, case):
    import torch
    from distributedfft_amd import api
    cid, M, n, kind, prec, _, inplace, composed, per_row = case
    m, lib = 2 * M, _lib()
    monkeypatch.delenv("DFFT_RCONV_FUSED", raising=False)
    K, rows, channels, batch = rconv_plan(case)
    assert bool(lib.dfft_rconv1d_fused_applies(n, m, CODE[prec], KIND[kind], int(n % 2 == 0))) == (not composed)   # the route of the case
    scratch = int(lib.dfft_rconv1d_scratch_bytes(n, m, channels, batch, CODE[prec]))
    assert (scratch > 0) == composed
    x, H, ref = rconv_base(M, n, kind, K)
    hbytes = channels * (M + 1) * RB[prec] * (1 if kind == "real" else 2)
    _, peak, _, _ = LE.case_plan(prec, x, ref, rows, 1, inplace, scratch + hbytes, K)
    _skip_unless_it_fits(peak)
    if per_row:
        Hd = torch.empty((channels, M + 1, 1), dtype=LE.torch_dtype(prec, kind == "complex"), device=gpu)
        LE.fill(Hd, LE.base_tensor(H, prec, gpu), K)
        Hd = Hd.view(channels, M + 1)
    else:
        Hd = _filter(H, prec, gpu)
    _run_rows(gpu, f"rconv1d {cid}", "rconv1d", prec, m, x, ref, rows,
              lambda t, o: api.rconv1d(t.view(batch, channels, n), Hd, m, out=o.view(batch, channels, n)), inplace, K, scratch + hbytes)


@pytest.mark.parametrize("case", OS_ROWS, ids=[c[0] for c in OS_ROWS])
def test_rconv1d_os_rows(gpu, monkeypatch, case):
    from distributedfft_amd import api
    cid, M, d, n, kind, prec, _ = case
    m, lib = 2 * M, _lib()
    monkeypatch.delenv("DFFT_RCONV_FUSED", raising=False)
    K, rows = os_rows_plan(case)
    assert lib.dfft_rconv1d_os_fused_applies(m, CODE[prec]) == 1 and lib.dfft_rconv1d_os_scratch_bytes(n, m, d, K, rows // K, CODE[prec]) == 0
    x, H, ref = os_rows_base(M, d, n, kind, K)
    Hd = _filter(H, prec, gpu)
    _run_rows(gpu, f"rconv1d_os {cid}", "rconv1d_os", prec, m, x, ref, rows,
              lambda t, o: api.rconv1d_os(t.view(rows // K, K, n), Hd, m, d, n, out=o.view(rows // K, K, n)), False, K, 0)


@pytest.mark.parametrize("case", LONG, ids=[c[0] for c in LONG])
def test_rconv1d_long(gpu, monkeypatch, case):
    from distributedfft_amd import api
    cid, m, n, kind, prec, _, inplace, composed = case
    lib = _lib()
    if composed:
        monkeypatch.setenv("DFFT_RCONV_LONG_FUSED", "0")
    else:
        monkeypatch.delenv("DFFT_RCONV_LONG_FUSED", raising=False)
    K, rows = long_plan(case)
    assert bool(lib.dfft_rconv1d_long_fused_applies(m, CODE[prec])) == (not composed)
    scratch = int(lib.dfft_rconv1d_long_scratch_bytes(n, m, K, rows // K, CODE[prec]))
    assert scratch > 0                                    # both routes lease: the fused passes hand over through a chunk of scratch rows
    if composed:
        scratch *= 3                                      # bins and padded rows of a chunk, and the four-step real rows' own scratch
    x, H, ref = rconv_base(m // 2, n, kind, K)
    Hp = api.rconv1d_long_filter(_filter(H, prec, gpu), m)
    _run_rows(gpu, f"rconv1d_long {cid}", "rconv1d_long", prec, m, x, ref, rows,
              lambda t, o: api.rconv1d_long(t.view(rows // K, K, n), Hp, m, out=o.view(rows // K, K, n)), inplace, K, scratch)


def _run_band(gpu, what, family, prec, m, base, small, band, p_out, out_complex, call, extra):
    K, peak, _, _ = LE.band_plan(prec, base, band, p_out, out_complex, extra, K=base.shape[0])
    _skip_unless_it_fits(peak)
    LE.run_band_case(gpu, what, family, prec, m, base, small, band, p_out, out_complex, call, K=K, scratch=extra)


def _band_k(band, p_in, p_out, eb_in, eb_out):
    return LE.band_pick_k(band, p_in, p_out, eb_in, eb_out)


@pytest.mark.parametrize("case", OS_BAND, ids=[c[0] for c in OS_BAND])
def test_rconv1d_os_one_row(gpu, monkeypatch, case):
    from distributedfft_amd import api
    cid, M, d, lines, kind, prec, fused = case
    m, lib = 2 * M, _lib()
    monkeypatch.delenv("DFFT_RCONV_FUSED", raising=False)
    band, S = os_band(case)
    n = lines * S
    assert bool(lib.dfft_rconv1d_os_fused_applies(m, CODE[prec])) == fused
    scratch = int(lib.dfft_rconv1d_os_scratch_bytes(n, m, d, 1, 1, CODE[prec]))
    assert (scratch == 0) == fused
    K = _band_k(band, S, S, RB[prec], RB[prec])
    base, H, small = os_band_base(M, d, kind, K)
    Hd = _filter(H, prec, gpu)
    _run_band(gpu, f"rconv1d_os {cid}", "rconv1d_os", prec, m, base, small, band, S, False,
              lambda t, o: api.rconv1d_os(t.view(1, 1, n), Hd, m, d, n, out=o.view(1, 1, n)), scratch)


@pytest.mark.parametrize("case", STFT, ids=[c[0] for c in STFT])
def test_stft1d(gpu, monkeypatch, case):
    import torch
    from distributedfft_amd import api
    cid, M, hop, lines, kind, prec, composed = case
    m, lib = 2 * M, _lib()
    if composed:
        monkeypatch.setenv("DFFT_STFT_FUSED", "0")
    else:
        monkeypatch.delenv("DFFT_STFT_FUSED", raising=False)
    monkeypatch.delenv("DFFT_STFT_CHUNK_BYTES", raising=False)          # the natural 256 MiB chunks
    band, _, bins = stft_band(case)
    n, frames = lines * hop, band.lout
    assert lib.dfft_stft1d_frames(n, m, hop, 0) == frames
    assert bool(lib.dfft_stft1d_fused_applies(m, CODE[prec])) == (not composed)
    scratch = int(lib.dfft_stft1d_scratch_bytes(m, frames, 1, CODE[prec], SC.KIND_CODE[kind]))
    assert (scratch > 0) == composed
    cplx = kind == "complex"
    K = _band_k(band, hop, bins, RB[prec], RB[prec] * (2 if cplx else 1))
    base, win, small = stft_base(M, hop, kind, K)
    wd = torch.from_numpy(win).to(LE.torch_dtype(prec, False)).to(gpu)
    _run_band(gpu, f"stft1d {cid}", "stft" if cplx else "stft-power", prec, m, base, small, band, bins, cplx,
              lambda t, o: api.stft(t.view(1, n), m, hop, window=wd, center=False, frames_last=False, power=None if cplx else 2,
                                    out=o.view(1, frames, bins)), scratch)


@pytest.mark.parametrize("case", ISTFT, ids=[c[0] for c in ISTFT])
def test_istft1d(gpu, monkeypatch, case):
    """Through the C ABI: api.istft builds the envelope of the whole row in fp64 beside the case's plan."""
    import torch
    import test_gpu_stft as TS
    cid, M, hop, rows, frames, prec = case
    m, lib = 2 * M, _lib()
    monkeypatch.delenv("DFFT_STFT_CHUNK_BYTES", raising=False)
    band, bins, _ = istft_band(case)
    n = band.lout * hop
    assert n == (frames - 1) * hop + m
    scratch = int(lib.dfft_istft1d_scratch_bytes(m, frames, rows, CODE[prec]))
    assert scratch > 0
    K = _band_k(band, bins, hop, 2 * RB[prec], RB[prec])
    base, win, small = istft_base(M, hop, K)
    extra = scratch + n * RB[prec]                                        # inv_env is part of the peak
    _, peak, _, _ = LE.band_plan(prec, base, band, hop, False, extra, K=K)
    _skip_unless_it_fits(peak)
    wd = torch.from_numpy(win).to(LE.torch_dtype(prec, False)).to(gpu)
    env = istft_inv_env(win, m, hop, frames, prec, gpu)
    assert env.numel() == n
    _run_band(gpu, f"istft1d {cid}", "istft", prec, m, base, small, band, hop, False,
              lambda t, o: TS._istft_raw(t, o, wd, env, n, m, hop, 0, frames, rows, prec), extra)
