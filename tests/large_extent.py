"""Helpers of the large-extent tests (tests/test_large_extent_host.py, tests/test_gpu_large_extent.py and the chunk-edge cases of
tests/test_gpu_bluestein.py / tests/test_gpu_r2r.py): tensors of tens of GiB whose every line is checked, without a reference of that size.

TILED INPUTS.  A tensor is seen as [batch][m][s]; its lines run along the middle axis, line L = b * s + c (rows: s = 1, L = the row).
Line L holds base line L mod K of K distinct base lines (accuracy_ref's complex_lines / real_lines / half_spectra / r2r_lines /
complex_planes, whose longdouble transforms are the reference); K is a small prime, 61 unless wrap_distinct rejects it for a shape.

CHECKS.  (1) The first K output lines against the longdouble reference, as accuracy_ref.nu under the family's BOUND (accuracy_ref.check:
no new tolerance).  (2) EVERY output line against output line L mod K, per line, relative L2 in fp64, in slices on the device: both are
within BOUND eps sqrt(log2 n) of the same true line, so they differ by at most 2 BOUND eps sqrt(log2 n) -- derived, not tuned.  The worst
line and its (b, c) are reported.  (3) Out of place: `out` starts as NaN (an unwritten line fails (2)) and the input is rebuilt and
compared bit for bit afterwards.  In place an unwritten line still holds its input and fails (2).  (4) wrap_distinct: an access that lands
2^31, 2^32 or 2^33 elements (or 2^31 / 2^32 bytes) away from where it should finds a DIFFERENT value there, a different (L mod K, k).

ROWS WHOSE NEIGHBOURING LINES INTERACT (Band, run_band_case: one long row of overlap-save blocks, STFT frames and their inverse).  Input
and output have their own line counts and lengths, and an output line depends on a few neighbouring input lines, so it is a function of
its index modulo K only away from a row's ends.  The base lines of check (2) are therefore the output lines K ... 2K - 1, the lines at a
row's ends are held against their own longdouble reference (rows past the first K: against the same lines of row r mod K), and the
reference of the K interior lines is the family's own reference on a short tiled row, whose lines K ... 2K - 1 see whole windows -- the
period-K circular form.  Families outside accuracy_ref.BOUND register the bound their own GPU module asserts in EXTRA_BOUND.

Everything takes torch tensors on any device: the host tests run the same code on CPU tensors with numpy standing in for the transform.
Temporaries stay under 1 GiB (SLICE_BYTES per temporary, a handful alive at once).

The mirrors of the library's chunk rules at the end size the chunk-edge cases and the peak memory of a case; tests/test_large_extent_host.py
holds them against the library's own dfft_*_scratch_bytes exports."""
import math
import time

import numpy as np

import accuracy_ref as A

K_DEFAULT = 61
K_CANDIDATES = (61, 67, 71, 73, 79, 83, 89, 97)
GIB = 1 << 30
SLICE_BYTES = 96 << 20
WRAPS_ELEMS = (1 << 31, 1 << 32, 1 << 33)      # 2^33 elements: 2^32 column pairs of fp32
WRAPS_BYTES = (1 << 31, 1 << 32)
CAP_80 = 80 * GIB                              # no case may need more


# ---- the wrap assertion ------------------------------------------------------------------------------------------------------------------
def wrap_hits(batch, m, s, K, shift):
    """The (carry, line delta) pairs at which flat element e and e + shift of [batch][m][s] hold the same (L mod K, k); [] is a pass.
    e = (b m + k) s + c; shift = q s + r moves c to c + r - carry s and the row b m + k by q + carry: k is kept iff m divides q + carry,
    and then the line index moves by (q + carry) / m * s + r - carry s, which must not be a multiple of K."""
    if shift >= batch * m * s:
        return []                                # no two elements of the tensor are that far apart
    q, r = divmod(shift, s)
    hits = []
    for carry in ((0, 1) if r else (0,)):
        rows = q + carry
        if rows % m == 0:
            dl = rows // m * s + r - carry * s
            if dl % K == 0:
                hits.append((carry, dl))
    return hits


def wrap_distinct(batch, m, s, K, elem_bytes):
    """True iff no shift of WRAPS_ELEMS elements or WRAPS_BYTES bytes (where that is whole elements) maps an element onto an equal one."""
    shifts = list(WRAPS_ELEMS) + [w // elem_bytes for w in WRAPS_BYTES if w % elem_bytes == 0]
    return all(not wrap_hits(batch, m, s, K, d) for d in shifts)


def pick_k(shapes):
    """The first K of K_CANDIDATES that wrap_distinct accepts for every (batch, m, s, elem_bytes) of `shapes`."""
    for K in K_CANDIDATES:
        if all(wrap_distinct(b, m, s, K, eb) for b, m, s, eb in shapes):
            return K
    raise AssertionError(f"no K of {K_CANDIDATES} keeps wrapped accesses apart for {shapes}")


# ---- slices --------------------------------------------------------------------------------------------------------------------------------
def blocks(batch, m, s, elem_bytes, budget=None):
    """(b0, b1, c0, c1) blocks covering [batch][m][s], each at most `budget` bytes (whole items, or column ranges of one item)."""
    budget = SLICE_BYTES if budget is None else budget
    item = m * s * elem_bytes
    if item <= budget:
        nb = max(1, budget // item)
        for b0 in range(0, batch, nb):
            yield b0, min(batch, b0 + nb), 0, s
    else:
        nc = max(1, budget // (m * elem_bytes))
        for b in range(batch):
            for c0 in range(0, s, nc):
                yield b, b + 1, c0, min(s, c0 + nc)


def _line_ids(b0, b1, c0, c1, s, K, device):
    import torch
    b = torch.arange(b0, b1, device=device, dtype=torch.int64)[:, None]
    c = torch.arange(c0, c1, device=device, dtype=torch.int64)[None, :]
    return (b * s + c) % K                       # [nb][nc]


def _tiled_block(baseT, ids):
    """baseT [m][K], ids [nb][nc] -> [nb][m][nc] (a view of the gathered [m][nb][nc]: the column index stays the fast one)"""
    return baseT[:, ids].permute(1, 0, 2)


def torch_dtype(prec, complex_):
    import torch
    return {("f64", True): torch.complex128, ("f32", True): torch.complex64, ("f64", False): torch.float64,
            ("f32", False): torch.float32}[(prec, bool(complex_))]


def base_tensor(base, prec, device):
    """numpy [K][m] base lines (float32-exact values) -> their transpose [m][K] in the working type on `device`."""
    import torch
    b = np.ascontiguousarray(np.asarray(base).T)
    return torch.from_numpy(b).to(device).to(torch_dtype(prec, np.iscomplexobj(b)))


def fill(t, baseT, K):
    """t [batch][m][s] <- line L = base line L mod K, in slices."""
    batch, m, s = t.shape
    assert baseT.shape == (m, K) and baseT.dtype == t.dtype
    for b0, b1, c0, c1 in blocks(batch, m, s, t.element_size()):
        t[b0:b1, :, c0:c1] = _tiled_block(baseT, _line_ids(b0, b1, c0, c1, s, K, t.device))
    return t


def _bits(v):
    """a tensor's elements as integers of the same width (complex: [..., 2]): bit-for-bit comparison, NaN included"""
    import torch
    v = torch.view_as_real(v.contiguous()) if v.is_complex() else v.contiguous()
    return v.view(torch.int64 if v.dtype == torch.float64 else torch.int32)


def _block_differs(t, baseT, K, blk):
    b0, b1, c0, c1 = blk
    want = _tiled_block(baseT, _line_ids(b0, b1, c0, c1, t.shape[2], K, t.device))
    ne = _bits(t[b0:b1, :, c0:c1]) != _bits(want)
    return ne.any(-1) if t.is_complex() else ne


def input_intact(t, baseT, K):
    """None if t still holds exactly what fill wrote (bit for bit), else the first differing (b, k, c)."""
    import torch
    batch, m, s = t.shape
    blks = list(blocks(batch, m, s, t.element_size()))
    counts = torch.stack([_block_differs(t, baseT, K, blk).sum() for blk in blks]).cpu().tolist()   # one host round trip
    for blk, n in zip(blks, counts):
        if n:
            i = torch.nonzero(_block_differs(t, baseT, K, blk))[0].cpu().tolist()
            return blk[0] + i[0], i[1], blk[2] + i[2]
    return None


def first_lines(t, K):
    """The first K lines of [batch][m][s] -> [K][m] (lines L = 0 ... K-1, i.e. (b, c) = divmod(L, s))."""
    import torch
    batch, m, s = t.shape
    assert batch * s >= K, "the tensor has fewer than K lines"
    if s >= K:
        return t[0, :, :K].T.contiguous()
    nb = -(-K // s)
    return t[:nb].permute(0, 2, 1).reshape(nb * s, m)[:K].contiguous()


def worst_line(out, K):
    """Every line of out [batch][m][s] against line L mod K of out itself: (worst per-line relative L2 difference in fp64, (b, c) of
    that line).  A line holding a NaN or an infinity counts as infinitely far."""
    import torch
    batch, m, s = out.shape
    wide = torch.complex128 if out.is_complex() else torch.float64
    first = first_lines(out, K).to(wide)
    firstT = first.T.contiguous()

    def sq(v):                                   # sum over the line axis (1) of |v|^2
        return torch.view_as_real(v).pow(2).sum((1, -1)) if v.is_complex() else v.pow(2).sum(1)

    den = sq(first)                              # [K]
    found = []
    for b0, b1, c0, c1 in blocks(batch, m, s, 16 if out.is_complex() else 8, SLICE_BYTES // 2):
        ids = _line_ids(b0, b1, c0, c1, s, K, out.device)
        d = out[b0:b1, :, c0:c1].to(wide) - _tiled_block(firstT, ids)
        rel = torch.sqrt(sq(d) / den[ids])
        rel = torch.nan_to_num(rel, nan=math.inf, posinf=math.inf)
        v, i = rel.reshape(-1).max(0)
        found.append((v, i, b0, c0, c1 - c0))
    vals = torch.stack([f[0] for f in found]).cpu().tolist()
    idxs = torch.stack([f[1] for f in found]).cpu().tolist()
    j = max(range(len(found)), key=lambda q: vals[q])
    _, _, b0, c0, nc = found[j]
    return float(vals[j]), (b0 + idxs[j] // nc, c0 + idxs[j] % nc)


EXTRA_BOUND = {}   # family -> {prec: bound}: the bounds that a family's own GPU module asserts, for families outside accuracy_ref.BOUND


def family_bound(family, prec):
    """The BOUND of check (1): accuracy_ref's, or the one a family outside accuracy_ref registered in EXTRA_BOUND (no new tolerance)."""
    return EXTRA_BOUND[family][prec] if family in EXTRA_BOUND else A.BOUND[family][prec]


def line_limit(family, prec, n_eff):
    """2 BOUND eps sqrt(log2 n): two results within BOUND eps sqrt(log2 n) (relative L2) of one true line."""
    return 2 * family_bound(family, prec) * A.EPS[prec] * math.sqrt(math.log2(max(n_eff, 2)))


def check_bound(family, prec, value, what):
    """accuracy_ref.check for every family: prints the figure and holds it against the family's BOUND."""
    if family in A.BOUND:
        return A.check(family, prec, value, what)
    print(f"accuracy {family} {prec} {what}: nu {value:.3f}")
    assert value <= family_bound(family, prec), (family, prec, what, value, family_bound(family, prec))


WORST_LINES = {}   # (family, prec) -> (worst line difference in units of its limit's eps sqrt(log2 n), case) of this process


def check_output(out, ref, K, family, prec, n_eff, what):
    """Checks (1) and (2) of the module's docstring on out [batch][m][s]; `ref` is the longdouble reference [K][m] of the base lines."""
    got = first_lines(out, K).cpu().numpy()
    per_line = [A.nu(got[i:i + 1], ref[i:i + 1], n_eff, prec, (1,)) for i in range(K)]
    i = max(range(K), key=lambda q: per_line[q] if per_line[q] == per_line[q] else math.inf)   # a NaN line is the worst
    try:
        check_bound(family, prec, max(per_line[i], A.nu(got, ref, n_eff, prec, (1,))), f"{what} base lines")
    except AssertionError as e:
        raise AssertionError((what, "worst base line", i, "at (b, c) =", divmod(i, out.shape[2]), per_line[i]) + tuple(e.args)) from None
    worst, (b, c) = worst_line(out, K)
    unit = A.EPS[prec] * math.sqrt(math.log2(max(n_eff, 2)))
    print(f"large-extent {family} {prec} {what}: worst line (b={b}, c={c}) differs from its base line by {worst / unit:.3f} eps sqrt(log2 n)"
          f" (limit {2 * family_bound(family, prec)})")
    if worst / unit > WORST_LINES.get((family, prec), (-1.0, ""))[0]:
        WORST_LINES[(family, prec)] = (worst / unit, what)
    assert worst <= line_limit(family, prec, n_eff), (what, "line", (b, c), "base line", (b * out.shape[2] + c) % K, worst / unit,
                                                     2 * family_bound(family, prec))


def case_plan(prec, base_in, ref, batch, s, inplace, scratch=0, K=None):
    """What a case allocates, before anything is allocated: (K, peak bytes, input dtype, output dtype).  The peak is the buffers, the
    library's scratch and 1 GiB; it never exceeds the 80 GiB a case may need."""
    import torch
    m_in, m_out = base_in.shape[1], ref.shape[1]
    tin, tout = torch_dtype(prec, np.iscomplexobj(base_in)), torch_dtype(prec, np.iscomplexobj(ref))
    eb_in, eb_out = torch.empty(0, dtype=tin).element_size(), torch.empty(0, dtype=tout).element_size()
    if inplace:
        assert (m_in, tin) == (m_out, tout)
    shapes = [(batch, m_in, s, eb_in)] + ([] if inplace else [(batch, m_out, s, eb_out)])
    K = pick_k(shapes) if K is None else K
    assert base_in.shape[0] == K and ref.shape[0] == K
    assert all(wrap_distinct(b, m, s_, K, eb) for b, m, s_, eb in shapes), (shapes, K)
    peak = peak_bytes(batch * m_in * s * eb_in, 0 if inplace else batch * m_out * s * eb_out, scratch)
    assert peak <= CAP_80, peak
    return K, peak, tin, tout


def run_case(device, what, family, prec, n_eff, base_in, ref, batch, s, call, inplace, K=None, scratch=0, offset=False):
    """One tiled case.  base_in [K][m_in] and ref [K][m_out] (numpy; complex or real each) fix the two tensors [batch][m][s];
    call(x, out) runs the transform (out is x in place).  Prints the seconds of the call, the peak bytes and the wall time of the whole
    case (fill, call, checks); returns (seconds of the call, peak bytes).  offset: the input starts one element past a 16-byte boundary
    (complex64: 8-byte aligned only, the scalar fp32 kernels)."""
    import torch
    t_case = time.perf_counter()
    K, peak, tin, tout = case_plan(prec, base_in, ref, batch, s, inplace, scratch, K)
    m_in, m_out = base_in.shape[1], ref.shape[1]
    baseT = base_tensor(base_in, prec, device)
    if offset:
        x = torch.empty(batch * m_in * s + 1, dtype=tin, device=device)[1:].view(batch, m_in, s)
        assert x.data_ptr() % 16 == x.element_size() % 16
    else:
        x = torch.empty((batch, m_in, s), dtype=tin, device=device)
    fill(x, baseT, K)
    out = x if inplace else torch.full((batch, m_out, s), math.nan, dtype=tout, device=device)
    if device.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    call(x, out)
    if device.type == "cuda":
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"large-extent {what}: call {dt:.3f} s, peak {peak} bytes = {peak / 2**30:.1f} GiB (K = {K})")
    try:
        if not inplace:
            hit = input_intact(x, baseT, K)
            assert hit is None, (what, "the input changed at (b, k, c) =", hit)
        check_output(out, ref, K, family, prec, n_eff, what)
    finally:
        del x, out, baseT
        if device.type == "cuda":
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
        print(f"large-extent {what}: case wall time {time.perf_counter() - t_case:.2f} s")
    return dt, peak


# ---- rows whose neighbouring lines interact (overlap-save, STFT, inverse STFT) ----------------------------------------------------------------
class Band:
    """`rows` rows cut into lines: a row holds `lin` input lines of p_in elements and `lout` output lines of p_out elements, and output
    line t of a row depends on the row's input lines t - qb ... t + qa (those inside [0, lin)).  Input line g = r * lin + i of the whole
    tensor holds base line g mod K, so output line (r, t) is a function of (r * lin + t) mod K alone wherever its window is whole:
    qb <= t < lin - qa, the INTERIOR lines.  The first qb lines of a row (head) and its last tail = lout - (lin - qa) lines see a cut
    window: EDGE lines.
        overlap-save, lines of S = m - d samples     qb = ceil(d / S), qa = 0, lout = lin
        STFT without centring, lines of hop samples  qb = 0, qa = m / hop - 1, lout = lin - qa (frames of m/2 + 1 bins): no edge line
        inverse STFT, lines of hop samples           qb = m / hop - 1, qa = 0, lout = lin + qb (lin frames)
    The base lines of check (2) are the output lines K ... 2K - 1 of row 0 (all interior: K >= qb, lin >= 2K + qa)."""

    def __init__(self, rows, lin, lout, qb, qa):
        self.rows, self.lin, self.lout, self.qb, self.qa = rows, lin, lout, qb, qa
        self.tail = lout - (lin - qa)
        assert rows >= 1 and qb >= 0 and qa >= 0 and self.tail >= 0 and lout >= 1, vars(self)

    def edge_rows(self, K):
        """rows whose edge lines are held against their own reference: row r's edges equal those of row r mod K"""
        return min(self.rows, K)

    def head_ids(self, K):
        """input lines of the small signal whose output lines 0 ... 2K - 1 are those of row 0"""
        return [g % K for g in range(2 * K + self.qa + self.qb)]

    def edge_ids(self, K, r, head):
        """input lines of a small signal that starts (head) or ends (not head) as row r does"""
        T = 2 * (self.qa + self.qb) + 2
        first = r * self.lin + (0 if head else self.lin - T)
        return [(first + i) % K for i in range(T)]


def band_wrap_hits(band, p_out, K, shift):
    """The output tensor [rows][lout][p_out] of a Band: (carry, class delta) at which element e and e + shift are the same element k of
    interior lines of one class; [] is a pass.  shift = (a lout + b) p_out moves line (r, t) to (r + a, t + b) or (r + a + 1, t + b -
    lout), and the class (r lin + t) mod K by a lin + b or (a + 1) lin + b - lout."""
    if shift >= band.rows * band.lout * p_out or shift % p_out:
        return []
    a, b = divmod(shift // p_out, band.lout)
    hits = []
    if (a * band.lin + b) % K == 0:
        hits.append((0, a * band.lin + b))
    if b and a + 1 < band.rows and ((a + 1) * band.lin + b - band.lout) % K == 0:
        hits.append((1, (a + 1) * band.lin + b - band.lout))
    return hits


def band_wrap_distinct(band, p_in, p_out, K, eb_in, eb_out):
    """wrap_distinct for both tensors of a Band: the input is [rows * lin][p_in][1] with line g = base line g mod K"""
    shifts = list(WRAPS_ELEMS) + [w // eb_out for w in WRAPS_BYTES if w % eb_out == 0]
    return (wrap_distinct(band.rows * band.lin, p_in, 1, K, eb_in) and all(not band_wrap_hits(band, p_out, K, d) for d in shifts)
            and band.lin >= 2 * K + band.qa and K >= band.qb)


def band_pick_k(band, p_in, p_out, eb_in, eb_out):
    for K in K_CANDIDATES:
        if band_wrap_distinct(band, p_in, p_out, K, eb_in, eb_out):
            return K
    raise AssertionError(f"no K of {K_CANDIDATES} keeps wrapped accesses apart for {vars(band)}, lines of {p_in} / {p_out}")


def band_refs(band, K, small):
    """The longdouble references of a Band from `small(ids) -> [lines][p_out]`, the family's reference of ONE complete row whose input
    lines are the base lines ids: (the K interior classes [K][p_out], heads [edge rows][qb][p_out], tails [edge rows][tail][p_out]).
    The classes are the period-K form of the reference: lines K ... 2K - 1 of a row of 2K + qa + qb tiled lines see whole windows."""
    o = np.asarray(small(band.head_ids(K)))
    assert o.shape[0] >= 2 * K, o.shape
    classes = o[K:2 * K]
    nk = band.edge_rows(K)
    heads = np.stack([np.asarray(small(band.edge_ids(K, r, True)))[:band.qb] for r in range(nk)]) if band.qb else None
    tails = np.stack([np.asarray(small(band.edge_ids(K, r, False)))[-band.tail:] for r in range(nk)]) if band.tail else None
    return classes, heads, tails


def band_table(out2, band, K):
    """out2 [rows * lout][p_out] -> what every line is compared with, [K + nk qb + nk tail][p_out]: the interior classes (lines K ...
    2K - 1 of row 0), then the head and the tail lines of the first nk = min(rows, K) rows."""
    import torch
    nk, o3 = band.edge_rows(K), out2.view(band.rows, band.lout, -1)
    parts = [out2[K:2 * K]]
    if band.qb:
        parts.append(o3[:nk, :band.qb].reshape(nk * band.qb, -1))
    if band.tail:
        parts.append(o3[:nk, band.lout - band.tail:].reshape(nk * band.tail, -1))
    return torch.cat(parts).contiguous()


def _band_index(g0, g1, band, K, device):
    """row of band_table for the output lines g0 ... g1 - 1 (g = r lout + t)"""
    import torch
    g = torch.arange(g0, g1, device=device, dtype=torch.int64)
    r = g // band.lout
    t = g - r * band.lout
    nk, rk = band.edge_rows(K), r % K
    idx = (r * band.lin + t) % K
    if band.qb:
        idx = torch.where(t < band.qb, K + rk * band.qb + t, idx)
    if band.tail:
        idx = torch.where(t >= band.lout - band.tail, K + nk * band.qb + rk * band.tail + (t - (band.lout - band.tail)), idx)
    return idx


def band_worst_line(out2, band, K):
    """Every line of out2 [rows * lout][p_out] against the line of band_table it must equal: (worst per-line relative L2 difference in
    fp64, (r, t) of that line).  A line holding a NaN or an infinity counts as infinitely far."""
    import torch
    lines, p = out2.shape
    wide = torch.complex128 if out2.is_complex() else torch.float64
    table = band_table(out2, band, K).to(wide)

    def sq(v):
        return torch.view_as_real(v).pow(2).sum((1, -1)) if v.is_complex() else v.pow(2).sum(1)

    den = sq(table)
    nl = max(1, SLICE_BYTES // 2 // (p * (16 if out2.is_complex() else 8)))
    found = []
    for g0 in range(0, lines, nl):
        g1 = min(lines, g0 + nl)
        idx = _band_index(g0, g1, band, K, out2.device)
        rel = torch.sqrt(sq(out2[g0:g1].to(wide) - table[idx]) / den[idx])
        v, i = torch.nan_to_num(rel, nan=math.inf, posinf=math.inf).max(0)
        found.append((v, i + g0))
    vals = torch.stack([f[0] for f in found]).cpu().tolist()
    at = torch.stack([f[1] for f in found]).cpu().tolist()
    j = max(range(len(found)), key=lambda q: vals[q])
    return float(vals[j]), divmod(at[j], band.lout)


def band_check_output(out2, refs, band, K, family, prec, n_eff, what):
    """Checks (1) and (2) for a Band: the K interior classes and every edge line of the first min(rows, K) rows against their longdouble
    references under the family's BOUND; every line against the line of those it must equal under twice that bound."""
    classes, heads, tails = refs
    table = band_table(out2, band, K).cpu().numpy()
    nk = band.edge_rows(K)
    named = [(table[:K], classes, [(0, K + i) for i in range(K)], "interior")]
    if band.qb:
        named.append((table[K:K + nk * band.qb], heads.reshape(nk * band.qb, -1), [(r, t) for r in range(nk) for t in range(band.qb)], "head"))
    if band.tail:
        named.append((table[K + nk * band.qb:], tails.reshape(nk * band.tail, -1),
                      [(r, band.lout - band.tail + t) for r in range(nk) for t in range(band.tail)], "tail"))
    worst = (-1.0, None, "")
    for got, ref, where, kind in named:
        assert got.shape == ref.shape, (kind, got.shape, ref.shape)
        for i in range(len(where)):
            v = A.nu(got[i:i + 1], ref[i:i + 1], n_eff, prec, (1,))
            v = math.inf if v != v else v                      # a NaN line is the worst
            if v > worst[0]:
                worst = (v, where[i], kind)
    try:
        check_bound(family, prec, worst[0], f"{what} base and edge lines")
    except AssertionError as e:
        raise AssertionError((what, "worst", worst[2], "line at (r, t) =", worst[1], worst[0]) + tuple(e.args)) from None
    far, (r, t) = band_worst_line(out2, band, K)
    unit = A.EPS[prec] * math.sqrt(math.log2(max(n_eff, 2)))
    print(f"large-extent {family} {prec} {what}: worst line (r={r}, t={t}) differs from its base line by {far / unit:.3f} eps sqrt(log2 n)"
          f" (limit {2 * family_bound(family, prec)})")
    if far / unit > WORST_LINES.get((family, prec), (-1.0, ""))[0]:
        WORST_LINES[(family, prec)] = (far / unit, what)
    assert far <= line_limit(family, prec, n_eff), (what, "line at (r, t) =", (r, t), "class", (r * band.lin + t) % K, far / unit,
                                                    2 * family_bound(family, prec))


def band_plan(prec, base_in, band, p_out, out_complex, scratch=0, K=None):
    """case_plan for a Band: (K, peak bytes, input dtype, output dtype) before anything is allocated"""
    import torch
    p_in = base_in.shape[1]
    tin, tout = torch_dtype(prec, np.iscomplexobj(base_in)), torch_dtype(prec, out_complex)
    eb_in, eb_out = torch.empty(0, dtype=tin).element_size(), torch.empty(0, dtype=tout).element_size()
    K = band_pick_k(band, p_in, p_out, eb_in, eb_out) if K is None else K
    assert base_in.shape[0] == K and band_wrap_distinct(band, p_in, p_out, K, eb_in, eb_out), (vars(band), K)
    peak = peak_bytes(band.rows * band.lin * p_in * eb_in, band.rows * band.lout * p_out * eb_out, scratch)
    assert peak <= CAP_80, peak
    return K, peak, tin, tout


def run_band_case(device, what, family, prec, n_eff, base_in, small, band, p_out, out_complex, call, K=None, scratch=0):
    """One tiled case of a Band, out of place.  base_in [K][p_in] (numpy) fixes the input [rows * lin][p_in]; small(ids) is the family's
    longdouble reference of one complete row of the base lines ids; call(x, out) runs the transform on x [rows * lin][p_in] and out
    [rows * lout][p_out].  Prints and returns what run_case does."""
    import torch
    t_case = time.perf_counter()
    K, peak, tin, tout = band_plan(prec, base_in, band, p_out, out_complex, scratch, K)
    refs = band_refs(band, K, small)
    p_in = base_in.shape[1]
    baseT = base_tensor(base_in, prec, device)
    x = torch.empty((band.rows * band.lin, p_in, 1), dtype=tin, device=device)
    fill(x, baseT, K)
    out = torch.full((band.rows * band.lout, p_out), math.nan, dtype=tout, device=device)
    if device.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    call(x.view(band.rows * band.lin, p_in), out)
    if device.type == "cuda":
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"large-extent {what}: call {dt:.3f} s, peak {peak} bytes = {peak / 2**30:.1f} GiB (K = {K})")
    try:
        hit = input_intact(x, baseT, K)
        assert hit is None, (what, "the input changed at (line, k, 0) =", hit)
        band_check_output(out, refs, band, K, family, prec, n_eff, what)
    finally:
        del x, out, baseT
        if device.type == "cuda":
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
        print(f"large-extent {what}: case wall time {time.perf_counter() - t_case:.2f} s")
    return dt, peak


def peak_bytes(in_bytes, out_bytes, scratch_bytes):
    """Buffers + the library's scratch + 1 GiB (the checks' slices, the allocator's slack, the tables)."""
    return in_bytes + out_bytes + scratch_bytes + GIB


# ---- base lines ----------------------------------------------------------------------------------------------------------------------------
def complex_base(n, K, direction):
    """-> (x [K][n], longdouble transform [K][n]) in `direction` (+1 forward, -1 unnormalised backward)"""
    x, F = A.complex_lines(n, (K, n), 1, 11000 + n)
    return x, (F if direction > 0 else A.reverse_bins(F, [1]))


def real_base(n, K):
    x, F = A.real_lines(n, K, 1, 12000 + n)
    return x[:, :, 0], F[:, :, 0]


def half_base(n, K):
    X, b = A.half_spectra(n, K, 1, 13000 + n)
    return X[:, :, 0], b[:, :, 0]


def r2r_base(n, K, kind):
    case = A.r2r_lines(n, K, 1, 14000 + n)
    return case[0][:, :, 0], case[1 + A.R2R_KINDS.index(kind)][:, :, 0]


def planes_base(n1, n2, K, direction):
    """planes as lines of n1 * n2 points"""
    x, F = A.complex_planes(n1, n2, K, 15000 + n1)
    F = F if direction > 0 else A.reverse_bins(F, (1, 2))
    return x.reshape(K, n1 * n2), F.reshape(K, n1 * n2)


def real_planes_base(n1, n2, K):
    x, F = A.real_planes(n1, n2, K, 16000 + n1)
    return x.reshape(K, n1 * n2), F.reshape(K, n1 * (n2 // 2 + 1))


def half_planes_base(n1, n2, K):
    X, b = A.half_planes(n1, n2, K, 17000 + n1)
    return X.reshape(K, n1 * (n2 // 2 + 1)), b.reshape(K, n1 * n2)


# ---- mirrors of the library's chunk rules ---------------------------------------------------------------------------------------------------
SCRATCH_CAP = 256 << 20                       # kScratchCap: the default of every `cap` below (DFFT_SCRATCH_CHUNK_BYTES lowers it per call)
CBYTES = {"f64": 16, "f32": 8}                # one complex element


def bluestein_per_transform_bytes(M, s, prec):
    """dfft_bluestein.hip per_transform_bytes: the padded data of one batch item, twice for a four-step M (long_fft's scratch)"""
    return M * s * CBYTES[prec] * (2 if M > 4096 else 1)


def cap_units(unit_bytes, units, cap=SCRATCH_CAP, at_least=1):
    """dfft_fused_host.h chunk_units: the units of `unit_bytes` each per chunk -- what fits `cap`, at least one and at least `at_least`,
    at most all of them"""
    return max(1, min(units, max(max(cap, unit_bytes) // unit_bytes, at_least)))


def chunk_sizes(units, per_chunk):
    """the chunk loop: [units of each chunk], in order"""
    return [min(per_chunk, units - u0) for u0 in range(0, units, per_chunk)]


def bluestein_chunk(M, s, batch, prec, cap=SCRATCH_CAP):
    """batch items per chunk of the multi-pass form"""
    return cap_units(bluestein_per_transform_bytes(M, s, prec), batch, cap)


def bluestein_scratch(M, s, batch, prec, fused, cap=SCRATCH_CAP):
    return 0 if fused else bluestein_chunk(M, s, batch, prec, cap) * bluestein_per_transform_bytes(M, s, prec)


def pair_units(s, batch):
    """dfft_r2r.hip r2r_units / r2r_sp: (units, packed pairs per row of a unit) -- batch items, or row pairs at s = 1"""
    return ((batch + 1) // 2, 1) if s == 1 else (batch, (s + 1) // 2)


def chunk_units(n, sp, prec, units, cap=SCRATCH_CAP):
    """units per chunk of the composed r2r route / items per chunk of the multi-pass real columns / pairs per chunk of the paired real
    rows (sp = 1): packed pairs within max(cap, one unit's)"""
    return cap_units(n * sp * CBYTES[prec], units, cap)


def chunk_bytes(n, sp, prec, nu, M, bs_fused, cap=SCRATCH_CAP):
    """scratch of one chunk: the packed pairs plus the inner transform's (M: the Bluestein padded length, 0 for kinds 1 and 2) -- the
    inner Bluestein chunks are cut by the same cap"""
    zb = nu * n * sp * CBYTES[prec]
    if M:
        return zb + bluestein_scratch(M, sp, nu, prec, bs_fused, cap)
    return 2 * zb if n > 4096 else zb


def composed_scratch(n, s, batch, prec, M, bs_fused, rows_pair=True, cap=SCRATCH_CAP):
    """r2r_scratch_bytes (rows_pair: s = 1 pairs rows) / real_cols_scratch_bytes (s > 1) of a call that does NOT run fused"""
    units, sp = pair_units(s, batch) if rows_pair else (batch, (s + 1) // 2)
    return chunk_bytes(n, sp, prec, chunk_units(n, sp, prec, units, cap), M, bs_fused, cap)


def real_pair_scratch(n, rows, prec, M, bs_fused, cap=SCRATCH_CAP):
    """real_pair_scratch_bytes of rows that do NOT run fused (real forms 2 and 3 outside the odd tuned lengths): chunks of whole pairs"""
    return chunk_bytes(n, 1, prec, chunk_units(n, 1, prec, (rows + 1) // 2, cap), M, bs_fused, cap)


def ragged_batch(cu):
    """two whole chunks and a ragged third"""
    return 2 * cu + max(1, cu // 3)
