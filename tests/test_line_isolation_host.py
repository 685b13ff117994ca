"""Host side of the line-isolation tests (no GPU): the partner rules of tests/line_isolation.py against a numpy restatement of each pairing
(which lines of the model turn NaN when one input line is NaN), the dirty-set builder and the two checks on same-precision CPU models
of every family -- and on a deliberately WRONG model that couples line i with line i + 2, which same_outside must reject naming the
right line --, and nu_pair of the same-precision CPU pipeline (scipy.fft on the packed pairs) on every paired case of
tests/test_gpu_line_isolation.py under the families' existing bounds.  The figures are printed.

Where scipy is missing, fp64 runs against numpy and fp32 is left out of the parameters (numpy computes complex64 transforms in double)."""
import numpy as np
import pytest

import accuracy_ref as A
import line_isolation as LI

try:
    import scipy.fft as sf
except ImportError:   # pragma: no cover
    sf = None

LD, CLD = A.LD, A.CLD
PRECS = [p for p in A.PRECS if sf is not None or p == "f64"]


def _fft(z, prec, inverse=False):
    """Unnormalised transform of the rows of z in the working precision"""
    z = np.ascontiguousarray(z).astype(A.CDT[prec])
    m = sf if sf is not None else np.fft
    return m.ifft(z, axis=-1, norm="forward") if inverse else m.fft(z, axis=-1)


# ---- numpy models of the pairings: lines [L][n], paired inside every group of consecutive lines ----------------------------------------
def _pairs(lines, groups, order=None):
    """-> (a [P][n], b [P][n], ia, ib): the lines packed two by two inside every group, an odd last line with zeros (ib = -1).
    order: a permutation of the lines applied first (the WRONG model pairs line i with i + 2 through it)."""
    ia, ib = [], []
    for g in groups:
        g = list(g) if order is None else [g[0] + j for j in order(len(g))]
        for p in range(0, len(g), 2):
            ia.append(g[p])
            ib.append(g[p + 1] if p + 1 < len(g) else -1)
    a = lines[ia]
    b = np.where(np.array(ib)[:, None] >= 0, lines[np.maximum(ib, 0)], 0)
    return a, b, ia, ib


def _unpack(L, width, dtype, ia, ib, ya, yb):
    out = np.empty((L, width), dtype=dtype)
    out[ia] = ya
    keep = [j for j, i in enumerate(ib) if i >= 0]
    out[[ib[j] for j in keep]] = yb[keep]
    return out


def model_rfft(lines, prec, groups, order=None):
    """Two real lines a, b as z = a + i b, one n-point transform, split: A[k] = (Z[k] + conj Z[-k]) / 2, B[k] = (Z[k] - conj Z[-k]) / 2i"""
    L, n = lines.shape
    a, b, ia, ib = _pairs(lines.astype(A.RDT[prec]), groups, order)
    Z = _fft(a + 1j * b, prec)
    Zr = np.conj(Z[:, (-np.arange(n)) % n])
    half = A.RDT[prec](0.5)
    ya, yb = ((Z + Zr) * half)[:, :n // 2 + 1], ((Z - Zr) * (-1j * half))[:, :n // 2 + 1]
    return _unpack(L, n // 2 + 1, A.CDT[prec], ia, ib, ya, yb)


def _hermitian(X, n):
    """[P][n/2 + 1] -> [P][n]: the imaginary parts of bin 0 and (n even) bin n/2 ignored"""
    X = np.array(X)
    X[:, 0] = X[:, 0].real
    if n % 2 == 0:
        X[:, -1] = X[:, -1].real
    return np.concatenate([X, np.conj(X[:, (n - 1) // 2:0:-1])], axis=1)


def model_irfft(lines, n, prec, groups, order=None):
    """Two half spectra merged into Z = A + i B, one inverse transform, a = Re z, b = Im z"""
    L = lines.shape[0]
    a, b, ia, ib = _pairs(lines.astype(A.CDT[prec]), groups, order)
    z = _fft(_hermitian(a, n) + 1j * _hermitian(b, n), prec, inverse=True)
    return _unpack(L, n, A.RDT[prec], ia, ib, z.real, z.imag)


def model_r2r(lines, kind, prec, groups, order=None):
    """DCT / DST II and III of two real lines through ONE n-point complex transform (Makhoul's reordering): type II v[j] = x[2j],
    v[n-1-j] = x[2j+1], y[k] = 2 Re(w_k V[k]) with w_k = exp(-i pi k / 2n); type III the transposed steps; the sine kinds through the
    sign and reversal identities of accuracy_ref.ld_r2r."""
    L, n = lines.shape
    rdt, cdt = A.RDT[prec], A.CDT[prec]
    x = lines.astype(rdt)
    alt = ((-1) ** np.arange(n)).astype(rdt)
    if kind == "dst2":
        return model_r2r(x * alt, "dct2", prec, groups, order)[:, ::-1]
    if kind == "dst3":
        return alt * model_r2r(x[:, ::-1], "dct3", prec, groups, order)
    k = np.arange(n)
    w = A.ld_phase(k.astype(np.int64), 4 * n, +1).astype(cdt)          # exp(-2 pi i k / 4n)
    perm = np.concatenate([np.arange(0, n, 2), np.arange(n - 1 - (n % 2), 0, -2)])   # v = x[perm]
    a, b, ia, ib = _pairs(x, groups, order)
    if kind == "dct2":
        Z = _fft(a[:, perm] + 1j * b[:, perm], prec)
        Zr = np.conj(Z[:, (-k) % n])
        Va, Vb = (Z + Zr) * rdt(0.5), (Z - Zr) * (-1j * rdt(0.5))
        return _unpack(L, n, rdt, ia, ib, 2 * (w * Va).real.astype(rdt), 2 * (w * Vb).real.astype(rdt))
    assert kind == "dct3"

    def c(X):                                                          # c[k] = conj(w_k) (X[k] - i X[n-k]), X[n] = 0: Hermitian
        Xr = np.concatenate([np.zeros((X.shape[0], 1), dtype=rdt), X[:, :0:-1]], axis=1)
        return np.conj(w) * (X - 1j * Xr)
    z = _fft(c(a) + 1j * c(b), prec, inverse=True)
    ya, yb = np.empty_like(a), np.empty_like(b)
    ya[:, perm], yb[:, perm] = z.real, z.imag
    return _unpack(L, n, rdt, ia, ib, ya, yb)


def model_rfft2(x, prec, paired, order=None):
    """dfft_rfft2d_batch forward: the rows of all planes flattened through the row model, then n1-point columns"""
    b, n1, n2 = x.shape
    rows = x.reshape(b * n1, n2)
    groups = [range(b * n1)] if paired else [[r] for r in range(b * n1)]
    X = model_rfft(rows, prec, groups, order).reshape(b, n1, n2 // 2 + 1)
    return np.moveaxis(_fft(np.moveaxis(X, 1, -1), prec), -1, 1)


def model_irfft2(X, n2, prec, paired, order=None):
    b, n1, nh = X.shape
    Y = np.moveaxis(_fft(np.moveaxis(X, 1, -1), prec, inverse=True), -1, 1).reshape(b * n1, nh)
    groups = [range(b * n1)] if paired else [[r] for r in range(b * n1)]
    return model_irfft(Y, n2, prec, groups, order).reshape(b, n1, n2)


def _skip2(count):
    """The wrong pairing: lines (0, 2), (1, 3), ... -- line i with line i + 2"""
    head = [j for q in range(0, count - count % 4, 4) for j in (q, q + 2, q + 1, q + 3)]
    return head + list(range(len(head), count))


def _r2r_ref(lines, kind):
    return A.ld_r2r(np.asarray(lines).T[None], kind)[0].T


# ---- the models are the transforms ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 15, 16, 97])
def test_the_models_compute_the_transforms(n):
    x = A.rand_real((5, n), 70 + n)
    X = A.rand_complex((5, n // 2 + 1), 71 + n)
    g = [range(5)]
    assert np.abs(model_rfft(x, "f64", g) - A.ld_rfft(x, 1)).max() < 1e-13 * n
    assert np.abs(model_irfft(X, n, "f64", g) - A.ld_irfft(X, n, 1)).max() < 1e-13 * n
    for kind in A.R2R_KINDS:
        assert np.abs(model_r2r(x, kind, "f64", g) - _r2r_ref(x, kind)).max() < 1e-13 * n, kind
    p = A.rand_real((3, 5, n), 72 + n)
    F = A.ld_fft(A.ld_rfft(p, 2), 1)
    assert np.abs(model_rfft2(p, "f64", True) - F).max() < 1e-12 * n
    P = A.rand_complex((3, 5, n // 2 + 1), 73 + n)
    assert np.abs(model_irfft2(P, n, "f64", True) - A.ld_irfft(A.ld_fft(P, 1, -1), n, 2)).max() < 1e-12 * n


# ---- the partner rules against the models -----------------------------------------------------------------------------------------------
def _touched(model, x, index_of, lines_out, count):
    """line -> the output lines of the model that turn non-finite when that input line is NaN, the line itself left out"""
    out = {}
    for line in range(count):
        with np.errstate(all="ignore"):
            y = lines_out(model(LI.poison(x, index_of(line), "nan")))
        out[line] = {int(v) for v in np.nonzero(LI.nonfinite(y).reshape(count, -1).any(axis=1))[0]} - {line}
    return out


@pytest.mark.parametrize("count", [1, 2, 5, 6])
def test_partner_rule_of_rows(count):
    x = A.rand_real((count, 15), 80)
    got = _touched(lambda v: model_rfft(v, "f64", [range(count)]), x, lambda q: (q,), lambda y: y, count)
    assert got == {q: LI.partners_rows(q, count) for q in range(count)}
    assert LI.partners_rows(count - 1, count) == (set() if count % 2 else {count - 2})     # the odd last row: zeros


@pytest.mark.parametrize("s", [1, 4, 5])
def test_partner_rule_of_columns(s):
    """columns 2c / 2c + 1 inside one [n][s] item; with odd s the last column of item b must NOT pair with the first of item b + 1"""
    batch, n = 3, 15
    x = A.rand_real((batch, n, s), 81)

    def model(v):
        y = model_rfft(LI.lines_cols(v), "f64", [range(b * s, (b + 1) * s) for b in range(batch)])
        return y.reshape(batch, s, n // 2 + 1).transpose(0, 2, 1)
    got = _touched(model, x, lambda q: LI.cols_index(x.shape, q), LI.lines_cols, batch * s)
    assert got == {q: LI.partners_cols(q, batch, s) for q in range(batch * s)}
    if s % 2:
        for b in range(batch - 1):
            assert LI.partners_cols(b * s + s - 1, batch, s) == set() and b * s + s - 1 not in LI.partners_cols((b + 1) * s, batch, s)


@pytest.mark.parametrize("n1,n2,paired", [(5, 15, True), (4, 15, True), (5, 16, False), (3, 15, True), (1, 15, True)])
@pytest.mark.parametrize("direction", [+1, -1])
def test_partner_rule_of_planes(n1, n2, paired, direction):
    """rows pair across planes where n1 is odd and n2 pairs: the last row of an even plane with the first row of the next one"""
    batch = 5
    if direction > 0:
        x = A.rand_real((batch, n1, n2), 82)
        model = lambda v: model_rfft2(v, "f64", paired)   # noqa: E731
    else:
        x = A.rand_complex((batch, n1, n2 // 2 + 1), 83)
        model = lambda v: model_irfft2(v, n2, "f64", paired)   # noqa: E731
    got = _touched(model, x, lambda q: (q,), LI.lines_planes, batch)
    assert got == {p: LI.partners_planes(p, batch, n1, paired) for p in range(batch)}
    if paired and n1 % 2:
        assert LI.partners_planes(0, batch, n1, True) == {1} and LI.partners_planes(4, batch, n1, True) == set()
        # groups of three planes: planes 0-1 and 3-4 couple, plane 2 is the odd last of its group
        assert [LI.partners_planes(p, batch, n1, True, group=3) for p in range(batch)] == [{1}, {0}, set(), {4}, {3}]
    else:
        assert all(LI.partners_planes(p, batch, n1, paired) == set() for p in range(batch))


# ---- the checks on the models, and on a wrong one ---------------------------------------------------------------------------------------
def test_checks_primitives():
    a = np.arange(12, dtype=np.float32).reshape(4, 3)
    b = a.copy()
    b[2, 1] = np.nan
    assert LI.dirty_set(b.astype(LD), {3}) == {2, 3}
    assert LI.same_outside(a, b, {2})
    with pytest.raises(AssertionError, match=r"line 2 changed, \+2 lines from the poisoned line 0"):
        LI.same_outside(a, b, {0, 1}, poisoned=0, what="x")
    z = a.copy()
    z[1, 0] = -0.0 if a[1, 0] == 0 else -a[1, 0]
    c = np.zeros((2, 2), dtype=np.float32)
    d = c.copy()
    d[1, 1] = -0.0                                              # equal as floats, different bytes
    with pytest.raises(AssertionError, match="line 1 changed"):
        LI.same_outside(c, d, set())
    n = np.full((2, 2), np.nan, dtype=np.float32)
    assert LI.same_outside(n, n.copy(), set())                  # NaN == NaN through the integer view
    assert LI.dead_inside(b, LI.nonfinite(b))
    with pytest.raises(AssertionError, match=r"element \(2, 1\) is finite"):
        LI.dead_inside(a, LI.nonfinite(b), "x")
    half = np.array([np.nan + 1j], dtype=np.complex64)
    assert LI.dead_inside(half, np.array([True]))               # one non-finite component is enough
    assert LI.is_zero(np.array([0.0, -0.0])) and not LI.is_zero(np.array([0.0, 1e-300]))
    assert LI.bits_equal(LI.scale_exact(np.array([-0.0 - 1j], dtype=np.complex64), 4.0), np.array([-0.0 - 4j], dtype=np.complex64))
    # nu_pair: a zero partner is allowed, a zero pair is not; equal norms give nu / sqrt 2
    r = A.rand_real((2, 64), 5).astype(LD)
    g = (r[0] * (1 + LD(1e-6))).astype(np.float64)
    solo = LI.nu_pair(g, r[0], None, 64, "f32")
    assert solo == pytest.approx(A.nu(g[None], r[:1], 64, "f32"), rel=1e-12)
    assert LI.nu_pair(g, r[0], np.zeros(64), 64, "f32") == solo
    assert LI.nu_pair(g, r[0], r[0], 64, "f32") == pytest.approx(solo / np.sqrt(2), rel=1e-12)
    with pytest.raises(AssertionError, match="identically zero"):
        LI.nu_pair(np.zeros(4), np.zeros(4, dtype=LD), None, 4, "f64")
    assert LI.poison_lines(5) == [0, 2, 3, 4] and LI.poison_lines(10) == [0, 4, 5, 9] and LI.poison_lines(1) == [0]
    x = A.rand_complex((3, 4), 1)
    assert np.isnan(LI.poison(x, (1,), "nan")[1].real).all() and np.isnan(LI.poison(x, (1,), "nan")[1].imag).all()
    one = LI.poison(x, (1,), "nan1", sample=2)
    assert np.isnan(one).sum() == 1 and np.isnan(one[1, 2])
    assert np.array_equal(LI.poison(x, (2,), "big")[2], x[2] * 2.0 ** 24) and LI.is_zero(LI.poison(x, (0,), "zero")[0])
    assert np.array_equal(LI.poison(x, (0,), "zero")[1:], x[1:]) and x.flags.writeable   # only that line, and a copy


def _row_cases():
    for n in LI.RFFT_ROWS_N:
        yield n, LI.BATCH


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", LI.RFFT_ROWS_N)
def test_rows_model_passes_and_wrong_model_fails(n, prec):
    """rfft / irfft rows of the GPU module on the pairing model: the checks pass and nu_pair stays under the family's bound; the model
    that pairs row i with row i + 2 is rejected by same_outside, which names row 2 (two lines from the poisoned row 0)."""
    L = LI.BATCH
    paired = n not in LI.UNPAIRED_ROWS_N
    groups = [range(L)] if paired else [[r] for r in range(L)]
    partners = (lambda q: LI.partners_rows(q, L)) if paired else LI.partners_none
    fam = LI.real_family(n) if paired else None
    x, _ = A.real_lines(n, L, 1, 2000 + n)
    X, _ = A.half_spectra(n, L, 1, 3000 + n)
    x, X = x[:, :, 0], X[:, :, 0]
    LI.check_case(lambda v: model_rfft(v, prec, groups), lambda v, key: A.ld_rfft(v, 1), x, lambda q: (q,), lambda y: y, partners, prec,
                  f"model rfft n={n}", "cpu rfft rows", fam, n)
    LI.check_case(lambda v: model_irfft(v, n, prec, groups), lambda v, key: A.ld_irfft(v, n, 1), X, lambda q: (q,), lambda y: y, partners,
                  prec, f"model irfft n={n}", "cpu irfft rows", fam, n)
    if paired:
        with pytest.raises(AssertionError, match=r"line 2 changed, \+2 lines from the poisoned line 0"):
            LI.check_case(lambda v: model_rfft(v, prec, groups, _skip2), lambda v, key: A.ld_rfft(v, 1), x, lambda q: (q,), lambda y: y,
                          partners, prec, f"wrong model rfft n={n}", "wrong", fam, n, lines=[0], kinds=("nan",))
    if paired and n > 2:   # (the 2-point inverse has no multiplication: Re and Im never mix, and its sums of float32 values are exact)
        with pytest.raises(AssertionError, match=r"line 2 changed, \+2 lines from the poisoned line 0"):
            LI.check_case(lambda v: model_irfft(v, n, prec, groups, _skip2), lambda v, key: A.ld_irfft(v, n, 1), X, lambda q: (q,),
                          lambda y: y, partners, prec, f"wrong model irfft n={n}", "wrong", fam, n, lines=[0], kinds=("big", "nan"))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("s", LI.STRIDED_S)
@pytest.mark.parametrize("n", LI.STRIDED_N)
def test_columns_model_passes_and_wrong_model_fails(n, s, prec):
    batch = 2
    groups = [range(b * s, (b + 1) * s) for b in range(batch)]
    partners = lambda q: LI.partners_cols(q, batch, s)   # noqa: E731
    fam = LI.real_family(n)
    x, _ = A.real_lines(n, batch, s, 2000 + n)
    X, _ = A.half_spectra(n, batch, s, 3000 + n)

    def fwd(v, order=None):
        return model_rfft(LI.lines_cols(v), prec, groups, order).reshape(batch, s, -1).transpose(0, 2, 1)

    def bwd(v, order=None):
        return model_irfft(LI.lines_cols(v), n, prec, groups, order).reshape(batch, s, -1).transpose(0, 2, 1)
    idx_x, idx_X = (lambda q: LI.cols_index(x.shape, q)), (lambda q: LI.cols_index(X.shape, q))
    LI.check_case(fwd, lambda v, key: A.ld_rfft(v, 1), x, idx_x, LI.lines_cols, partners, prec, f"model rfft n={n} s={s}", "cpu rfft cols", fam, n)
    LI.check_case(bwd, lambda v, key: A.ld_irfft(v, n, 1), X, idx_X, LI.lines_cols, partners, prec, f"model irfft n={n} s={s}", "cpu irfft cols", fam, n)
    with pytest.raises(AssertionError, match=r"line 2 changed, \+2 lines from the poisoned line 0"):
        LI.check_case(lambda v: fwd(v, _skip2), lambda v, key: A.ld_rfft(v, 1), x, idx_x, LI.lines_cols, partners, prec, "wrong model", "wrong",
                      fam, n, lines=[0], kinds=("nan",))
    # a model that pairs columns ACROSS items (the flattened batch) is rejected too where s is odd: column 5 = item 1's first
    if s % 2:
        flat = lambda v: model_rfft(LI.lines_cols(v), prec, [range(batch * s)]).reshape(batch, s, -1).transpose(0, 2, 1)   # noqa: E731
        with pytest.raises(AssertionError, match=rf"line {s} changed, \+1 lines from the poisoned line {s - 1}"):
            LI.check_case(flat, lambda v, key: A.ld_rfft(v, 1), x, idx_x, LI.lines_cols, partners, prec, "flat model", "wrong", fam, n,
                          lines=[s - 1], kinds=("nan",))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n1,n2", LI.RFFT_2D)
def test_planes_model_passes_and_wrong_model_fails(n1, n2, prec):
    """the 2-D route: planes couple exactly where the rule says (odd n1, n2 = 15).  The same model judged by the rule of EVEN n1
    ("none") is rejected: plane 1 changes, one plane from the poisoned one.  (test_planes_wrong_model_fails pairs row i with row i + 2.)"""
    b = LI.PLANES
    paired = n2 == 15
    coupled = paired and n1 % 2 == 1
    partners = lambda q: LI.partners_planes(q, b, n1, paired)   # noqa: E731
    fam = "real" if coupled else None
    x, _ = A.real_planes(n1, n2, b, 4000 + n1)
    X, _ = A.half_planes(n1, n2, b, 5000 + n1)
    LI.check_case(lambda v: model_rfft2(v, prec, paired), lambda v, key: A.ld_fft(A.ld_rfft(v, 2), 1), x, lambda q: (q,), LI.lines_planes,
                  partners, prec, f"model rfft2 {n1}x{n2}", "cpu rfft2", fam, n1 * n2)
    LI.check_case(lambda v: model_irfft2(v, n2, prec, paired), lambda v, key: A.ld_irfft(A.ld_fft(v, 1, -1), n2, 2), X, lambda q: (q,),
                  LI.lines_planes, partners, prec, f"model irfft2 {n1}x{n2}", "cpu irfft2", fam, n1 * n2)
    if coupled:   # the rule for EVEN n1 ("none") applied to this model: plane 1 changes, one plane from the poisoned one
        with pytest.raises(AssertionError, match=r"line 1 changed, \+1 lines from the poisoned line 0"):
            LI.check_case(lambda v: model_rfft2(v, prec, paired), lambda v, key: A.ld_fft(A.ld_rfft(v, 2), 1), x, lambda q: (q,),
                          LI.lines_planes, LI.partners_none, prec, "planes taken for independent", "wrong", None, n1 * n2, lines=[0],
                          kinds=("nan",))


def test_planes_wrong_model_fails():
    x, _ = A.real_planes(1, 15, 5, 4001)
    with pytest.raises(AssertionError, match=r"line 2 changed, \+2 lines from the poisoned line 0"):
        LI.check_case(lambda v: model_rfft2(v, "f64", True, _skip2), lambda v, key: A.ld_fft(A.ld_rfft(v, 2), 1), x, lambda q: (q,),
                      LI.lines_planes, lambda q: LI.partners_planes(q, 5, 1, True), "f64", "wrong planes", "wrong", "real", 15, lines=[0],
                      kinds=("nan",))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", A.R2R_KINDS)
@pytest.mark.parametrize("n", LI.R2R_N)
def test_r2r_model_passes_and_wrong_model_fails(n, kind, prec):
    fam = LI.real_family(n, "r2r")
    L = LI.BATCH
    x = A.r2r_lines(n, L, 1, 6000 + n)[0][:, :, 0]
    ref = lambda v, key: _r2r_ref(v, kind)   # noqa: E731
    LI.check_case(lambda v: model_r2r(v, kind, prec, [range(L)]), ref, x, lambda q: (q,), lambda y: y, lambda q: LI.partners_rows(q, L), prec,
                  f"model {kind} n={n} rows", "cpu r2r rows", fam, n)
    for s in LI.STRIDED_S:
        batch = 2
        groups = [range(b * s, (b + 1) * s) for b in range(batch)]
        xs = A.r2r_lines(n, batch, s, 6000 + n)[0]
        model = lambda v: model_r2r(LI.lines_cols(v), kind, prec, groups).reshape(batch, s, n).transpose(0, 2, 1)   # noqa: E731
        LI.check_case(model, lambda v, key: A.ld_r2r(v, kind), xs, lambda q: LI.cols_index(xs.shape, q), LI.lines_cols,
                      lambda q: LI.partners_cols(q, batch, s), prec, f"model {kind} n={n} s={s}", "cpu r2r cols", fam, n)
    with pytest.raises(AssertionError, match=r"line 2 changed, \+2 lines from the poisoned line 0"):
        LI.check_case(lambda v: model_r2r(v, kind, prec, [range(L)], _skip2), ref, x, lambda q: (q,), lambda y: y,
                      lambda q: LI.partners_rows(q, L), prec, "wrong r2r model", "wrong", fam, n, lines=[0], kinds=("zero", "nan"))


@pytest.mark.parametrize("prec", PRECS)
def test_long_convolution_composed_route_model(prec):
    """dfft_rconv1d_long's composed route: pad to m, the PAIRED real rows of length m (real form 3), multiply, the paired inverse rows,
    truncate -- rows 2p / 2p + 1 of the 6 rows share their transforms; nu_pair under the route's own bound"""
    import rconv1d_cases as RC
    import rconv1d_long_cases as LC
    m, rows, channels = LI.long_length(), 6, 3
    assert LC.split(m) is not None and m > 8192
    n = m // 2 + 1
    x = A.rand_real((rows, n), 9000)
    H = RC.make_filter(channels, m, "complex", 9001)

    def model(v, order=None):
        xp = np.zeros((rows, m), dtype=A.RDT[prec])
        xp[:, :n] = v
        Y = model_rfft(xp, prec, [range(rows)], order) * (H[np.arange(rows) % channels] / m).astype(A.CDT[prec])
        return model_irfft(Y, m, prec, [range(rows)], order)[:, :n]
    partners = lambda q: LI.partners_rows(q, rows)   # noqa: E731
    ref = lambda v, key: RC.reference(v, H, m)   # noqa: E731
    LI.check_case(model, ref, x, lambda q: (q,), lambda y: y, partners, prec, f"model rconv1d_long m={m}", "cpu rconv1d_long composed", LC.BOUND, m,
                  lines=[0, 5])
    with pytest.raises(AssertionError, match=r"line 2 changed, \+2 lines from the poisoned line 0"):
        LI.check_case(lambda v: model(v, _skip2), ref, x, lambda q: (q,), lambda y: y, partners, prec, "wrong model", "wrong", LC.BOUND, m,
                      lines=[0], kinds=("nan",))


@pytest.mark.parametrize("prec", PRECS)
def test_unpaired_model_passes_and_coupled_model_fails(prec):
    """plain per-line transforms (the unpaired families): exactly 2^24 times the clean line under "big", exactly zero under "zero"; a
    model that leaks 2^-30 of line i + 2 into line i fails same_outside under "big" although every value still rounds the same under nu"""
    x, _ = A.complex_lines(16, (5, 16), 1, 1016)
    ref = lambda v, key: A.ld_fft(v, 1, +1)   # noqa: E731
    LI.check_case(lambda v: _fft(v, prec), ref, x, lambda q: (q,), lambda y: y, LI.partners_none, prec, "plain rows", "cpu rows")

    def leaky(v):
        y = _fft(v, prec)
        y[:3] += y[2:] * A.RDT[prec](2.0 ** -30)
        return y
    with pytest.raises(AssertionError, match=r"line 0 changed, -2 lines from the poisoned line 2"):
        LI.check_case(leaky, ref, x, lambda q: (q,), lambda y: y, LI.partners_none, prec, "leaky rows", "wrong", lines=[2], kinds=("big",))


def test_print_worst():
    for (label, prec), (value, what) in sorted(LI.WORST.items()):
        if label != "wrong":
            print(f"line isolation worst {label} {prec}: nu_pair {value:.3f}  {what}")
