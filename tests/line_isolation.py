"""Which lines of a batch may influence which (tests/test_line_isolation_host.py, tests/test_gpu_line_isolation.py): one line of an otherwise
clean case is poisoned -- all NaN, one NaN, times 2^24, or zero -- and the result is compared with the clean run's.  What may change is
decided here from the documentation (include/dfft.h, DESIGN.md "Which lines share arithmetic"), never from the code under test:

    dirty(case, poisoned line) = lines whose longdouble reference on the poisoned input is non-finite  +  the documented partner(s)

Every line outside `dirty` must be BIT-identical to the clean run (same_outside), every output element whose reference is non-finite
must have a non-finite component (dead_inside), and the lines of a paired family are judged relative to their pair's combined norm
(nu_pair) against the family's existing accuracy_ref.BOUND entry -- no constant of its own.

A line is addressed by its index in the flattened batch: rows of (..., n) by the flattened leading dimensions, columns of [batch][n][s]
by b * s + c, planes of [batch][n1][n2] by the plane.  The *_index functions give the numpy index of a line in the input, the lines_*
functions the output as [lines][elements of a line].

A plain module: no conftest, no pytest settings, works on numpy arrays and device tensors alike (tensors are copied to the host)."""
import numpy as np

import accuracy_ref as A

LD, CLD = A.LD, A.CLD
KINDS = ("nan", "big", "zero")    # "nan1" (one sample) only where a family has locality inside a row
BIG = 2.0 ** 24                   # exact, far above line_scales' 2^+-8, no overflow in fp32 at the lengths of the tests


def to_numpy(a):
    """numpy array of a numpy array or a (device) tensor"""
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


# ---- poison ---------------------------------------------------------------------------------------------------------------------------
def poison(x, index, kind, sample=None):
    """A writable copy of x whose line x[index] (basic indexing: a view) is poisoned.  nan: every sample NaN, both components of complex
    data; nan1: only element `sample` of the line; big: the line times 2^24; zero: the line identically zero."""
    y = np.array(x, order="C")
    nan = complex(np.nan, np.nan) if np.iscomplexobj(y) else np.nan
    if kind == "nan":
        y[index] = nan
    elif kind == "nan1":
        line = y[index]
        assert line.base is not None and sample is not None, "nan1 needs a view of one line and a sample"
        line[sample] = nan
    elif kind == "big":
        y[index] = y[index] * BIG
    elif kind == "zero":
        y[index] = 0
    else:
        raise ValueError(kind)
    return y


def poison_lines(count):
    """The first line, an interior even line, its odd neighbour and the last line"""
    mid = max(0, (count // 2) & ~1)
    return sorted({0, mid, min(mid + 1, count - 1), count - 1})


# ---- where a line lives ---------------------------------------------------------------------------------------------------------------
def rows_index(shape, line):
    """Row `line` of (..., n): the flattened leading dimensions"""
    return tuple(int(v) for v in np.unravel_index(line, shape[:-1]))


def cols_index(shape, line):
    """Column b * s + c of [batch][n][s]"""
    b, c = divmod(line, shape[2])
    return (b, slice(None), c)


def planes_index(shape, line):
    return (line,)


def lines_rows(a):
    a = to_numpy(a)
    return a.reshape(-1, a.shape[-1])


def lines_cols(a):
    a = to_numpy(a)
    return np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(a.shape[0] * a.shape[2], a.shape[1])


def lines_planes(a):
    a = to_numpy(a)
    return a.reshape(a.shape[0], -1)


# ---- the documented partner rules (include/dfft.h) ------------------------------------------------------------------------------------
def partners_none(line):
    """fft1d_rows / fft1d_cols / fft1d_any / fft2d_batch, real form 1 rows, rconv1d, rconv1d_os, rconv1d_long, stft, istft"""
    return set()


def partners_rows(line, count):
    """dfft_rfft1d forms 2 and 3, dfft_r2r1d_strided with s = 1: rows 2p and 2p + 1 of the flattened batch share one transform; an odd
    last row is paired with zeros"""
    q = line ^ 1
    return {q} if q < count else set()


def partners_cols(line, batch, s):
    """dfft_rfft1d_strided / dfft_r2r1d_strided with s > 1: columns 2c and 2c + 1 inside one [n][s] item; an odd last column is paired with
    zeros, never with the first column of the next item"""
    b, c = divmod(line, s)
    assert b < batch
    q = c ^ 1
    return {b * s + q} if q < s else set()


def partners_planes(plane, batch, n1, paired, group=None):
    """dfft_rfft2d_batch: the rows of a plane GROUP (all `batch` planes unless the bins exceed 256 MiB) go through dfft_rfft1d's row
    transform flattened, so for n2 of real form 2 or 3 (`paired`) rows 2p and 2p + 1 of group_planes * n1 rows pair up: with odd n1 the
    last row of an even plane of the group shares a transform with the first row of the next plane, and the column pass spreads that
    over the plane.  Even n1, or n2 of real form 1: none."""
    if not paired:
        return set()
    group = batch if group is None else group
    g0 = plane // group * group
    rows = min(group, batch - g0) * n1
    out = set()
    for r in range((plane - g0) * n1, (plane - g0 + 1) * n1):
        if (r ^ 1) < rows:
            out.add(g0 + (r ^ 1) // n1)
    return out - {plane}


# ---- the expected dirty set and the two checks -----------------------------------------------------------------------------------------
def nonfinite(ref):
    """Element mask of a reference: numpy propagates NaN, so the reference itself says what must die"""
    return ~np.isfinite(to_numpy(ref))


def dirty_set(ref_poisoned, partners):
    """ref_poisoned [lines][...]: the longdouble reference on the poisoned input; partners: the documented partner lines"""
    bad = nonfinite(ref_poisoned)
    dead = np.nonzero(bad.reshape(bad.shape[0], -1).any(axis=1))[0]
    return {int(v) for v in dead} | {int(v) for v in partners}


def _bits(a):
    """[lines][integers]: the bytes of every line through an integer view (a NaN never compares equal as a float, -0.0 always does)"""
    a = np.ascontiguousarray(to_numpy(a))
    size = a.dtype.itemsize // (2 if np.iscomplexobj(a) else 1)
    return a.view({4: np.uint32, 8: np.uint64}[size]).reshape(a.shape[0], -1)


def bits_equal(a, b):
    """mem_contract.bits_equal on host arrays: same dtype, same shape, same bytes"""
    a, b = to_numpy(a), to_numpy(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.array_equal(_bits(a.reshape(1, -1)), _bits(b.reshape(1, -1))))


def same_outside(got_clean, got_poisoned, dirty, poisoned=None, what=""):
    """Every line outside `dirty` holds the same bytes in the clean run and in the poisoned run ([lines][...] each).  On failure the
    assertion names the first offending line and its distance from the poisoned one."""
    c, p = to_numpy(got_clean), to_numpy(got_poisoned)
    assert c.shape == p.shape and c.dtype == p.dtype, (c.shape, p.shape, c.dtype, p.dtype)
    changed = np.nonzero((_bits(c) != _bits(p)).any(axis=1))[0]
    bad = [int(v) for v in changed if int(v) not in dirty]
    if bad:
        where = "" if poisoned is None else f", {bad[0] - poisoned:+d} lines from the poisoned line {poisoned}"
        raise AssertionError(f"{what}: line {bad[0]} changed{where}; it is outside the dirty set {sorted(dirty)} "
                             f"({len(bad)} such lines: {bad[:8]})")
    return True


def dead_inside(got_poisoned, must_die, what=""):
    """Every output element whose reference is non-finite (`must_die`, an element mask of got's shape) has a non-finite component: no NaN
    is swallowed by an fmax, a compare-select or a skipped tile."""
    g, m = to_numpy(got_poisoned), np.asarray(must_die, dtype=bool)
    assert g.shape == m.shape, (g.shape, m.shape)
    alive = m & np.isfinite(g)
    if alive.any():
        first = tuple(int(v) for v in np.argwhere(alive)[0])
        raise AssertionError(f"{what}: element {first} is finite ({g[first]}) where the reference is not; {int(alive.sum())} of {int(m.sum())} such elements")
    return True


def scale_exact(a, factor):
    """a times a power of two, component by component (a complex product would add signed zeros)"""
    a = np.ascontiguousarray(to_numpy(a))
    if not np.iscomplexobj(a):
        return a * a.dtype.type(factor)
    r = a.view(a.real.dtype)
    return (r * r.dtype.type(factor)).view(a.dtype)


def is_zero(a):
    """identically zero, of either sign"""
    return bool(np.all(to_numpy(a) == 0))


# ---- the pair measure -----------------------------------------------------------------------------------------------------------------
def _norm2(v):
    v = np.asarray(v)
    return np.sum(v.real.astype(LD) ** 2 + v.imag.astype(LD) ** 2)


def nu_pair(got, ref, partner_ref, n_eff, prec):
    """||got - ref||_2 / sqrt(||ref||^2 + ||partner_ref||^2) / (eps sqrt(log2 n_eff)) of ONE line: the pair's complex line a + i b has
    norm^2 ||a||^2 + ||b||^2 and its transform obeys the family's bound relative to that norm; the split adds O(1) eps.  partner_ref
    None or zero: the line paired with zeros.  A zero PAIR is refused."""
    got, ref = to_numpy(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = got.astype(CLD if np.iscomplexobj(ref) or np.iscomplexobj(got) else LD) - ref
    den = _norm2(ref) + (0 if partner_ref is None else _norm2(partner_ref))
    assert den > 0, "the pair is identically zero"
    return float(np.sqrt(_norm2(d) / den) / (A.EPS[prec] * np.sqrt(np.log2(max(n_eff, 2)))))


WORST = {}   # (family label, prec) -> (worst nu_pair, case) of this process


def check_pair(label, family, prec, value, what):
    """Print the figure, keep the worst per label, and hold it against accuracy_ref.BOUND[family] (family a dict: that route's own
    existing bound per precision, where accuracy_ref has no entry for it)"""
    print(f"line isolation {label} {prec} {what}: nu_pair {value:.3f}")
    if value > WORST.get((label, prec), (-1.0, ""))[0]:
        WORST[(label, prec)] = (value, what)
    bound = (family if isinstance(family, dict) else A.BOUND[family])[prec]
    assert value <= bound, (label, family, prec, what, value, bound)


# ---- one case, every poisoned line and kind ---------------------------------------------------------------------------------------------
def check_case(run, ref, x, index_of, lines_out, partners, prec, what, label, family=None, n_eff=None, lines=None, kinds=KINDS):
    """x: the clean input; run(x) -> the result of the code under test; ref(x, key) -> the longdouble reference (key: None for the clean
    input, else (line, kind): the caller may cache); index_of(line) -> numpy index of input line `line`; lines_out(y) -> [lines][...];
    partners(line) -> the documented partner lines.  family: the accuracy_ref.BOUND entry of a paired family (every line is then judged
    with nu_pair under "big" and "zero"), None for an unpaired one (the poisoned line is then exactly 2^24 times the clean result under
    "big" and exactly zero under "zero").  Returns the number of poisoned runs."""
    clean = lines_out(run(x))
    count = clean.shape[0]
    runs = 0
    for line in (poison_lines(count) if lines is None else lines):
        for kind in kinds:
            tag = f"{what} line {line} {kind}"
            xp = poison(x, index_of(line), kind)
            got = lines_out(run(xp))
            with np.errstate(all="ignore"):
                rp = lines_out(ref(xp, (line, kind)))
            assert got.shape == rp.shape == clean.shape, (got.shape, rp.shape, clean.shape)
            mates = set(partners(line))
            dirty = dirty_set(rp, mates | {line})
            same_outside(clean, got, dirty, line, tag)
            dead_inside(got, nonfinite(rp), tag)
            runs += 1
            if kind == "nan":
                assert np.all(nonfinite(rp[line])), f"{tag}: the reference of the poisoned line is not NaN throughout"
                continue
            assert not nonfinite(rp).any(), f"{tag}: a finite input gave a non-finite reference"
            if family is None:
                if kind == "big":
                    assert bits_equal(got[line], scale_exact(clean[line], BIG)), f"{tag}: not exactly 2^24 times the clean result"
                else:
                    assert is_zero(got[line]), f"{tag}: a zero line gave a non-zero result"
                continue
            for q in range(count):                    # every line, each relative to its own pair
                mate = sorted(partners(q))
                assert len(mate) <= 1, (q, mate)
                pr = rp[mate[0]] if mate else None
                if _norm2(rp[q]) + (0 if pr is None else _norm2(pr)) == 0:
                    assert is_zero(got[q]), f"{tag}: a zero pair gave a non-zero result in line {q}"
                    continue
                check_pair(label, family, prec, nu_pair(got[q], rp[q], pr, n_eff, prec), f"{tag} line {q}")
    return runs


# ---- the paired cases both test modules run ----------------------------------------------------------------------------------------------
BATCH = 5                                            # rows: pairs (0, 1), (2, 3) and row 4 with zeros
RFFT_ROWS_N = [16, 2, 15, 125, 97, 15625]            # real form 1 (unpaired) | form 2 | form 3: Bluestein, four-step
STRIDED_N = [16, 15, 97, 512]                        # dim 1 of (2, n, s)
STRIDED_S = [4, 5]
RFFT_2D = [(8, 16), (5, 16), (4, 15), (5, 15)]       # n2 = 16: form 1; n2 = 15 with odd n1: rows pair across planes
PLANES = 3
R2R_N = [16, 15, 97]
BLUESTEIN_N = {97}                                   # the lengths above of length kind 3
UNPAIRED_ROWS_N = {16}                               # the lengths of RFFT_ROWS_N of real form 1


def long_length():
    """The smallest padded length of dfft_rconv1d_long past 8192 (rconv1d_long_cases.split restates the library's rule)"""
    import rconv1d_long_cases as LC
    m = 8194
    while LC.split(m) is None:
        m += 2
    return m


def real_family(n, name="real"):
    """The accuracy_ref.BOUND entry of a paired real route of length n"""
    return name + "-bluestein" if n in BLUESTEIN_N else name
