"""The case tables of the tuned-length sweep (tests/test_tuned_sweep_host.py, tests/test_gpu_tuned_sweep.py): for every kernel family that
is instantiated once per entry of DFFT_PLAN_TABLE (csrc/dfft_plans.h), the lengths it is instantiated for, the (length, precision,
variant) triples its route rule sends to the composed form (ROUTED), and the smallest shapes that run every template variant of the
instantiation.  No GPU, no scipy, no library call: the host test holds every table here against the source and the library.

The plan table is read from the header, never copied: a new X(...) line without a sweep entry fails the host test.  Inputs and
longdouble references come from the generators the other modules already use (accuracy_ref, rconv1d_cases, rconv1d_os_cases,
stft_cases), called with the swept length; inputs hold float32 values, so both precisions share one reference.

Variants.  Most fused kernels exist in a form that moves two reals per access (VEC: every size the addresses depend on is even) and a
per-real form.  Every family's cases reach both forms at every length, which for odd half-lengths needs a case beyond the base shapes:
    rconv1d       n = m (even: VEC, the circular case); n = M - 1 (1 where M = 2); and where M - 1 is even (odd M), n = M as well, so
                  the per-real form runs with the cut inside a pair.
    overlap-save  d = M with n = n_out = 2 S + S / 2 (a ragged last block); an odd d (M - 1, or M - 2 where M is odd); and where the
                  first case is not all-even (odd M, or an odd n), an all-even case (d = M or M - 1, n rounded up to even) for VEC.
    STFT          the base case of stft_cases (hop = m / 4, pad = M, n = 3 m + 2); hop + 1 where hop is even (no two-real loads); and
                  where hop or pad is odd, an all-even case (hop + 1, pad = M or M - 1) for VEC.
"""
import re
from functools import lru_cache
from pathlib import Path

import numpy as np

import accuracy_ref as A
import rconv1d_cases as RC
import rconv1d_os_cases as RCO
import stft_cases as SC

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "distributedfft_amd" / "csrc"
PRECS = A.PRECS
CODE = {"f64": 0, "f32": 1}
FILTER_CODE = {"complex": 0, "real": 1}
R2R_CODE = {"dct2": 0, "dct3": 1, "dst2": 2, "dst3": 3}          # DFFT_R2R_* of include/dfft.h (the host test checks them)
FAMILIES = ("real_rows", "real_pair", "real_cols", "r2r", "bluestein", "rconv", "osconv", "stft")


def plan_lengths(text=None):
    """The lengths of DFFT_PLAN_TABLE, ascending (the regex of rconv1d_cases.plan_points / test_real_strided_host.py)"""
    if text is None:
        return sorted(RC.plan_points())
    return sorted(int(n) for n, _ in re.findall(r"^\s*X\((\d+),\s*\d+,\s*(\d+),", text, re.M))


PLAN = plan_lengths()


# ---- which entries a family instantiates ------------------------------------------------------------------------------------------------
# family -> (source file, instantiation macro).  The macro's line reads "template struct XInst<(GRP == DFFT_INST_GROUP [&& gate]), N>":
# the host test reads the gate from there and evaluates it with GATES.  The families of the shared scaffold (dfft_fused_host.h) have one
# macro, DFFT_FUSED_INST, which each unit expands through DFFT_FUSED_INSTANTIATE(<its tag>): FUSED_UNITS names the unit and the tag.
FUSED = ("dfft_fused_host.h", "DFFT_FUSED_INST")
INSTANTIATION = {
    "real_rows": ("dfft_real.hip", "DFFT_REAL_INST"),
    "real_pair": ("dfft_real_pair.hip", "DFFT_PAIR_INST"),
    "real_cols": FUSED,
    "r2r":       FUSED,
    "bluestein": ("dfft_bluestein.hip", "DFFT_BS_INST"),
    "rconv":     FUSED,
    "osconv":    FUSED,
    "stft":      FUSED,
    # not swept here (the conv modules run all of their lengths), but held to the same reading of the source
    "conv_x":       ("dfft_conv.hip", "DFFT_XC_INST"),
    "conv_x_multi": ("dfft_conv_multi.hip", "DFFT_XM_INST"),
}
FUSED_UNITS = {"real_cols": ("dfft_real_cols.hip", "ColsTag"), "r2r": ("dfft_r2r.hip", "R2rTag"), "rconv": ("dfft_rconv.hip", "RconvTag"),
               "osconv": ("dfft_osconv.hip", "OsconvTag"), "stft": ("dfft_stft.hip", "StftTag")}


def source_constant(name, file):
    """`constexpr int name = value;` (or long long) of a source file"""
    return int(re.search(r"constexpr\s+(?:int|long long)\s+" + name + r"\s*=\s*(\d+)\s*;", (CSRC / file).read_text()).group(1))


def conv_fused_lengths():
    """The lengths conv_fused_n (dfft_conv_impl.h) names"""
    body = re.search(r"constexpr bool conv_fused_n\(int n\) \{ return ([^;]+); \}", (CSRC / "dfft_conv_impl.h").read_text()).group(1)
    parts = [p.strip() for p in body.split("||")]
    assert all(re.fullmatch(r"n == \d+", p) for p in parts), body
    return sorted(int(p[5:]) for p in parts)


GATES = {
    "": lambda n: True,
    "N % 2 == 1": lambda n: n % 2 == 1,
    "N >= kFusedMinM": lambda n: n >= source_constant("kFusedMinM", "dfft_bluestein.hip"),
    "conv_fused_n(N)": lambda n: n in conv_fused_lengths(),
}


def instantiation_gate(family):
    """The gate text of the family's instantiation macro ("" where every entry is instantiated)"""
    file, macro = INSTANTIATION[family]
    line = re.search(r"#define " + macro + r"\(N, GRP, E, \.\.\.\) template struct \w+<(?:\w+, )?\(GRP == DFFT_INST_GROUP(?: && ([^)]*(?:\([^)]*\))?[^)]*))?\), N>;",
                     (CSRC / file).read_text())
    assert line, (family, "the instantiation macro is not where the sweep reads it")
    if INSTANTIATION[family] == FUSED:   # ... and the unit expands it, once, for its own tag, in its instantiation groups
        unit, tag = FUSED_UNITS[family]
        assert len(re.findall(r"^DFFT_FUSED_INSTANTIATE\(" + tag + r"\)$", (CSRC / unit).read_text(), re.M)) == 1, (family, unit)
    return (line.group(1) or "").strip()


def instantiated(family, lengths=None):
    """The plan-table entries the family's source instantiates"""
    gate = instantiation_gate(family)
    assert gate in GATES, (family, gate, "a gate the sweep does not know: teach GATES and the sweep tables")
    return [n for n in (PLAN if lengths is None else lengths) if GATES[gate](n)]


# ---- Bluestein: the non-smooth n that reaches a padded length ---------------------------------------------------------------------------
BLUESTEIN_MIN_M = 21          # kFusedMinM of dfft_bluestein.hip (the host test reads it from the source)
BLUESTEIN_MAX_N = 2048        # kBluesteinFusedMaxLength of dfft_bluestein.h


def seven_smooth(n):
    for p in (2, 3, 5, 7):
        while n % p == 0:
            n //= p
    return n == 1


def bluestein_padded(n, lengths=None):
    """The smallest tuned length >= 2 n - 1 (bluestein_padded_length for 1 < n <= 2048)"""
    return next(m for m in (PLAN if lengths is None else lengths) if m >= 2 * n - 1)


def bluestein_reach(lengths=None):
    """M -> the largest n <= 2048 of length kind 3 (not 7-smooth) whose padded length is M"""
    out = {}
    for n in range(2, BLUESTEIN_MAX_N + 1):
        if not seven_smooth(n):
            out[bluestein_padded(n, lengths)] = n
    return out


BLUESTEIN_N = bluestein_reach()
# M is reached by the n with P < 2 n - 1 <= M, P the tuned length before M, i.e. (P + 1) / 2 < n <= (M + 1) / 2; at these five every such
# n is 7-smooth and runs the single-pass kernels instead:
#   27 (P = 25): n = 14            32 (P = 27): n = 15, 16         49 (P = 48): n = 25
#   100 (P = 96): n = 49, 50       128 (P = 125): n = 64
# Below 21 nothing is instantiated, and nothing would be reached: M <= 16 needs n <= 8, and every n <= 10 is 7-smooth.
BLUESTEIN_UNREACHABLE = [27, 32, 49, 100, 128]


# ---- lengths and routes -----------------------------------------------------------------------------------------------------------------
LENGTHS = {
    "real_rows": list(PLAN),                                    # M: n = 2 M
    "real_pair": [n for n in PLAN if n % 2 == 1],
    "real_cols": list(PLAN),
    "r2r":       list(PLAN),
    "bluestein": sorted(BLUESTEIN_N),                           # M >= 21 that some n reaches
    "rconv":     list(PLAN),                                    # M: m = 2 M
    "osconv":    list(PLAN),
    "stft":      list(PLAN),
}

REAL_COLS_S = (6, 7, 34)             # VEC with a ragged tile; scalar with an odd last column; whole tiles plus a ragged one
# fp32 n = 2048: multi_pass_faster goes multi-pass where the 8-pair tiles per row, ceil(ceil(s / 2) / 8), are even in number.  s = 40 has
# 20 pairs in 3 tiles (fused, as 6, 7 and 34 with 1, 1 and 3 tiles); s = 24 has 12 pairs in 2 tiles: the multi-pass side.
REAL_COLS_S_EXTRA = {2048: (40, 24)}
R2R_FORMS = {"rows": 1, "cols_vec": 6, "cols": 7}               # form -> s
R2R_FORM_OF_S = {s: f for f, s in R2R_FORMS.items()}
R2R_THREE = {"dct2": False, "dct3": True, "dst2": False, "dst3": True}

# (length, precision, variant...) on the composed form although the length is tuned.  Variants: real_cols s; r2r (type III?, form).
ROUTED = {
    "real_rows": set(),
    "real_pair": set(),
    # multi_pass_faster (dfft_real_cols.hip): measured faster, every s -- and fp32 2048 by the parity of its tile count
    "real_cols": ({(n, "f64", s) for n in (2401, 4096) for s in REAL_COLS_S} |
                  {(n, "f32", s) for n in (2187, 2401, 3125, 4096) for s in REAL_COLS_S} | {(2048, "f32", 24)}),
    # r2r_fused_ok (dfft_r2r.hip): instantiations that would spill
    "r2r": ({(n, "f64", True, form) for n in (100, 384, 400, 3125) for form in ("cols", "rows")} | {(1536, "f64", True, "rows")} |
            {(2048, "f64", False, "cols"), (3125, "f64", False, "rows"), (3125, "f32", True, "rows")}),
    "bluestein": set(),          # kFusedMinM routes M < 21, which no Bluestein length reaches (above)
    "rconv":  {(3125, "f64"), (3125, "f32"), (1536, "f64")},                       # rconv_fused_ok
    "osconv": {(3125, "f64"), (3125, "f32"), (1536, "f64"), (2401, "f32")},        # osconv_fused_ok
    "stft":   {(2401, "f64"), (3125, "f64")},                                      # stft_fused_ok
}
# The routed instantiations that exist only because the fused kernel would spill, and a neighbouring fused length that runs the composed
# route under the family's switch: family -> (environment switch, length)
COMPOSED_NEIGHBOUR = {"r2r": ("DFFT_R2R_FUSED", 2401), "rconv": ("DFFT_RCONV_FUSED", 2401), "osconv": ("DFFT_RCONV_FUSED", 2187),
                      "stft": ("DFFT_STFT_FUSED", 2187)}


def route(family, length, prec, *variant):
    """"fused" or "composed": what the case is there for"""
    assert length in LENGTHS[family], (family, length)
    return "composed" if (length, prec) + tuple(variant) in ROUTED[family] else "fused"


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
ROWS = 5                      # real rows: a ragged last thread group wherever G > 5, one workgroup per row where G = 1; an odd last pair


def _scaled_rows(x, F):
    """Row i times 2^s_i (exact): a row that picks up part of its neighbour fails on its own norm"""
    sc = A.line_scales(x.shape[0])
    return x * sc.reshape((-1,) + (1,) * (x.ndim - 1)), F * sc.astype(A.LD).reshape((-1,) + (1,) * (F.ndim - 1))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@lru_cache(maxsize=4)
def real_rows_case(n, scaled):
    """-> (x [5][n], rfft [5][n/2+1], X [5][n/2+1], n irfft(X) [5][n]).  scaled: the rows carry different scales (not for the pair kernels,
    whose two rows share one transform)."""
    x, F = A.real_lines(n, ROWS, 1, 41000 + n)
    X, b = A.half_spectra(n, ROWS, 1, 42000 + n)
    x, F, X, b = x[:, :, 0], F[:, :, 0], X[:, :, 0], b[:, :, 0]
    if scaled:
        x, F = _scaled_rows(x, F)
        X, b = _scaled_rows(X, b)
    return _frozen(np.ascontiguousarray(x), np.ascontiguousarray(F), np.ascontiguousarray(X), np.ascontiguousarray(b))


def real_cols_s(n):
    return REAL_COLS_S + REAL_COLS_S_EXTRA.get(n, ())


def real_cols_case(n, s):
    """-> (x [2][n][s], rfft along 1, X [2][n/2+1][s], n irfft(X) along 1); equal line scales: two columns share one transform"""
    return A.real_lines(n, 2, s, 43000 + n) + A.half_spectra(n, 2, s, 44000 + n)


def r2r_case(n, s):
    """-> (x [2][n][s], dct2, dct3, dst2, dst3 along 1)"""
    return A.r2r_lines(n, 2, s, 45000 + n)


def bluestein_cases(M):
    """-> n, then (shape, axis, x, F) for the rows kernel ([3][n]) and the cols kernel ([2][n][3]); backward: A.reverse_bins(F, [axis])"""
    n = BLUESTEIN_N[M]
    out = []
    for shape in ((3, n), (2, n, 3)):
        x, F = A.complex_lines(n, shape, 1, 46000 + n)
        out.append((shape, 1, x, F))
    return n, out


RCONV_CHANNELS = 3


def rconv_n_values(M):
    m = 2 * M
    ns = [m, M - 1 if M > 2 else 1]
    if M > 2 and (M - 1) % 2 == 0:
        ns.append(M)
    return ns


def rconv_cases(M):
    """(n, kind, batch) of the half-length; the data: RC.case(M, n, 3, batch, kind)"""
    batch = RC.batch_for(M, RCONV_CHANNELS)
    return [(n, kind, batch) for n in rconv_n_values(M) for kind in RC.KINDS]


def _ragged(S):
    return 2 * S + S // 2


def osconv_shapes(M):
    """(d, n) with n_out = n"""
    m = 2 * M
    shapes = [(M, _ragged(M))]
    d_odd = M - 1 if (M - 1) % 2 else max(1, M - 2)
    shapes.append((d_odd, _ragged(m - d_odd)))
    if M % 2 or _ragged(M) % 2:
        d = M - M % 2
        n = _ragged(m - d)
        shapes.append((d, n + n % 2))
    return shapes


def osconv_vec(d, n):
    return d % 2 == 0 and n % 2 == 0


def osconv_cases(M):
    """(d, n, n_out, channels, batch, kind); the data: RCO.case(M, *that)"""
    return [(d, n, n, 3, 2, kind) for d, n in osconv_shapes(M) for kind in RCO.KINDS]


def stft_shapes(M):
    """(M, hop, pad, n, window) of stft_cases.forward_case"""
    base = SC._base(M)
    _, hop, pad, n, w = base
    shapes = [base]
    if hop % 2 == 0:
        shapes.append((M, hop + 1, pad, n, w))
    if hop % 2 or pad % 2:
        shapes.append((M, hop + hop % 2, pad - pad % 2, n, w))
    return shapes


def stft_vec(shape):
    _, hop, pad, n, _ = shape
    return hop % 2 == 0 and pad % 2 == 0 and n % 2 == 0


def stft_cases(M):
    """(shape, mode, kind): every shape in both pad modes and both output kinds"""
    return [(shape, mode, kind) for shape in stft_shapes(M) for mode in SC.MODES for kind in SC.KINDS]
