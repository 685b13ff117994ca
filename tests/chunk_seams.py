"""The table behind tests/test_chunk_cap_host.py and tests/test_gpu_chunk_seams.py: one small problem (a *seam*) per composed route and
chunk seam, run with the chunk cap unset (one chunk) and under caps that cut it into three or more chunks.  No GPU is needed to import it.

Every plan-less route that works through scratch cuts its batch into chunks of at most max(cap, one unit) bytes (chunk_units of
csrc/dfft_fused_host.h; cap = 256 MiB, or DFFT_SCRATCH_CHUNK_BYTES read once per call).  The chunk loops carry the index arithmetic a
one-chunk call never runs: the unit offset into in / out / the filter, the `row0 % channels` start of the accumulating kernels, the
`first` flag that starts a sum, the ragged last chunk, the half-empty last pair of a paired route.  The seams below are the smallest
problems at which each of these exists.

A seam wraps an op of tests/call_mix.py (inputs, the raw call, the entry point's own lease query, the family's longdouble reference,
measure and bound -- nothing here sets a tolerance) and adds the mirror of its chunk rule: the bytes of one unit as the cap counts them,
the number of units, the lease under a cap, and the caps to run (in units per chunk)."""
import accuracy_ref as A
import call_mix as CM
import large_extent as LE
import rconv1d_long_cases as LC
import rxspec1d_long_cases as XL

ENV = "DFFT_SCRATCH_CHUNK_BYTES"
DEFAULT_CAP = LE.SCRATCH_CAP
LONG_M = 10240                      # 64 x 80: the smallest padded length of the long families with both routes in both precisions
SHAPE = (50, 3, 7)                  # n, channels, batch of the short convolutions and cross-spectra: 21 rows
OS_SHAPE = (2, 3)                   # channels, batch of the overlap-save seams: 6 rows of 4 blocks
LONG_ROWS = (3, 3)                  # batch, channels of the long seams: 9 rows


def _lib():
    from distributedfft_amd import _lib as L
    return L.load()


def bluestein_M(n):
    """The padded length of a Bluestein n (0: n is not one) -- host arithmetic of the library"""
    lib = _lib()
    return int(lib.dfft_bluestein_length(n)) if lib.dfft_length_kind(n) == 3 else 0


def bluestein_fused(n, s, switches):
    """dfft_bluestein.hip bluestein_runs_fused under the seam's switches"""
    return str(switches.get("DFFT_BLUESTEIN_FUSED", 1)) != "0" and n <= 2048 and (s <= 1 or n * s < 1 << 31)


class Seam:
    """`op`: the call-mix op (its switches exclude the cap).  `unit_bytes` / `units`: the chunk rule's unit and how many the call has.
    `lease(cap)`: the mirror of the call's lease under `cap` bytes.  `caps`: {label: units per chunk} of the several-chunk runs.
    `exact`: the chunked result is the one-chunk result bit for bit (units are independent, or a sum is taken in unit order whatever the
    cut); else `sums` = (m, n, channels, batch, order, autos) tells the GPU test how to add the chunks' own sums.  `inplace`: out is x."""

    def __init__(self, family, op, unit, unit_bytes, units, lease, caps, exact=True, inplace=False, sums=None, query=True, whole_pairs=False):
        self.family, self.op, self.unit, self._unit_bytes, self.units = family, op, unit, unit_bytes, int(units)
        self._lease, self.caps, self.exact, self.inplace, self.sums = lease, dict(caps), exact, inplace, sums
        self.whole_pairs = whole_pairs   # the composed long routes: a chunk that is not the whole call holds whole pairs of rows
        self.query = query          # the lease comes from a dfft_*_scratch_bytes query of the entry point (else: from call_mix's rule)
        self.name = f"{family}:{op.name}" + ("-inplace" if inplace else "")

    def __repr__(self):
        return self.name

    @property
    def unit_bytes(self):
        """(a callable where the library has to tell a length first: resolved on first use)"""
        if callable(self._unit_bytes):
            self._unit_bytes = self._unit_bytes()
        return int(self._unit_bytes)

    def cap_bytes(self, label):
        """The cap of a labelled run: that many whole units (a half unit more where the label says so never changes the cut)"""
        return int(self.caps[label] * self.unit_bytes)

    def per_chunk(self, cap=None):
        cap = DEFAULT_CAP if cap is None else cap
        if self.whole_pairs:
            return CM.long_composed_chunk_rows(self.unit_bytes, self.units, cap)
        return LE.cap_units(self.unit_bytes, self.units, cap)

    def chunks(self, cap=None):
        """[units of each chunk] under `cap` bytes"""
        return LE.chunk_sizes(self.units, self.per_chunk(cap))

    def lease(self, cap=None):
        return int(self._lease(DEFAULT_CAP if cap is None else cap))

    def switches(self, cap=None):
        """The environment of a run: the op's route switches and, for a capped run, the cap"""
        out = dict(self.op.switches)
        if cap is not None:
            out[ENV] = int(cap)
        return out

    def need(self, lib, cap=None):
        """The lease the entry point's own query announces under `cap`"""
        with CM.env({ENV: "" if cap is None else int(cap)}):
            return self.op.need(lib)

    def host_caps(self):
        """The caps of the host test: one unit, 2.5 units, exactly three units, one byte (still one unit), above the whole problem (its
        whole lease: a nested chunking is cut by the same cap)"""
        u = self.unit_bytes
        return {"one-unit": u, "2.5-units": 5 * u // 2, "3-units": 3 * u, "one-byte": 1, "whole": self.lease() + 1}


def _cs(prec):
    return CM.ESIZE[prec]


# ---- the short convolutions and cross-spectra: rows, or overlap-save items -----------------------------------------------------------------
def _route(M, switch):
    """half 36 has no tuned plan (the composed route by itself, the two-launch real rows); half 32 is tuned and is switched off"""
    return {} if M == 36 else {switch: 0}


def rconv_seams(prec):
    n, channels, batch = SHAPE
    for M in (36, 32):
        rb = (M + 1) * _cs(prec) + 2 * M * _cs(prec) // 2
        for kind in ("real", "complex"):
            op = CM.rconv1d(f"seam-rconv-{M}-{kind}", M, n, channels, kind, prec, CM.LEASES, _route(M, "DFFT_RCONV_FUSED"), batch=batch)
            for inplace in (False, True):
                s = Seam("rconv1d", op, "row", rb, batch * channels, None, {"4-rows": 4, "1-row": 1}, inplace=inplace)
                s._lease = lambda cap, s=s: s.per_chunk(cap) * s.unit_bytes
                yield s


def rxspec_seams(prec):
    n = SHAPE[0]
    for M in (36, 32):
        rb = 2 * (M + 1) * _cs(prec) + 2 * M * _cs(prec) // 2
        for channels, batch in ((3, 7), (1, 21), (21, 1)):
            for autos in (False, True):
                op = CM.rxspec1d(f"seam-rxspec-{M}-{'auto' if autos else 'cross'}-{channels}x{batch}", M, n, channels, batch, autos, prec,
                                 CM.LEASES, _route(M, "DFFT_RXSPEC_FUSED"))
                s = Seam("rxspec1d", op, "row", rb, batch * channels, None, {"4-rows": 4, "1-row": 1})
                s._lease = lambda cap, s=s: s.per_chunk(cap) * s.unit_bytes
                yield s


def osconv_seams(prec):
    channels, batch = OS_SHAPE
    # (M, discard, n_out, n): four blocks per row, the last ragged; n = n_out - discard (the least the call accepts) and a longer row
    for M, d, n_out, n in ((36, 22, 3 * 50 + 17, 145), (36, 22, 3 * 50 + 17, 160), (32, 22, 3 * 42 + 17, 121)):
        ib = (M + 1) * _cs(prec) + 2 * M * _cs(prec) // 2
        nb = -(-n_out // (2 * M - d))
        assert nb == 4 and n >= n_out - d
        for kind in ("real", "complex"):
            op = CM.rconv1d_os(f"seam-osconv-{M}-{n}-{kind}", M, d, n, n_out, kind, prec, CM.LEASES, _route(M, "DFFT_RCONV_FUSED"),
                               channels=channels, batch=batch)
            s = Seam("rconv1d_os", op, "item", ib, batch * channels * nb, None, {"5-items": 5, "1-item": 1})
            s._lease = lambda cap, s=s: s.per_chunk(cap) * s.unit_bytes
            yield s


# ---- the long convolution and cross-spectrum ------------------------------------------------------------------------------------------------
def long_composed_lease(m, rows, prec, fields, cap):
    """dfft_batch.cpp, the composed long routes: the bins of `fields` fields and the padded rows of a chunk, rounded up to 256 bytes, plus
    the scratch of the paired real rows of length m on that chunk -- cut by the same cap"""
    rb = CM.long_row_bytes(m, prec, fields)
    nr = CM.long_composed_chunk_rows(rb, rows, cap)
    return (nr * rb + 255) // 256 * 256 + LE.real_pair_scratch(m, nr, prec, 0, False, cap)


def lconv_seams(prec):
    m = LONG_M
    batch, channels = LONG_ROWS
    rows = batch * channels
    for n, kind in ((7, "complex"), (m, "real")):
        for fused in (False, True):
            tag = "fused" if fused else "composed"
            op = CM.rconv1d_long(f"seam-lconv-{tag}-n{n}", m, n, kind, prec, {} if fused else {"DFFT_RCONV_LONG_FUSED": 0}, rows=LONG_ROWS)
            for inplace in (False, True):
                if fused:   # pass-A rows: m/2 complex each; odd chunks end on a half-empty pair of scratch rows
                    s = Seam("rconv1d_long", op, "row", (m // 2) * _cs(prec), rows, None, {"3-rows": 3, "1-row": 1, "4-rows": 4}, inplace=inplace)
                    s._lease = lambda cap, s=s: s.per_chunk(cap) * s.unit_bytes
                else:
                    s = Seam("rconv1d_long", op, "row", CM.long_row_bytes(m, prec, 1), rows, None, {"2-rows": 2, "1-row": 1}, inplace=inplace,
                             query=False, whole_pairs=True)
                    s._lease = lambda cap: long_composed_lease(m, rows, prec, 1, cap)
                yield s


def lxspec_seams(prec):
    m = LONG_M
    batch, channels = LONG_ROWS
    rows = batch * channels
    for n, autos, order in ((7, False, 0), (7, True, 1), (m, False, 1), (m, True, 0)):
        for fused in (False, True):
            tag = f"{'fused' if fused else 'composed'}-{'auto' if autos else 'cross'}-n{n}-order{order}"
            op = CM.rxspec1d_long(f"seam-lxspec-{tag}", m, n, channels, batch, autos, order, prec, {} if fused else {"DFFT_RXSPEC_LONG_FUSED": 0})
            if fused:
                s = Seam("rxspec1d_long", op, "row", 2 * (m // 2) * _cs(prec), rows, None, {"3-rows": 3, "1-row": 1, "4-rows": 4}, exact=False,
                         sums=(m, n, channels, batch, order, autos))
                s._lease = lambda cap: XL.scratch_bytes(m, channels, batch, prec, cap)
            else:
                s = Seam("rxspec1d_long", op, "row", CM.long_row_bytes(m, prec, 2), rows, None, {"2-rows": 2, "1-row": 1}, query=False, whole_pairs=True)
                s._lease = lambda cap: long_composed_lease(m, rows, prec, 2, cap)
            yield s


# ---- real rows in pairs, strided real columns, r2r, Bluestein -------------------------------------------------------------------------------
def real_pair_seams(prec):
    batch = 7                       # three whole pairs and a half-empty one
    for n, switches in ((375, {}), (1009, {}), (1009, {"DFFT_BLUESTEIN_FUSED": 0})):
        family = "real-bluestein" if n == 1009 else "real"
        for direction in (CM.FWD, CM.BWD):
            tag = f"seam-{'rfft' if direction > 0 else 'irfft'}-{n}" + ("-multi-pass" if switches else "")
            op = CM.real_1d(tag, family, n, 1, prec, direction, CM.LEASES, False, batch=batch, switches=switches)
            s = Seam("real-rows", op, "pair", n * _cs(prec), (batch + 1) // 2, None, {"2-pairs": 2, "1-pair": 1})
            s._lease = lambda cap, n=n, sw=switches: LE.real_pair_scratch(n, batch, prec, bluestein_M(n), bluestein_fused(n, 1, sw), cap)
            yield s


def real_cols_seams(prec):
    n, batch = 375, 5
    for s_ in (3, 4):
        sp = (s_ + 1) // 2
        for direction in (CM.FWD, CM.BWD):
            op = CM.real_1d(f"seam-{'rfft' if direction > 0 else 'irfft'}-cols-{n}x{s_}", "real", n, s_, prec, direction, CM.LEASES, True, batch=batch)
            s = Seam("real-cols", op, "item", n * sp * _cs(prec), batch, None, {"2-items": 2, "1-item": 1})
            s._lease = lambda cap, s_=s_: LE.composed_scratch(n, s_, batch, prec, 0, False, rows_pair=False, cap=cap)
            yield s


def r2r_seams(prec):
    shapes = [(375, 1, 7, kind, {}) for kind in A.R2R_KINDS] + [(375, 3, 5, kind, {}) for kind in A.R2R_KINDS]
    shapes += [(1009, 1, 7, kind, {"DFFT_BLUESTEIN_FUSED": 0}) for kind in ("dct2", "dst3")]   # Bluestein chunks inside an r2r chunk
    for n, s_, batch, kind, switches in shapes:
        units, sp = LE.pair_units(s_, batch)
        family = "r2r-bluestein" if n == 1009 else "r2r"
        op = CM.r2r_1d(f"seam-{kind}-{n}x{s_}", family, n, s_, kind, prec, CM.LEASES, switches, batch=batch)
        for inplace in (False, True):
            s = Seam("r2r", op, "unit", n * sp * _cs(prec), units, None, {"2-units": 2, "1-unit": 1}, inplace=inplace)
            s._lease = lambda cap, n=n, s_=s_, batch=batch, sw=switches, sp=sp: LE.composed_scratch(
                n, s_, batch, prec, bluestein_M(n), bluestein_fused(n, sp, sw), cap=cap)
            yield s


def bluestein_seams(prec):
    batch = 5
    for n, s_, switches in ((4099, 1, {}), (4099, 5, {}), (1009, 3, {"DFFT_BLUESTEIN_FUSED": 0})):
        for direction in (CM.FWD, CM.BWD):
            shape = (batch, n, s_)
            op = CM.complex_1d(f"seam-any-{n}x{s_}-{'fwd' if direction > 0 else 'bwd'}", "dfft_fft1d_any", "bluestein", n, shape, prec,
                               direction=direction, switches=switches)
            for inplace in (False, True):
                s = Seam("bluestein", op, "transform", lambda n=n, s_=s_: LE.bluestein_per_transform_bytes(bluestein_M(n), s_, prec), batch, None,
                         {"2-transforms": 2, "1-transform": 1}, inplace=inplace)
                s._lease = lambda cap, n=n, s_=s_: LE.bluestein_scratch(bluestein_M(n), s_, batch, prec, False, cap)
                yield s


BUILDERS = (rconv_seams, rxspec_seams, osconv_seams, lconv_seams, lxspec_seams, real_pair_seams, real_cols_seams, r2r_seams, bluestein_seams)
FAMILIES = ("rconv1d", "rxspec1d", "rconv1d_os", "rconv1d_long", "rxspec1d_long", "real-rows", "real-cols", "r2r", "bluestein")


def seams_of(prec):
    return [s for build in BUILDERS for s in build(prec)]


SEAMS = seams_of("f64") + seams_of("f32")
BY_NAME = {s.name: s for s in SEAMS}
assert len(BY_NAME) == len(SEAMS), "seam names repeat"
assert {s.family for s in SEAMS} == set(FAMILIES)
