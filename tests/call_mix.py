"""The registry behind tests/test_call_mix_host.py and tests/test_gpu_call_mix.py: one small case (an *op*) of every plan-less entry point
and of every configuration of it that lays the shared per-(device, stream) scratch buffer out differently.  No GPU is needed to import it.

An op carries its inputs (numpy, already in the working precision), the raw ctypes call with a stream argument, the lease the call takes
(through the entry point's own dfft_*_scratch_bytes query), its longdouble reference, the measure and bound of its family (the existing
ones: accuracy_ref.BOUND[...] or the constant of the family's GPU module -- nothing here sets a tolerance), a same-precision CPU model of
the reference, the environment switches of its route, and whether it `leases` scratch or takes `no_lease`.

Cases, references and bounds are those of the families' own builders: accuracy_ref, rconv1d_cases, rconv1d_os_cases, rconv1d_long_cases,
rxspec1d_cases, rxspec1d_long_cases, stft_cases, rcsd1d_cases.  Sizes are the smallest that still take the route.

rconv1d, rconv1d_os and rxspec1d composed run in SEVERAL chunks too: their rule cuts at 256 MiB of scratch, beyond the 64 MiB this module
allows itself, so the ops carry the general chunk cap DFFT_SCRATCH_CHUNK_BYTES in their environment, as the stft1d, istft1d and rcsd1d
ops carry DFFT_STFT_CHUNK_BYTES / DFFT_RCSD_CHUNK_BYTES.  (Every other composed route's seams: tests/chunk_seams.py.)

Left out, on purpose:
  * a dfft_rconv1d_long length whose fused kernels spill: there is none (dfft_lconv.hip, lconv_fused_ok is true for every factor), so the
    composed route is reached through DFFT_RCONV_LONG_FUSED=0 only.  dfft_rxspec1d_long does have such lengths (N2 = 384, fp64)."""
import contextlib
import importlib
import os
import re

import numpy as np

import accuracy_ref as A
import rconv1d_cases as RC
import rconv1d_long_cases as LC
import rconv1d_os_cases as OC
import rcsd1d_cases as WC
import rxspec1d_cases as XC
import rxspec1d_long_cases as XL
import stft_cases as SC

try:
    import scipy.fft as sf
except ImportError:  # the same-precision CPU models then run on torch's CPU FFT
    sf = None

CODE = {"f64": 0, "f32": 1}
ESIZE = {"f64": 16, "f32": 8}
FWD, BWD = +1, -1
MEMORY_CAP = 64 << 20          # no op leases or writes more
LEASES, NO_LEASE = "leases", "no_lease"

# The plan-less entry points (include/dfft.h) that can take scratch from the shared buffer: each needs at least one leasing op.
ENTRY_POINTS = ("dfft_fft1d_rows", "dfft_fft1d_cols", "dfft_fft1d_any", "dfft_rfft1d", "dfft_rfft1d_strided", "dfft_rfft2d_batch",
                "dfft_fft2d_batch", "dfft_r2r1d_strided", "dfft_rconv1d", "dfft_rconv1d_os", "dfft_rconv1d_long", "dfft_rxspec1d",
                "dfft_rxspec1d_long", "dfft_stft1d", "dfft_istft1d", "dfft_rcsd1d")

# Every other symbol of _lib.SIGNATURES, by pattern, with the reason it is not an op.  A new symbol that matches nothing fails
# test_call_mix_host.py::test_the_registry_is_complete until it is registered or excluded here.
EXCLUDED = (
    (r"dfft_plan_\w+|dfft_execute|dfft_stage_times|dfft_kernel_times|dfft_conv_set_\w+", "plans own their buffers and streams: out of scope"),
    (r"dfft_scale", "one elementwise launch: takes no lease, reads no table, keeps no state"),
    (r"dfft_rconv1d_long_filter", "a pure permutation of the filter: takes no lease, reads no table, keeps no state"),
    (r"dfft_fft2d_batch_status", "reads the pinned error words of dfft_fft2d_batch; the GPU tests call it after every tour"),
    (r"dfft_trim|dfft_debug_scratch_\w+", "the state management and test hooks the GPU tests drive themselves"),
    (r"dfft_\w+_(scratch_bytes|fused_applies|slices|length|split|block|frames|supported|kind|form)|dfft_length_\w+|dfft_bluestein_length|dfft_real_form",
     "host arithmetic: no device, no stream"),
    (r"dfft_version|dfft_last_error|dfft_device_\w+|dfft_proper_device_count|dfft_local_\w+|dfft_max_count|dfft_exchange_\w+|dfft_r2c_counts|"
     r"dfft_conv_\w+|dfft_trace_dump", "queries and layout arithmetic: enqueue nothing"),
    (r"dfft_comm_\w+|dfft_rccl_unique_id|dfft_boot_\w+", "communicators and the rendezvous: several devices are out of scope"),
    (r"dfft_alloc|dfft_free", "allocation: enqueues nothing on a caller's stream"),
)


def exclusion(name):
    """The reason `name` is not an op, or None"""
    for pattern, reason in EXCLUDED:
        if re.fullmatch(pattern, name):
            return reason
    return None


@contextlib.contextmanager
def env(switches):
    """Environment switches the library reads per call, set around the calls inside (as tests/test_gpu_rcsd1d.py does)"""
    old = {k: os.environ.get(k) for k in switches}
    os.environ.update({k: str(v) for k, v in switches.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def family_bound(module, name="BOUND"):
    """A constant of a family's GPU test module (imported late: those modules are test modules)"""
    return getattr(importlib.import_module(module), name)


# ---- same-precision CPU transforms (scipy.fft; torch's CPU FFT where scipy is missing -- numpy computes float32 transforms in double) ----
def _torch_fft(fn, x, **kw):
    import torch
    return getattr(torch.fft, fn)(torch.from_numpy(np.ascontiguousarray(x)), **kw).numpy()


def c_fft(x, axis, sign, prec):
    x = np.asarray(x).astype(A.CDT[prec])
    if sf is not None:
        return sf.fft(x, axis=axis) if sign > 0 else sf.ifft(x, axis=axis, norm="forward")
    return _torch_fft("fft", x, dim=axis) if sign > 0 else _torch_fft("ifft", x, dim=axis, norm="forward")


def c_rfft(x, axis, prec):
    x = np.asarray(x).astype(A.RDT[prec])
    out = sf.rfft(x, axis=axis) if sf is not None else _torch_fft("rfft", x, dim=axis)
    assert out.dtype == A.CDT[prec]
    return out


def c_irfft(X, n, axis, prec):
    """n * irfft(X, n) in the working precision"""
    X = np.asarray(X).astype(A.CDT[prec])
    out = sf.irfft(X, n, axis=axis, norm="forward") if sf is not None else _torch_fft("irfft", X, n=n, dim=axis, norm="forward")
    assert out.dtype == A.RDT[prec]
    return out


def c_r2r(x, kind, prec):
    """accuracy_ref.ld_r2r's mirror construction on the working-precision FFT: [b][n][s] along axis 1"""
    x = np.asarray(x).astype(A.RDT[prec])
    b, n, s = x.shape
    alt = ((-1.0) ** np.arange(n)).astype(A.RDT[prec])[None, :, None]
    if kind == "dct2":
        u = np.zeros((b, 4 * n, s), dtype=A.RDT[prec])
        u[:, 1:2 * n:2, :] = x
        u[:, 4 * n - 1:2 * n:-2, :] = x
        return c_fft(u, 1, +1, prec)[:, :n, :].real
    if kind == "dct3":
        v = np.zeros((b, 4 * n, s), dtype=A.RDT[prec])
        v[:, :n, :] = 2 * x
        v[:, 0, :] = x[:, 0, :]
        return c_fft(v, 1, +1, prec)[:, 1:2 * n:2, :].real
    if kind == "dst2":
        return c_r2r(x * alt, "dct2", prec)[:, ::-1, :]
    return alt * c_r2r(x[:, ::-1, :], "dct3", prec)


# ---- the op ------------------------------------------------------------------------------------------------------------------------------
class Op:
    """One small case of one entry point.  `build()` -> (inputs {name: numpy array in the working precision}, out shape, out numpy dtype,
    longdouble reference); `call(lib, p, out, stream)` with p = {name: device pointer} -> the entry point's return code;
    `need(lib)` -> the bytes the call leases, by the entry point's own query (evaluate it under `switches`); `measure(got, ref)` -> the
    family's error figure, held against `bound` (whose origin `bound_name` spells out); `model(inputs)` -> the same-precision CPU result."""

    def __init__(self, name, entry, prec, flag, build, call, need, measure, bound, bound_name, model, switches=None, tables=False):
        self.name, self.entry, self.prec, self.flag = f"{name}-{prec}", entry, prec, flag
        self._build, self._call, self._need, self._measure, self._model = build, call, need, measure, model
        self._bound, self.bound_name = bound, bound_name
        self.switches = dict(switches or {})
        self.tables = tables    # reads tables that dfft_trim drops (Bluestein chirps, r2r quarter waves) or that are built on first use
        self._case = None

    def __repr__(self):
        return self.name

    @property
    def case(self):
        if self._case is None:
            inputs, shape, dtype, ref = self._build()
            for a in inputs.values():
                a.setflags(write=False)
            self._case = (inputs, tuple(shape), np.dtype(dtype), ref)
        return self._case

    @property
    def bound(self):
        return self._bound() if callable(self._bound) else self._bound

    def need(self, lib):
        with env(self.switches):
            return int(self._need(lib))

    def call(self, lib, pointers, out, stream):
        """Enqueue on `stream` (an integer handle, 0 / None: the NULL stream) under the op's switches"""
        with env(self.switches):
            return self._call(lib, pointers, out, stream or None)

    def call_as_is(self, lib, pointers, out, stream):
        """The same call with the environment left alone: for host threads, which must not change it under each other (the caller
        sets `switches` around the whole threaded section)"""
        return self._call(lib, pointers, out, stream or None)

    def measure(self, got):
        return self._measure(np.asarray(got), self.case[3])

    def model(self):
        with env(self.switches):
            return self._model(self.case[0])

    def out_bytes(self):
        _, shape, dtype, _ = self.case
        return int(np.prod(shape)) * dtype.itemsize


def _cplx(a, prec):
    return np.ascontiguousarray(np.asarray(a).astype(A.CDT[prec]))


def _real(a, prec):
    return np.ascontiguousarray(np.asarray(a).astype(A.RDT[prec]))


def _acc(family, prec):
    return A.BOUND[family][prec], f"accuracy_ref.BOUND[{family!r}][{prec!r}]"


# ---- complex 1-D: four-step rows / columns, Bluestein -------------------------------------------------------------------------------------
def complex_1d(name, entry, family, n, shape, prec, direction=FWD, flag=LEASES, switches=None, base=0):
    """`shape` = (batch, n) for rows, (batch, n, s) for columns / dfft_fft1d_any; the transform runs along axis 1"""
    batch, s = shape[0], (shape[2] if len(shape) == 3 else 1)
    code = CODE[prec]

    def build():
        x, F = A.complex_lines(n, shape, 1, 1000 + n, base)
        return {"x": _cplx(x, prec)}, shape, A.CDT[prec], (F if direction > 0 else A.reverse_bins(F, [1]))

    def call(lib, p, out, stream):
        if entry == "dfft_fft1d_rows":
            return lib.dfft_fft1d_rows(p["x"], out, n, batch, code, direction, stream)
        return getattr(lib, entry)(p["x"], out, n, s, batch, code, direction, stream)

    bound, bname = _acc(family, prec)
    return Op(name, entry, prec, flag, build, call, lambda lib: lib.dfft_fft1d_any_scratch_bytes(n, s, batch, code),
              lambda got, ref: A.nu(got, ref, n, prec, (1,)), bound, bname, lambda inp: c_fft(inp["x"], 1, direction, prec), switches,
              tables=True)


# ---- real 1-D rows and strided columns ----------------------------------------------------------------------------------------------------
def real_1d(name, family, n, s, prec, direction, flag, strided, batch=None, switches=None):
    """dfft_rfft1d on [3][n] (strided=False) or dfft_rfft1d_strided on [2][n][s] (or on `batch` rows / items)"""
    batch, code, nh = batch or (2 if strided else 3), CODE[prec], n // 2 + 1

    def build():
        if direction > 0:
            x, ref = A.real_lines(n, batch, s, 2000 + n)
            src, shape, dtype = _real(x, prec), (batch, nh, s), A.CDT[prec]
        else:
            X, ref = A.half_spectra(n, batch, s, 3000 + n)
            src, shape, dtype = _cplx(X, prec), (batch, n, s), A.RDT[prec]
        if not strided:
            src, shape, ref = np.ascontiguousarray(src[:, :, 0]), shape[:2], ref[:, :, 0]
        return {"x": src}, shape, dtype, ref

    def call(lib, p, out, stream):
        if strided:
            return lib.dfft_rfft1d_strided(p["x"], out, n, s, batch, code, direction, stream)
        return lib.dfft_rfft1d(p["x"], out, n, batch, code, direction, stream)

    def need(lib):
        return lib.dfft_rfft1d_strided_scratch_bytes(n, s, batch, code) if strided else lib.dfft_rfft1d_scratch_bytes(n, batch, code, direction)

    def model(inp):
        return c_rfft(inp["x"], 1, prec) if direction > 0 else c_irfft(inp["x"], n, 1, prec)

    bound, bname = _acc(family, prec)
    return Op(name, "dfft_rfft1d_strided" if strided else "dfft_rfft1d", prec, flag, build, call, need,
              lambda got, ref: A.nu(got, ref, n, prec, (1,)), bound, bname, model, switches, tables=True)


def r2r_1d(name, family, n, s, kind, prec, flag, switches=None, batch=2):
    code, k = CODE[prec], A.R2R_KINDS.index(kind)

    def build():
        case = A.r2r_lines(n, batch, s, 6000 + n)
        return {"x": _real(case[0], prec)}, (batch, n, s), A.RDT[prec], case[1 + k]

    bound, bname = _acc(family, prec)
    return Op(name, "dfft_r2r1d_strided", prec, flag, build,
              lambda lib, p, out, stream: lib.dfft_r2r1d_strided(p["x"], out, n, s, batch, code, k, stream),
              lambda lib: lib.dfft_r2r1d_strided_scratch_bytes(n, s, batch, code, k, int(s % 2 == 0)),
              lambda got, ref: A.nu(got, ref, n, prec, (1,)), bound, bname, lambda inp: c_r2r(inp["x"], kind, prec), switches, tables=True)


# ---- 2-D ----------------------------------------------------------------------------------------------------------------------------------
def real_2d(name, n1, n2, batch, prec, direction, flag):
    code, nh = CODE[prec], n2 // 2 + 1

    def build():
        if direction > 0:
            x, ref = A.real_planes(n1, n2, batch, 4000 + n1)
            return {"x": _real(x, prec)}, (batch, n1, nh), A.CDT[prec], ref
        X, ref = A.half_planes(n1, n2, batch, 5000 + n1)
        return {"x": _cplx(X, prec)}, (batch, n1, n2), A.RDT[prec], ref

    def model(inp):
        if direction > 0:
            return c_fft(c_rfft(inp["x"], 2, prec), 1, +1, prec)
        return c_irfft(c_fft(inp["x"], 1, -1, prec), n2, 2, prec)

    bound, bname = _acc("real", prec)
    return Op(name, "dfft_rfft2d_batch", prec, flag, build,
              lambda lib, p, out, stream: lib.dfft_rfft2d_batch(p["x"], out, n1, n2, batch, code, direction, stream),
              lambda lib: lib.dfft_rfft2d_batch_scratch_bytes(n1, n2, batch, code, direction),
              lambda got, ref: A.nu(got, ref, n1 * n2, prec, (1, 2)), bound, bname, model)


def complex_2d(name, family, n1, n2, batch, prec, direction, flag):
    code = CODE[prec]

    def build():
        x, F = A.complex_planes(n1, n2, batch, 7000 + n1)
        return {"x": _cplx(x, prec)}, (batch, n1, n2), A.CDT[prec], (F if direction > 0 else A.reverse_bins(F, (1, 2)))

    bound, bname = _acc(family, prec)
    return Op(name, "dfft_fft2d_batch", prec, flag, build,
              lambda lib, p, out, stream: lib.dfft_fft2d_batch(p["x"], out, n1, n2, batch, code, direction, stream),
              lambda lib: lib.dfft_fft2d_batch_scratch_bytes(n1, n2, batch, code),
              lambda got, ref: A.nu(got, ref, n1 * n2, prec, (1, 2)), bound, bname,
              lambda inp: c_fft(c_fft(inp["x"], 2, direction, prec), 1, direction, prec))


# ---- 1-D real convolutions ----------------------------------------------------------------------------------------------------------------
def _filter(H, kind, prec):
    return _real(H, prec) if kind == "real" else _cplx(H, prec)


def _conv_model(xp, H, m, n, prec):
    """irfft(rfft(xp) * H) / m of padded rows (or blocks) xp [...][m], filter rows H broadcast against them, first n samples"""
    Y = c_rfft(xp, -1, prec) * H.astype(A.CDT[prec])
    return (c_irfft(Y, m, -1, prec) / A.RDT[prec](m))[..., :n]


def _pad(x, m, prec):
    xp = np.zeros(x.shape[:-1] + (m,), dtype=A.RDT[prec])
    xp[..., :x.shape[-1]] = x
    return xp


def rconv1d(name, M, n, channels, kind, prec, flag, switches=None, batch=None):
    m, code, batch = 2 * M, CODE[prec], batch or RC.batch_for(M, channels)

    def build():
        x, H, ref = RC.case(M, n, channels, batch, kind)
        return {"x": _real(x, prec), "h": _filter(H, kind, prec)}, x.shape, A.RDT[prec], ref

    def model(inp):
        rows = inp["x"].shape[0]
        return _conv_model(_pad(inp["x"], m, prec), inp["h"][np.arange(rows) % channels], m, n, prec)

    return Op(name, "dfft_rconv1d", prec, flag, build,
              lambda lib, p, out, stream: lib.dfft_rconv1d(p["x"], out, p["h"], n, m, channels, batch, code, int(kind == "real"), stream),
              lambda lib: lib.dfft_rconv1d_scratch_bytes(n, m, channels, batch, code),
              lambda got, ref: RC.nu_rows(got, ref, m, prec), lambda: family_bound("test_gpu_rconv1d")[prec], "test_gpu_rconv1d.BOUND", model,
              switches)


def rconv1d_os(name, M, d, n, n_out, kind, prec, flag, switches=None, channels=3, batch=2):
    m, code = 2 * M, CODE[prec]

    def build():
        x, H, ref = OC.case(M, d, n, n_out, channels, batch, kind)
        return {"x": _real(x, prec), "h": _filter(H, kind, prec)}, (x.shape[0], n_out), A.RDT[prec], ref

    def model(inp):
        rows = inp["x"].shape[0]
        xb = OC.gather(inp["x"], m, d, n_out).astype(A.RDT[prec])
        cb = _conv_model(xb, inp["h"][np.arange(rows) % channels][:, None, :], m, m, prec)
        return cb[:, :, d:].reshape(rows, -1)[:, :n_out]

    return Op(name, "dfft_rconv1d_os", prec, flag, build,
              lambda lib, p, out, stream: lib.dfft_rconv1d_os(p["x"], out, p["h"], n, n_out, m, d, channels, batch, code, int(kind == "real"),
                                                              stream),
              lambda lib: lib.dfft_rconv1d_os_scratch_bytes(n_out, m, d, channels, batch, code),
              lambda got, ref: OC.nu_rows(got, ref, m, prec), lambda: family_bound("test_gpu_rconv1d_os")[prec], "test_gpu_rconv1d_os.BOUND",
              model, switches)


def long_row_bytes(m, prec, fields):
    """One row of the composed long routes: its bins of `fields` fields and its m padded reals"""
    return fields * (m // 2 + 1) * ESIZE[prec] + m * (ESIZE[prec] // 2)


def long_composed_chunk_rows(rb, rows, cap):
    """dfft_batch.cpp long_composed_chunk_rows: rows of rb bytes within max(cap, one row's), never fewer than two, and whole pairs (an
    even count) unless the chunk is the whole call -- rows 2p and 2p + 1 share their transforms"""
    nr = max(1, min(rows, max(max(cap, rb) // rb, 2)))
    return nr - (nr & 1) if nr < rows else nr


def chunk_cap():
    """The cap of the chunk rule as the library reads it per call: a positive DFFT_SCRATCH_CHUNK_BYTES, else 256 MiB"""
    text = os.environ.get("DFFT_SCRATCH_CHUNK_BYTES", "")
    try:
        value = int(text)
    except ValueError:
        value = 0
    return value if value > 0 else 256 << 20


def _long_composed_need(lib, m, rows, prec, fields):
    """The lease of the composed routes of dfft_rconv1d_long (fields = 1) / dfft_rxspec1d_long (fields = 2) by the rule in
    dfft_batch.cpp: the bins of `fields` fields and the padded rows of a chunk, rounded up to 256 bytes, plus the real rows' own scratch
    (the entry points have no query of their own for this route; the real rows' query reads the same cap)"""
    nr = long_composed_chunk_rows(long_row_bytes(m, prec, fields), rows, chunk_cap())
    rb = long_row_bytes(m, prec, fields)
    inner = max(lib.dfft_rfft1d_scratch_bytes(m, nr, CODE[prec], d) for d in ((FWD, BWD) if fields == 1 else (FWD,)))
    return (nr * rb + 255) // 256 * 256 + inner


def rconv1d_long(name, m, n, kind, prec, switches=None, rows=None):
    """`rows` = (batch, channels): another row count than the accuracy sweep's, with rconv1d_cases' longdouble reference at length m"""
    code = CODE[prec]
    batch, channels = rows or LC.ACC_ROWS
    n1, n2 = LC.SPLITS.get(m) or LC.split(m)

    def build():
        if rows:
            x, H, _ = LC.case(m, n, channels, batch, kind)
            ref = RC.reference(x, H, m)
        else:
            x, H, ref = LC.acc_case(m, n, kind)
        return {"x": _real(x, prec), "hp": _filter(LC.permute_filter(H, n1, n2), kind, prec), "h": _filter(H, kind, prec)}, x.shape, A.RDT[prec], ref

    def need(lib):
        if lib.dfft_rconv1d_long_fused_applies(m, code):
            return lib.dfft_rconv1d_long_scratch_bytes(n, m, channels, batch, code)
        return _long_composed_need(lib, m, batch * channels, prec, 1)

    def model(inp):
        rows = inp["x"].shape[0]
        return _conv_model(_pad(inp["x"], m, prec), inp["h"][np.arange(rows) % channels], m, n, prec)

    return Op(name, "dfft_rconv1d_long", prec, LEASES, build,
              lambda lib, p, out, stream: lib.dfft_rconv1d_long(p["x"], out, p["hp"], n, m, channels, batch, code, int(kind == "real"), stream),
              need, lambda got, ref: LC.nu_rows(got, ref, m, prec), LC.BOUND[prec], "rconv1d_long_cases.BOUND", model, switches, tables=True)


# ---- cross-spectra ------------------------------------------------------------------------------------------------------------------------
def _xspec_model(x, g, m, channels, prec):
    X = c_rfft(_pad(x, m, prec), 1, prec)
    G = X if g is x else c_rfft(_pad(g, m, prec), 1, prec)
    return (np.conj(X) * G).reshape(x.shape[0] // channels, channels, m // 2 + 1).sum(axis=0, dtype=A.CDT[prec])


def rxspec1d(name, M, n, channels, batch, autos, prec, flag, switches=None):
    m, code = 2 * M, CODE[prec]

    def build():
        x, g, ref, auto = XC.case(M, n, channels, batch)
        inputs = {"x": _real(x, prec)} if autos else {"x": _real(x, prec), "g": _real(g, prec)}
        return inputs, (channels, M + 1), A.CDT[prec], (auto if autos else ref)

    return Op(name, "dfft_rxspec1d", prec, flag, build,
              lambda lib, p, out, stream: lib.dfft_rxspec1d(p["x"], p["x" if autos else "g"], out, n, m, channels, batch, code, stream),
              lambda lib: lib.dfft_rxspec1d_scratch_bytes(n, m, channels, batch, code),
              lambda got, ref: XC.nu_lines(got, ref, m, prec), lambda: family_bound("test_gpu_rxspec1d")[prec], "test_gpu_rxspec1d.BOUND",
              lambda inp: _xspec_model(inp["x"], inp["x"] if autos else inp["g"], m, channels, prec), switches)


def rxspec1d_long(name, m, n, channels, batch, autos, order, prec, switches=None):
    code = CODE[prec]
    n1, n2 = XL.SPLITS.get(m) or LC.split(m)

    def build():
        x, g, ref, auto = XL.case(m, n, channels, batch)
        ref = auto if autos else ref
        inputs = {"x": _real(x, prec)} if autos else {"x": _real(x, prec), "g": _real(g, prec)}
        return inputs, (channels, m // 2 + 1), A.CDT[prec], (LC.permute_filter(ref, n1, n2) if order else ref)

    def need(lib):
        if lib.dfft_rxspec1d_long_fused_applies(m, code):
            return lib.dfft_rxspec1d_long_scratch_bytes(n, m, channels, batch, code)
        return _long_composed_need(lib, m, batch * channels, prec, 2)

    def model(inp):
        S = _xspec_model(inp["x"], inp["x"] if autos else inp["g"], m, channels, prec)
        return LC.permute_filter(S, n1, n2) if order else S

    assert XL.klass(n, batch) == "sweep"
    return Op(name, "dfft_rxspec1d_long", prec, LEASES, build,
              lambda lib, p, out, stream: lib.dfft_rxspec1d_long(p["x"], p["x" if autos else "g"], out, n, m, channels, batch, code, order, stream),
              need, lambda got, ref: XL.nu_lines(got, ref, m, prec), XL.BOUND[prec]["sweep"], "rxspec1d_long_cases.BOUND[prec]['sweep']", model,
              switches, tables=True)


# ---- framed transforms --------------------------------------------------------------------------------------------------------------------
def stft_item_bytes(m, prec, kind):
    """dfft_stft.hip, fwd_item_bytes: the m windowed reals of an item and, for the power form, its m/2 + 1 bins"""
    return m * ESIZE[prec] // 2 + ((m // 2 + 1) * ESIZE[prec] if kind == "power" else 0)


def stft1d(name, case, mode, kind, prec, flag, switches=None):
    M, hop, pad, n, wkind = case
    m, code = 2 * M, CODE[prec]
    frames, rows = SC.frames_of(n, m, hop, pad), SC.ROWS

    def build():
        x, win, nf, ref = SC.forward_case(M, hop, pad, n, wkind, mode)
        assert nf == frames
        power = kind == "power"
        return ({"x": _real(x, prec), "win": _real(win, prec)}, ref.shape, A.RDT[prec] if power else A.CDT[prec], SC.power(ref) if power else ref)

    def model(inp):
        X = c_rfft(SC.gather(inp["x"], m, hop, pad, frames, mode).astype(A.RDT[prec]) * inp["win"], 2, prec)
        return SC.power(X) if kind == "power" else X

    factor = 2.0 if kind == "power" else 1.0      # tests/test_gpu_stft.py holds the squared moduli to twice the cap
    return Op(name, "dfft_stft1d", prec, flag, build,
              lambda lib, p, out, stream: lib.dfft_stft1d(p["x"], out, p["win"], n, m, hop, pad, frames, rows, code, SC.MODE_CODE[mode],
                                                          SC.KIND_CODE[kind], 1.0, stream),
              lambda lib: lib.dfft_stft1d_scratch_bytes(m, frames, rows, code, SC.KIND_CODE[kind]),
              lambda got, ref: SC.nu_frames(got, ref, m, prec), lambda: factor * family_bound("test_gpu_stft", "CAP")[prec],
              "test_gpu_stft.CAP" + (" x 2 (power)" if kind == "power" else ""), model, switches)


def istft_item_bytes(m, prec, tuned):
    """dfft_stft.hip, inv_item_bytes: the m reals of an item and, for an untuned m/2, the copy of its m/2 + 1 bins"""
    return m * ESIZE[prec] // 2 + (0 if tuned else (m // 2 + 1) * ESIZE[prec])


def istft1d(name, case, prec, switches=None):
    M, hop, pad, frames, wkind = case
    m, code, rows = 2 * M, CODE[prec], SC.ROWS

    def build():
        X, win, inv_env, n, ref = SC.inverse_case(M, hop, pad, frames, wkind)
        return {"x": _cplx(X, prec), "win": _real(win, prec), "env": _real(inv_env, prec)}, (rows, n), A.RDT[prec], ref

    def n_of():
        return SC.inverse_case(M, hop, pad, frames, wkind)[3]

    def model(inp):
        n = n_of()
        c = c_irfft(inp["x"], m, 2, prec) * inp["win"] / A.RDT[prec](m)
        y = np.zeros((rows, (frames - 1) * hop + m), dtype=A.RDT[prec])
        for f in range(frames):
            y[:, f * hop:f * hop + m] += c[:, f]
        return y[:, pad:pad + n] * inp["env"]

    return Op(name, "dfft_istft1d", prec, LEASES, build,
              lambda lib, p, out, stream: lib.dfft_istft1d(p["x"], out, p["win"], p["env"], n_of(), m, hop, pad, frames, rows, code, stream),
              lambda lib: lib.dfft_istft1d_scratch_bytes(m, frames, rows, code),
              lambda got, ref: SC.nu_rows(got, ref, m, prec), lambda: family_bound("test_gpu_stft", "CAP")[prec], "test_gpu_stft.CAP", model,
              switches)


def rcsd_item_bytes(m, prec):
    """tests/test_gpu_rcsd1d.py, _item_bytes: a frame's windowed reals and its bins of both fields"""
    return m * ESIZE[prec] // 2 + 2 * (m // 2 + 1) * ESIZE[prec]


def rcsd1d(name, M, rows, frames, hop, autos, prec, flag, switches=None):
    m, code = 2 * M, CODE[prec]
    n = (frames - 1) * hop + m

    def build():
        x, g, win, ref, auto = WC.case(M, rows, frames, hop, 0, "hann")
        inputs = {"x": _real(x, prec), "win": _real(win, prec)}
        if not autos:
            inputs["g"] = _real(g, prec)
        return inputs, (rows, M + 1), A.CDT[prec], (auto if autos else ref)

    def model(inp):
        X = c_rfft(WC.frames_of(inp["x"], m, hop) * inp["win"], 2, prec)
        G = X if autos else c_rfft(WC.frames_of(inp["g"], m, hop) * inp["win"], 2, prec)
        return (np.conj(X) * G).sum(axis=1, dtype=A.CDT[prec])

    return Op(name, "dfft_rcsd1d", prec, flag, build,
              lambda lib, p, out, stream: lib.dfft_rcsd1d(p["x"], p["x" if autos else "g"], out, p["win"], n, m, hop, frames, rows, 1.0, code,
                                                          stream),
              lambda lib: lib.dfft_rcsd1d_scratch_bytes(m, frames, rows, code, int(autos)),
              lambda got, ref: WC.nu_lines(got, ref, m, prec), lambda: family_bound("test_gpu_rcsd1d")[prec], "test_gpu_rcsd1d.BOUND", model,
              switches)


# ---- the registry -------------------------------------------------------------------------------------------------------------------------
STFT_BASE = (64, 32, 64, 386, "hann")       # stft_cases' base case: M, hop, pad, n, window
ISTFT_BASE = (64, 32, 64, 9, "hann")        # M, hop, pad, frames, window
RCSD_M, RCSD_ROWS = 64, 3
RXSPEC_M, RXSPEC_CHANNELS = 64, 3
CHUNK_ENV = "DFFT_SCRATCH_CHUNK_BYTES"       # the general chunk cap, read once per call
LONG_M = 16384                               # the smallest padded length of the long families: 64 x 128
LONG_SPILL_M = XL.mid_length(384)            # dfft_rxspec1d_long: N2 = 384 spills in fp64 (rxspec1d_long_cases.ROUTED)


def chunks_cap(prec):
    """The cap of the several-chunk ops of rconv1d / rconv1d_os / rxspec1d: four rows of dfft_rconv1d at m = 72 (37 bins and 72 reals)"""
    return 4 * (37 * ESIZE[prec] + 72 * ESIZE[prec] // 2)


def ops_of(prec):
    """Every op of one precision, in a fixed order"""
    out = []
    f64 = prec == "f64"
    # four-step rows and columns at n = 8192
    out.append(complex_1d("rows-8192", "dfft_fft1d_rows", "four-step", 8192, (4, 8192), prec, base=2))
    out.append(complex_1d("cols-8192", "dfft_fft1d_cols", "four-step", 8192, (2, 8192, 4), prec, direction=BWD, base=2))
    # dfft_fft1d_any with Bluestein: one launch, multi-pass by the switch, multi-pass by its length, Bluestein over four-step
    out.append(complex_1d("any-97-one-launch", "dfft_fft1d_any", "bluestein", 97, (2, 97, 3), prec, flag=NO_LEASE))
    out.append(complex_1d("any-97-multi-pass", "dfft_fft1d_any", "bluestein", 97, (2, 97, 3), prec, direction=BWD,
                          switches={"DFFT_BLUESTEIN_FUSED": 0}))
    out.append(complex_1d("any-2053", "dfft_fft1d_any", "bluestein", 2053, (3, 2053), prec))
    out.append(complex_1d("any-10007", "dfft_fft1d_any", "bluestein", 10007, (2, 10007), prec))
    # dfft_rfft1d: half-length (nothing leased; backward with an untuned half copies the bins), paired single-pass, paired generic, Bluestein
    out.append(real_1d("rfft-512", "real", 512, 1, prec, FWD, NO_LEASE, False))
    out.append(real_1d("irfft-512", "real", 512, 1, prec, BWD, NO_LEASE, False))
    out.append(real_1d("irfft-72-untuned-half", "real", 72, 1, prec, BWD, LEASES, False))
    out.append(real_1d("rfft-243", "real", 243, 1, prec, FWD, NO_LEASE, False))
    out.append(real_1d("irfft-243", "real", 243, 1, prec, BWD, NO_LEASE, False))
    out.append(real_1d("rfft-375", "real", 375, 1, prec, FWD, LEASES, False))
    out.append(real_1d("rfft-1009", "real-bluestein", 1009, 1, prec, FWD, LEASES, False))
    out.append(real_1d("irfft-1009", "real-bluestein", 1009, 1, prec, BWD, LEASES, False))
    # dfft_rfft1d_strided: one launch, and the composed routes (it has no switch: a generic and a Bluestein length)
    out.append(real_1d("rfft-cols-243", "real", 243, 6, prec, FWD, NO_LEASE, True))
    out.append(real_1d("irfft-cols-243", "real", 243, 6, prec, BWD, NO_LEASE, True))
    out.append(real_1d("rfft-cols-375", "real", 375, 7, prec, FWD, LEASES, True))
    out.append(real_1d("irfft-cols-1009", "real-bluestein", 1009, 6, prec, BWD, LEASES, True))
    # dfft_r2r1d_strided, every kind: one launch, composed by DFFT_R2R_FUSED=0, composed with a Bluestein length; a generic length twice
    for kind in A.R2R_KINDS:
        out.append(r2r_1d(f"{kind}-243", "r2r", 243, 6, kind, prec, NO_LEASE))
        out.append(r2r_1d(f"{kind}-243-composed", "r2r", 243, 6, kind, prec, LEASES, {"DFFT_R2R_FUSED": 0}))
        out.append(r2r_1d(f"{kind}-97", "r2r-bluestein", 97, 7, kind, prec, LEASES))
    out.append(r2r_1d("dct2-375", "r2r", 375, 7, "dct2", prec, LEASES))
    out.append(r2r_1d("dst3-375-rows", "r2r", 375, 1, "dst3", prec, LEASES))
    # 2-D
    out.append(real_2d("rfft2-64x96", 64, 96, 3, prec, FWD, NO_LEASE))
    out.append(real_2d("irfft2-64x96", 64, 96, 3, prec, BWD, LEASES))
    out.append(complex_2d("fft2-256x256", "2d-one-launch", 256, 256, 2, prec, FWD, NO_LEASE))     # fp64: the one-launch stage
    out.append(complex_2d("fft2-64x96", "2d", 64, 96, 3, prec, BWD, NO_LEASE))
    out.append(complex_2d("fft2-8192x8", "2d", 8192, 8, 2, prec, FWD, LEASES))                   # a four-step axis
    # dfft_rconv1d / dfft_rconv1d_os: one launch, composed by DFFT_RCONV_FUSED=0, composed with an untuned half (the bins are copied)
    out.append(rconv1d("rconv-64", 64, 128, 3, "complex", prec, NO_LEASE))
    out.append(rconv1d("rconv-64-composed", 64, 63, 3, "real", prec, LEASES, {"DFFT_RCONV_FUSED": 0}))
    out.append(rconv1d("rconv-36-untuned", 36, 72, 3, "complex", prec, LEASES))
    out.append(rconv1d_os("osconv-64", 64, 32, 240, 272, "complex", prec, NO_LEASE))
    out.append(rconv1d_os("osconv-64-composed", 64, 33, 237, 237, "real", prec, LEASES, {"DFFT_RCONV_FUSED": 0}))
    out.append(rconv1d_os("osconv-36-untuned", 36, 10, 155, 165, "complex", prec, LEASES))
    # the same two composed in several chunks, and dfft_rxspec1d with them (an untuned half: composed by itself), under ONE cap -- four
    # rows of the convolution, so that host threads can share the environment: 21 rows in chunks of 4, 18 items in chunks of 4, 21 rows
    # in chunks of 2
    capped = {CHUNK_ENV: chunks_cap(prec)}
    out.append(rconv1d("rconv-36-chunks", 36, 72, 3, "complex", prec, LEASES, capped, batch=7))
    out.append(rconv1d_os("osconv-36-chunks", 36, 10, 155, 165, "complex", prec, LEASES, capped))
    out.append(rxspec1d("rxspec-cross-chunks", 36, 72, 3, 7, False, prec, LEASES, capped))
    # dfft_stft1d: one launch, composed, composed in several chunks (five items each), the power form, an untuned half
    chunked = lambda kind: {"DFFT_STFT_FUSED": 0, "DFFT_STFT_CHUNK_BYTES": 5 * stft_item_bytes(128, prec, kind)}  # noqa: E731
    out.append(stft1d("stft-64", STFT_BASE, "reflect", "complex", prec, NO_LEASE))
    out.append(stft1d("stft-64-power", STFT_BASE, "zero", "power", prec, NO_LEASE))
    out.append(stft1d("stft-64-composed", STFT_BASE, "reflect", "complex", prec, LEASES, {"DFFT_STFT_FUSED": 0}))
    out.append(stft1d("stft-64-composed-power", STFT_BASE, "zero", "power", prec, LEASES, {"DFFT_STFT_FUSED": 0}))
    out.append(stft1d("stft-64-chunks", STFT_BASE, "reflect", "complex", prec, LEASES, chunked("complex")))
    out.append(stft1d("stft-64-chunks-power", STFT_BASE, "zero", "power", prec, LEASES, chunked("power")))
    out.append(stft1d("stft-18-untuned", (18, 5, 3, 77, "rect"), "zero", "complex", prec, LEASES))
    # dfft_istft1d: whole rows, rows cut into chunks of five frames, an untuned half (the bins are copied)
    out.append(istft1d("istft-64", ISTFT_BASE, prec))
    out.append(istft1d("istft-64-chunks", ISTFT_BASE, prec, {"DFFT_STFT_CHUNK_BYTES": 5 * istft_item_bytes(128, prec, True)}))
    out.append(istft1d("istft-18-untuned", (18, 7, 0, 11, "rect"), prec))
    # dfft_rcsd1d, cross and auto: one launch with one slice and with several, composed, composed in several chunks
    frames = WC.frame_counts(RCSD_M, RCSD_ROWS)[1]
    assert WC.slices_rule(RCSD_M, RCSD_ROWS, frames) >= 2
    for autos in (False, True):
        tag = "auto" if autos else "cross"
        out.append(rcsd1d(f"rcsd-{tag}-one-slice", RCSD_M, RCSD_ROWS, 1, RCSD_M, autos, prec, NO_LEASE))
        out.append(rcsd1d(f"rcsd-{tag}-slices", RCSD_M, RCSD_ROWS, frames, RCSD_M, autos, prec, LEASES))
        out.append(rcsd1d(f"rcsd-{tag}-composed", RCSD_M, RCSD_ROWS, frames, RCSD_M, autos, prec, LEASES, {"DFFT_RCSD_FUSED": 0}))
        out.append(rcsd1d(f"rcsd-{tag}-chunks", RCSD_M, RCSD_ROWS, frames, RCSD_M + 1, autos, prec, LEASES,
                          {"DFFT_RCSD_FUSED": 0, "DFFT_RCSD_CHUNK_BYTES": 5 * rcsd_item_bytes(2 * RCSD_M, prec)}))
    # dfft_rxspec1d, cross and auto: one launch with one slice and with several, composed
    batch = XC.batches(RXSPEC_M, RXSPEC_CHANNELS)[1]
    assert XC.slices_rule(RXSPEC_M, RXSPEC_CHANNELS, batch) >= 2
    for autos in (False, True):
        tag = "auto" if autos else "cross"
        out.append(rxspec1d(f"rxspec-{tag}-one-slice", RXSPEC_M, 128, RXSPEC_CHANNELS, 1, autos, prec, NO_LEASE))
        out.append(rxspec1d(f"rxspec-{tag}-slices", RXSPEC_M, 63, RXSPEC_CHANNELS, batch, autos, prec, LEASES))
        out.append(rxspec1d(f"rxspec-{tag}-composed", RXSPEC_M, 128, RXSPEC_CHANNELS, batch, autos, prec, LEASES, {"DFFT_RXSPEC_FUSED": 0}))
    # dfft_rxspec1d_long: fused with several slices (cross in natural order, auto in the filter's order), composed by the switch, and in
    # fp64 the composed route a spilling split takes by itself
    lb = XL.ragged_batch(LONG_M)
    assert XL.call_slices(LONG_M, 1, lb, prec) >= 2
    out.append(rxspec1d_long("lxspec-cross-slices", LONG_M, LONG_M // 2 + 1, 1, lb, False, 0, prec))
    out.append(rxspec1d_long("lxspec-auto-slices", LONG_M, LONG_M // 2, 1, lb, True, 1, prec))
    out.append(rxspec1d_long("lxspec-cross-composed", LONG_M, LONG_M // 2 + 1, 3, 2, False, 0, prec, {"DFFT_RXSPEC_LONG_FUSED": 0}))
    if f64:
        out.append(rxspec1d_long("lxspec-cross-spilling-split", LONG_SPILL_M, LONG_SPILL_M // 2 + 1, 1, 2, False, 1, prec))
    # dfft_rconv1d_long: three launches, and the composed route by the switch
    out.append(rconv1d_long("lconv-16384", LONG_M, LONG_M // 2 + 1, "complex", prec))
    out.append(rconv1d_long("lconv-16384-composed", LONG_M, LONG_M, "real", prec, {"DFFT_RCONV_LONG_FUSED": 0}))
    return out


REGISTRY = ops_of("f64") + ops_of("f32")
BY_NAME = {op.name: op for op in REGISTRY}
assert len(BY_NAME) == len(REGISTRY), "op names repeat"


def ops(prec=None):
    return [op for op in REGISTRY if prec is None or op.prec == prec]


def long_op(prec="f64"):
    """Four-step rows, n = 65536, 64 rows: 64 MiB in fp64, still running when the next call is enqueued (not part of the tours)"""
    return complex_1d("rows-65536x64", "dfft_fft1d_rows", "four-step", 65536, (64, 65536), prec, base=2)


# ---- the tour -----------------------------------------------------------------------------------------------------------------------------
def tour(k):
    """A closed walk over the ops 0 ... k - 1 in which every ordered pair (a, b), a != b, is a pair of neighbours exactly once: an Eulerian
    circuit of the complete directed graph on k vertices (every vertex has k - 1 edges in and k - 1 out), by Hierholzer's algorithm with
    the edges taken in ascending order -- deterministic, of length k (k - 1) + 1."""
    if k < 2:
        return list(range(k))
    nxt = {a: [b for b in range(k - 1, -1, -1) if b != a] for a in range(k)}   # popped from the end: ascending
    stack, walk = [0], []
    while stack:
        v = stack[-1]
        if nxt[v]:
            stack.append(nxt[v].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    return walk
