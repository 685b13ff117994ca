"""The argument checks of the six plan-creating entry points and of the plan-less transforms, pinned exactly: for every row of the
tables below the return code AND the text of dfft_last_error() are what the library gave when the tables were recorded.  Per entry
point the rows follow the order in which the code tests its arguments -- first one fault at a time, then two faults at once for
adjacent checks, so that the order of the checks is pinned too (the first failing check decides code and message).  Every row is
refused before the device is queried (fake non-null pointers, no communicator), so the result is the same with and without a GPU."""
import ctypes as C

import pytest

A, B, D = 0x10000000, 0x20000000, 0x30000000  # never dereferenced


def _lib():
    from distributedfft_amd import _lib
    return _lib.load()


def _create(entry, plan=True, n=(64, 64, 64), dtype=0, direction=1, inp=A, out=B, P=1, g=0, flags=0, outs=(B, D), nout=None):
    """One call of a plan-creating entry point without a communicator; `outs` / `nout` are dfft_plan_create_conv_real_multi's."""
    lib = _lib()
    h = C.c_void_p()
    hp = C.byref(h) if plan else None
    if entry in ("dfft_plan_create", "dfft_plan_create_r2c", "dfft_plan_create_r2c_any"):
        rc = getattr(lib, entry)(hp, *n, dtype, direction, inp, out, None, g, P, flags)
    elif entry in ("dfft_plan_create_conv", "dfft_plan_create_conv_real"):
        rc = getattr(lib, entry)(hp, *n, dtype, inp, out, None, g, P, flags)
    else:
        arr = None if outs is None else (C.c_void_p * len(outs))(*outs)
        count = nout if nout is not None else (len(outs) if outs is not None else 1)
        rc = lib.dfft_plan_create_conv_real_multi(hp, *n, dtype, inp, arr, count, None, g, P, flags)
    assert h.value is None, "a refused create must not hand out a plan"
    return rc, lib.dfft_last_error().decode()


def _call(entry, args):
    """A plan-less entry point on its positional arguments (the stream, always NULL, is appended)."""
    lib = _lib()
    rc = getattr(lib, entry)(*args, None)
    return rc, lib.dfft_last_error().decode()


# Recorded from the library; keys of the create rows are _create's keyword arguments (defaults: a valid 64^3 fp64 forward call on one
# device, out of place), the rows of the plan-less entry points are their C arguments without the stream.
# ---- TABLE BEGIN
CREATE_TABLE = {
    "dfft_plan_create": [
        ({'out': A + 16}, -1, 'dfft_plan_create: in and out overlap partly (a plan runs out of place or exactly in place)'),
        ({'out': A - 16}, -1, 'dfft_plan_create: in and out overlap partly (a plan runs out of place or exactly in place)'),
        ({'plan': False}, -1, 'dfft_plan_create: null plan/in'),
        ({'inp': None}, -1, 'dfft_plan_create: null plan/in'),
        ({'n': (0, 64, 64)}, -1, 'dfft_plan_create: sizes must be positive'),
        ({'n': (64, -1, 64)}, -1, 'dfft_plan_create: sizes must be positive'),
        ({'n': (64, 64, 0)}, -1, 'dfft_plan_create: sizes must be positive'),
        ({'dtype': 2}, -1, 'dfft_plan_create: dtype'),
        ({'dtype': -1}, -1, 'dfft_plan_create: dtype'),
        ({'direction': 0}, -1, 'dfft_plan_create: direction'),
        ({'direction': 2}, -1, 'dfft_plan_create: direction'),
        ({'P': 0}, -1, 'dfft_plan_create: device index'),
        ({'g': -1}, -1, 'dfft_plan_create: device index'),
        ({'g': 1}, -1, 'dfft_plan_create: device index'),
        ({'P': 4, 'g': 4}, -1, 'dfft_plan_create: device index'),
        ({'P': 2}, -1, 'dfft_plan_create: a communicator is required for P > 1'),
        ({'P': 4, 'g': 3}, -1, 'dfft_plan_create: a communicator is required for P > 1'),
        ({'out': A + 16, 'direction': 0}, -1, 'dfft_plan_create: in and out overlap partly (a plan runs out of place or exactly in place)'),
        ({'out': A + 16, 'P': 2}, -1, 'dfft_plan_create: in and out overlap partly (a plan runs out of place or exactly in place)'),
        ({'inp': None, 'n': (0, 64, 64)}, -1, 'dfft_plan_create: null plan/in'),
        ({'plan': False, 'n': (64, 64, 0)}, -1, 'dfft_plan_create: null plan/in'),
        ({'n': (64, 0, 64), 'dtype': 2}, -1, 'dfft_plan_create: sizes must be positive'),
        ({'dtype': 2, 'direction': 0}, -1, 'dfft_plan_create: dtype'),
        ({'direction': 0, 'g': 1}, -1, 'dfft_plan_create: direction'),
        ({'P': 2, 'g': 2}, -1, 'dfft_plan_create: device index'),
    ],
    "dfft_plan_create_r2c": [
        ({'plan': False}, -1, 'dfft_plan_create_r2c: null plan/in'),
        ({'inp': None}, -1, 'dfft_plan_create_r2c: null plan/in'),
        ({'n': (0, 64, 64)}, -1, 'dfft_plan_create_r2c: sizes must be positive'),
        ({'n': (64, -1, 64)}, -1, 'dfft_plan_create_r2c: sizes must be positive'),
        ({'n': (64, 64, 0)}, -1, 'dfft_plan_create_r2c: sizes must be positive'),
        ({'dtype': 2}, -1, 'dfft_plan_create_r2c: dtype'),
        ({'direction': 0}, -1, 'dfft_plan_create_r2c: direction'),
        ({'P': 0}, -1, 'dfft_plan_create_r2c: device index'),
        ({'g': -1}, -1, 'dfft_plan_create_r2c: device index'),
        ({'g': 1}, -1, 'dfft_plan_create_r2c: device index'),
        ({'P': 2}, -1, 'dfft_plan_create_r2c: a communicator is required for P > 1'),
        ({'out': None}, -1, 'dfft_plan_create_r2c: real-to-complex plans are out of place (out != NULL, out != in)'),
        ({'out': A}, -1, 'dfft_plan_create_r2c: real-to-complex plans are out of place (out != NULL, out != in)'),
        ({'flags': 1}, -6, 'dfft_plan_create_r2c: only DFFT_PLAN_DEFAULT and DFFT_PLAN_INPUT_FROM_IN are supported (no OVERLAP, NATURAL or UNFUSED real-to-complex plans)'),
        ({'flags': 4}, -6, 'dfft_plan_create_r2c: only DFFT_PLAN_DEFAULT and DFFT_PLAN_INPUT_FROM_IN are supported (no OVERLAP, NATURAL or UNFUSED real-to-complex plans)'),
        ({'flags': 8}, -6, 'dfft_plan_create_r2c: only DFFT_PLAN_DEFAULT and DFFT_PLAN_INPUT_FROM_IN are supported (no OVERLAP, NATURAL or UNFUSED real-to-complex plans)'),
        ({'flags': 16}, -6, 'dfft_plan_create_r2c: only DFFT_PLAN_DEFAULT and DFFT_PLAN_INPUT_FROM_IN are supported (no OVERLAP, NATURAL or UNFUSED real-to-complex plans)'),
        ({'flags': 6}, -6, 'dfft_plan_create_r2c: only DFFT_PLAN_DEFAULT and DFFT_PLAN_INPUT_FROM_IN are supported (no OVERLAP, NATURAL or UNFUSED real-to-complex plans)'),
        ({'n': (64, 64, 9)}, -6, 'dfft_plan_create_r2c: N2 = 9 -- the real axis must be even with N2/2 a supported length of at most 4096'),
        ({'n': (64, 64, 1 << 30)}, -6, 'dfft_plan_create_r2c: N2 = 1073741824 -- the real axis must be even with N2/2 a supported length of at most 4096'),
        ({'n': (64, 64, 194)}, -6, 'dfft_plan_create_r2c: N2 = 194 -- the real axis must be even with N2/2 a supported length of at most 4096'),
        ({'n': (64, 64, 1)}, -6, 'dfft_plan_create_r2c: N2 = 1 -- the real axis must be even with N2/2 a supported length of at most 4096'),
        ({'n': (64, 64, 2)}, -6, 'dfft_plan_create_r2c: N2 = 2 -- the real axis must be even with N2/2 a supported length of at most 4096'),
        ({'n': (8192, 64, 64)}, -6, 'dfft_plan_create_r2c: FFT length 8192 -- N0 and N1 must be single-pass lengths (products of 2, 3, 5, 7 up to 4096)'),
        ({'n': (64, 97, 64)}, -6, 'dfft_plan_create_r2c: FFT length 97 -- N0 and N1 must be single-pass lengths (products of 2, 3, 5, 7 up to 4096)'),
        ({'n': (1 << 30, 64, 64)}, -6, 'dfft_plan_create_r2c: FFT length 1073741824 -- N0 and N1 must be single-pass lengths (products of 2, 3, 5, 7 up to 4096)'),
        ({'n': (4096, 4096, 256)}, -6, 'dfft_plan_create_r2c: more than 2^31 complex elements per device'),
        ({'inp': None, 'n': (0, 64, 64)}, -1, 'dfft_plan_create_r2c: null plan/in'),
        ({'n': (64, 0, 64), 'dtype': 2}, -1, 'dfft_plan_create_r2c: sizes must be positive'),
        ({'dtype': 2, 'direction': 0}, -1, 'dfft_plan_create_r2c: dtype'),
        ({'direction': 0, 'g': 1}, -1, 'dfft_plan_create_r2c: direction'),
        ({'P': 2, 'g': 2}, -1, 'dfft_plan_create_r2c: device index'),
        ({'P': 2, 'out': None}, -1, 'dfft_plan_create_r2c: a communicator is required for P > 1'),
        ({'out': A, 'flags': 1}, -1, 'dfft_plan_create_r2c: real-to-complex plans are out of place (out != NULL, out != in)'),
        ({'flags': 8, 'n': (64, 64, 1 << 30)}, -6, 'dfft_plan_create_r2c: only DFFT_PLAN_DEFAULT and DFFT_PLAN_INPUT_FROM_IN are supported (no OVERLAP, NATURAL or UNFUSED real-to-complex plans)'),
        ({'flags': 8, 'n': (64, 64, 9)}, -6, 'dfft_plan_create_r2c: only DFFT_PLAN_DEFAULT and DFFT_PLAN_INPUT_FROM_IN are supported (no OVERLAP, NATURAL or UNFUSED real-to-complex plans)'),
        ({'n': (97, 64, 1 << 30)}, -6, 'dfft_plan_create_r2c: N2 = 1073741824 -- the real axis must be even with N2/2 a supported length of at most 4096'),
        ({'n': (97, 64, 9)}, -6, 'dfft_plan_create_r2c: N2 = 9 -- the real axis must be even with N2/2 a supported length of at most 4096'),
        ({'n': (8192, 4096, 1)}, -6, 'dfft_plan_create_r2c: N2 = 1 -- the real axis must be even with N2/2 a supported length of at most 4096'),
        ({'n': (97, 64, 1)}, -6, 'dfft_plan_create_r2c: N2 = 1 -- the real axis must be even with N2/2 a supported length of at most 4096'),
    ],
    "dfft_plan_create_r2c_any": [
        ({'plan': False}, -1, 'dfft_plan_create_r2c_any: null plan/in'),
        ({'inp': None}, -1, 'dfft_plan_create_r2c_any: null plan/in'),
        ({'n': (0, 64, 64)}, -1, 'dfft_plan_create_r2c_any: sizes must be positive'),
        ({'n': (64, -1, 64)}, -1, 'dfft_plan_create_r2c_any: sizes must be positive'),
        ({'n': (64, 64, 0)}, -1, 'dfft_plan_create_r2c_any: sizes must be positive'),
        ({'dtype': 2}, -1, 'dfft_plan_create_r2c_any: dtype'),
        ({'direction': 0}, -1, 'dfft_plan_create_r2c_any: direction'),
        ({'P': 0}, -1, 'dfft_plan_create_r2c_any: device index'),
        ({'g': -1}, -1, 'dfft_plan_create_r2c_any: device index'),
        ({'g': 1}, -1, 'dfft_plan_create_r2c_any: device index'),
        ({'P': 2}, -1, 'dfft_plan_create_r2c_any: a communicator is required for P > 1'),
        ({'out': None}, -1, 'dfft_plan_create_r2c_any: real-to-complex plans are out of place (out != NULL, out != in)'),
        ({'out': A}, -1, 'dfft_plan_create_r2c_any: real-to-complex plans are out of place (out != NULL, out != in)'),
        ({'flags': 1}, -6, 'dfft_plan_create_r2c_any: only DFFT_PLAN_DEFAULT and DFFT_PLAN_INPUT_FROM_IN are supported (no OVERLAP, NATURAL or UNFUSED real-to-complex plans)'),
        ({'flags': 4}, -6, 'dfft_plan_create_r2c_any: only DFFT_PLAN_DEFAULT and DFFT_PLAN_INPUT_FROM_IN are supported (no OVERLAP, NATURAL or UNFUSED real-to-complex plans)'),
        ({'flags': 8}, -6, 'dfft_plan_create_r2c_any: only DFFT_PLAN_DEFAULT and DFFT_PLAN_INPUT_FROM_IN are supported (no OVERLAP, NATURAL or UNFUSED real-to-complex plans)'),
        ({'flags': 16}, -6, 'dfft_plan_create_r2c_any: only DFFT_PLAN_DEFAULT and DFFT_PLAN_INPUT_FROM_IN are supported (no OVERLAP, NATURAL or UNFUSED real-to-complex plans)'),
        ({'flags': 6}, -6, 'dfft_plan_create_r2c_any: only DFFT_PLAN_DEFAULT and DFFT_PLAN_INPUT_FROM_IN are supported (no OVERLAP, NATURAL or UNFUSED real-to-complex plans)'),
        ({'n': (64, 64, 1 << 30)}, -6, 'dfft_plan_create_r2c_any: N2 = 1073741824 -- no real form (at most 2^23, or a four-step length)'),
        ({'n': (64, 64, 1)}, -1, 'dfft_r2c_counts: bad arguments'),
        ({'n': (8192, 64, 64)}, -6, 'dfft_plan_create_r2c_any: FFT length 8192 -- N0 and N1 must be single-pass lengths (products of 2, 3, 5, 7 up to 4096)'),
        ({'n': (64, 97, 64)}, -6, 'dfft_plan_create_r2c_any: FFT length 97 -- N0 and N1 must be single-pass lengths (products of 2, 3, 5, 7 up to 4096)'),
        ({'n': (1 << 30, 64, 64)}, -6, 'dfft_plan_create_r2c_any: FFT length 1073741824 -- N0 and N1 must be single-pass lengths (products of 2, 3, 5, 7 up to 4096)'),
        ({'n': (4096, 4096, 256)}, -6, 'dfft_plan_create_r2c_any: more than 2^31 complex elements per device'),
        ({'inp': None, 'n': (0, 64, 64)}, -1, 'dfft_plan_create_r2c_any: null plan/in'),
        ({'n': (64, 0, 64), 'dtype': 2}, -1, 'dfft_plan_create_r2c_any: sizes must be positive'),
        ({'dtype': 2, 'direction': 0}, -1, 'dfft_plan_create_r2c_any: dtype'),
        ({'direction': 0, 'g': 1}, -1, 'dfft_plan_create_r2c_any: direction'),
        ({'P': 2, 'g': 2}, -1, 'dfft_plan_create_r2c_any: device index'),
        ({'P': 2, 'out': None}, -1, 'dfft_plan_create_r2c_any: a communicator is required for P > 1'),
        ({'out': A, 'flags': 1}, -1, 'dfft_plan_create_r2c_any: real-to-complex plans are out of place (out != NULL, out != in)'),
        ({'flags': 8, 'n': (64, 64, 1 << 30)}, -6, 'dfft_plan_create_r2c_any: only DFFT_PLAN_DEFAULT and DFFT_PLAN_INPUT_FROM_IN are supported (no OVERLAP, NATURAL or UNFUSED real-to-complex plans)'),
        ({'flags': 8, 'n': (64, 64, 9)}, -6, 'dfft_plan_create_r2c_any: only DFFT_PLAN_DEFAULT and DFFT_PLAN_INPUT_FROM_IN are supported (no OVERLAP, NATURAL or UNFUSED real-to-complex plans)'),
        ({'n': (97, 64, 1 << 30)}, -6, 'dfft_plan_create_r2c_any: N2 = 1073741824 -- no real form (at most 2^23, or a four-step length)'),
        ({'n': (97, 64, 9)}, -6, 'dfft_plan_create_r2c_any: FFT length 97 -- N0 and N1 must be single-pass lengths (products of 2, 3, 5, 7 up to 4096)'),
        ({'n': (8192, 4096, 1)}, -6, 'dfft_plan_create_r2c_any: FFT length 8192 -- N0 and N1 must be single-pass lengths (products of 2, 3, 5, 7 up to 4096)'),
        ({'n': (97, 64, 1)}, -6, 'dfft_plan_create_r2c_any: FFT length 97 -- N0 and N1 must be single-pass lengths (products of 2, 3, 5, 7 up to 4096)'),
    ],
    "dfft_plan_create_conv": [
        ({'plan': False}, -1, 'dfft_plan_create_conv: null plan/in'),
        ({'inp': None}, -1, 'dfft_plan_create_conv: null plan/in'),
        ({'n': (0, 64, 64)}, -1, 'dfft_plan_create_conv: sizes must be positive'),
        ({'n': (64, -1, 64)}, -1, 'dfft_plan_create_conv: sizes must be positive'),
        ({'n': (64, 64, 0)}, -1, 'dfft_plan_create_conv: sizes must be positive'),
        ({'dtype': 2}, -1, 'dfft_plan_create_conv: dtype'),
        ({'P': 0}, -1, 'dfft_plan_create_conv: device index'),
        ({'g': -1}, -1, 'dfft_plan_create_conv: device index'),
        ({'g': 1}, -1, 'dfft_plan_create_conv: device index'),
        ({'P': 2}, -1, 'dfft_plan_create_conv: a communicator is required for P > 1'),
        ({'flags': 1}, -6, 'dfft_plan_create_conv: only DFFT_PLAN_DEFAULT is supported (no OVERLAP, NATURAL, UNFUSED, INPUT_FROM_IN -- which is implied -- or ANY_LENGTH spectral-filter plans)'),
        ({'flags': 2}, -6, 'dfft_plan_create_conv: only DFFT_PLAN_DEFAULT is supported (no OVERLAP, NATURAL, UNFUSED, INPUT_FROM_IN -- which is implied -- or ANY_LENGTH spectral-filter plans)'),
        ({'flags': 4}, -6, 'dfft_plan_create_conv: only DFFT_PLAN_DEFAULT is supported (no OVERLAP, NATURAL, UNFUSED, INPUT_FROM_IN -- which is implied -- or ANY_LENGTH spectral-filter plans)'),
        ({'flags': 8}, -6, 'dfft_plan_create_conv: only DFFT_PLAN_DEFAULT is supported (no OVERLAP, NATURAL, UNFUSED, INPUT_FROM_IN -- which is implied -- or ANY_LENGTH spectral-filter plans)'),
        ({'flags': 16}, -6, 'dfft_plan_create_conv: only DFFT_PLAN_DEFAULT is supported (no OVERLAP, NATURAL, UNFUSED, INPUT_FROM_IN -- which is implied -- or ANY_LENGTH spectral-filter plans)'),
        ({'n': (8192, 64, 64)}, -6, 'dfft_plan_create_conv: FFT length 8192 -- every axis must be a single-pass length (products of 2, 3, 5, 7 up to 4096)'),
        ({'n': (64, 97, 64)}, -6, 'dfft_plan_create_conv: FFT length 97 -- every axis must be a single-pass length (products of 2, 3, 5, 7 up to 4096)'),
        ({'n': (64, 64, 8192)}, -6, 'dfft_plan_create_conv: FFT length 8192 -- every axis must be a single-pass length (products of 2, 3, 5, 7 up to 4096)'),
        ({'n': (64, 64, 97)}, -6, 'dfft_plan_create_conv: FFT length 97 -- every axis must be a single-pass length (products of 2, 3, 5, 7 up to 4096)'),
        ({'out': A + 16}, -1, 'dfft_plan_create_conv: in and out overlap partly (a plan runs out of place or exactly in place)'),
        ({'out': A - 16}, -1, 'dfft_plan_create_conv: in and out overlap partly (a plan runs out of place or exactly in place)'),
        ({'inp': None, 'n': (0, 64, 64)}, -1, 'dfft_plan_create_conv: null plan/in'),
        ({'n': (64, 0, 64), 'dtype': 2}, -1, 'dfft_plan_create_conv: sizes must be positive'),
        ({'dtype': 2, 'g': 1}, -1, 'dfft_plan_create_conv: dtype'),
        ({'P': 2, 'g': 2}, -1, 'dfft_plan_create_conv: device index'),
        ({'P': 2, 'flags': 1}, -1, 'dfft_plan_create_conv: a communicator is required for P > 1'),
        ({'flags': 2, 'n': (97, 64, 64)}, -6, 'dfft_plan_create_conv: only DFFT_PLAN_DEFAULT is supported (no OVERLAP, NATURAL, UNFUSED, INPUT_FROM_IN -- which is implied -- or ANY_LENGTH spectral-filter plans)'),
        ({'n': (64, 64, 97), 'out': A + 16}, -6, 'dfft_plan_create_conv: FFT length 97 -- every axis must be a single-pass length (products of 2, 3, 5, 7 up to 4096)'),
        ({'n': (97, 8192, 64)}, -6, 'dfft_plan_create_conv: FFT length 97 -- every axis must be a single-pass length (products of 2, 3, 5, 7 up to 4096)'),
    ],
    "dfft_plan_create_conv_real": [
        ({'plan': False}, -1, 'dfft_plan_create_conv_real: null plan/in'),
        ({'inp': None}, -1, 'dfft_plan_create_conv_real: null plan/in'),
        ({'n': (0, 64, 64)}, -1, 'dfft_plan_create_conv_real: sizes must be positive'),
        ({'n': (64, -1, 64)}, -1, 'dfft_plan_create_conv_real: sizes must be positive'),
        ({'n': (64, 64, 0)}, -1, 'dfft_plan_create_conv_real: sizes must be positive'),
        ({'dtype': 2}, -1, 'dfft_plan_create_conv_real: dtype'),
        ({'P': 0}, -1, 'dfft_plan_create_conv_real: device index'),
        ({'g': -1}, -1, 'dfft_plan_create_conv_real: device index'),
        ({'g': 1}, -1, 'dfft_plan_create_conv_real: device index'),
        ({'P': 2}, -1, 'dfft_plan_create_conv_real: a communicator is required for P > 1'),
        ({'flags': 1}, -6, 'dfft_plan_create_conv_real: only DFFT_PLAN_DEFAULT is supported (no OVERLAP, NATURAL, UNFUSED, INPUT_FROM_IN -- which is implied -- or ANY_LENGTH spectral-filter plans)'),
        ({'flags': 2}, -6, 'dfft_plan_create_conv_real: only DFFT_PLAN_DEFAULT is supported (no OVERLAP, NATURAL, UNFUSED, INPUT_FROM_IN -- which is implied -- or ANY_LENGTH spectral-filter plans)'),
        ({'flags': 4}, -6, 'dfft_plan_create_conv_real: only DFFT_PLAN_DEFAULT is supported (no OVERLAP, NATURAL, UNFUSED, INPUT_FROM_IN -- which is implied -- or ANY_LENGTH spectral-filter plans)'),
        ({'flags': 8}, -6, 'dfft_plan_create_conv_real: only DFFT_PLAN_DEFAULT is supported (no OVERLAP, NATURAL, UNFUSED, INPUT_FROM_IN -- which is implied -- or ANY_LENGTH spectral-filter plans)'),
        ({'flags': 16}, -6, 'dfft_plan_create_conv_real: only DFFT_PLAN_DEFAULT is supported (no OVERLAP, NATURAL, UNFUSED, INPUT_FROM_IN -- which is implied -- or ANY_LENGTH spectral-filter plans)'),
        ({'n': (8192, 64, 64)}, -6, 'dfft_plan_create_conv_real: FFT length 8192 -- N0 and N1 must be single-pass lengths (products of 2, 3, 5, 7 up to 4096)'),
        ({'n': (64, 97, 64)}, -6, 'dfft_plan_create_conv_real: FFT length 97 -- N0 and N1 must be single-pass lengths (products of 2, 3, 5, 7 up to 4096)'),
        ({'n': (64, 64, 9)}, -6, 'dfft_plan_create_conv_real: N2 = 9 -- the real axis must be of dfft_real_form 1 (even, N2/2 a single-pass length)'),
        ({'n': (64, 64, 194)}, -6, 'dfft_plan_create_conv_real: N2 = 194 -- the real axis must be of dfft_real_form 1 (even, N2/2 a single-pass length)'),
        ({'n': (64, 64, 1 << 30)}, -6, 'dfft_plan_create_conv_real: N2 = 1073741824 -- the real axis must be of dfft_real_form 1 (even, N2/2 a single-pass length)'),
        ({'n': (64, 64, 2)}, -6, 'dfft_plan_create_conv_real: N2 = 2 -- the real axis must be of dfft_real_form 1 (even, N2/2 a single-pass length)'),
        ({'n': (4096, 4096, 256)}, -6, 'dfft_plan_create_conv_real: more than 2^31 complex elements per device'),
        ({'inp': None, 'n': (0, 64, 64)}, -1, 'dfft_plan_create_conv_real: null plan/in'),
        ({'n': (64, 0, 64), 'dtype': 2}, -1, 'dfft_plan_create_conv_real: sizes must be positive'),
        ({'dtype': 2, 'g': 1}, -1, 'dfft_plan_create_conv_real: dtype'),
        ({'P': 2, 'g': 2}, -1, 'dfft_plan_create_conv_real: device index'),
        ({'P': 2, 'flags': 1}, -1, 'dfft_plan_create_conv_real: a communicator is required for P > 1'),
        ({'flags': 2, 'n': (97, 64, 64)}, -6, 'dfft_plan_create_conv_real: only DFFT_PLAN_DEFAULT is supported (no OVERLAP, NATURAL, UNFUSED, INPUT_FROM_IN -- which is implied -- or ANY_LENGTH spectral-filter plans)'),
        ({'n': (64, 97, 9)}, -6, 'dfft_plan_create_conv_real: FFT length 97 -- N0 and N1 must be single-pass lengths (products of 2, 3, 5, 7 up to 4096)'),
        ({'n': (97, 8192, 64)}, -6, 'dfft_plan_create_conv_real: FFT length 97 -- N0 and N1 must be single-pass lengths (products of 2, 3, 5, 7 up to 4096)'),
    ],
    "dfft_plan_create_conv_real_multi": [
        ({'outs': None}, -1, 'dfft_plan_create_conv_real_multi: outs is NULL'),
        ({'outs': None, 'nout': 0}, -1, 'dfft_plan_create_conv_real_multi: outs is NULL'),
        ({'nout': 0}, -1, 'dfft_plan_create_conv_real_multi: noutputs must be 1 .. 8'),
        ({'nout': 9}, -1, 'dfft_plan_create_conv_real_multi: noutputs must be 1 .. 8'),
        ({'nout': -1}, -1, 'dfft_plan_create_conv_real_multi: noutputs must be 1 .. 8'),
        ({'plan': False}, -1, 'dfft_plan_create_conv_real_multi: null plan/in'),
        ({'inp': None}, -1, 'dfft_plan_create_conv_real_multi: null plan/in'),
        ({'outs': (None,)}, -1, 'dfft_plan_create_conv_real_multi: outs[0] is NULL'),
        ({'outs': (B, None)}, -1, 'dfft_plan_create_conv_real_multi: outs[1] is NULL'),
        ({'outs': (B, B)}, -1, 'dfft_plan_create_conv_real_multi: outs[0] and outs[1] are the same buffer'),
        ({'outs': (B, D, B)}, -1, 'dfft_plan_create_conv_real_multi: outs[0] and outs[2] are the same buffer'),
        ({'outs': (B, D, D)}, -1, 'dfft_plan_create_conv_real_multi: outs[1] and outs[2] are the same buffer'),
        ({'n': (0, 64, 64)}, -1, 'dfft_plan_create_conv_real_multi: sizes must be positive'),
        ({'n': (64, -1, 64)}, -1, 'dfft_plan_create_conv_real_multi: sizes must be positive'),
        ({'n': (64, 64, 0)}, -1, 'dfft_plan_create_conv_real_multi: sizes must be positive'),
        ({'dtype': 2}, -1, 'dfft_plan_create_conv_real_multi: dtype'),
        ({'P': 0}, -1, 'dfft_plan_create_conv_real_multi: device index'),
        ({'g': -1}, -1, 'dfft_plan_create_conv_real_multi: device index'),
        ({'g': 1}, -1, 'dfft_plan_create_conv_real_multi: device index'),
        ({'P': 2}, -1, 'dfft_plan_create_conv_real_multi: a communicator is required for P > 1'),
        ({'flags': 1}, -6, 'dfft_plan_create_conv_real_multi: only DFFT_PLAN_DEFAULT is supported (no OVERLAP, NATURAL, UNFUSED, INPUT_FROM_IN -- which is implied -- or ANY_LENGTH spectral-filter plans)'),
        ({'flags': 2}, -6, 'dfft_plan_create_conv_real_multi: only DFFT_PLAN_DEFAULT is supported (no OVERLAP, NATURAL, UNFUSED, INPUT_FROM_IN -- which is implied -- or ANY_LENGTH spectral-filter plans)'),
        ({'flags': 4}, -6, 'dfft_plan_create_conv_real_multi: only DFFT_PLAN_DEFAULT is supported (no OVERLAP, NATURAL, UNFUSED, INPUT_FROM_IN -- which is implied -- or ANY_LENGTH spectral-filter plans)'),
        ({'flags': 8}, -6, 'dfft_plan_create_conv_real_multi: only DFFT_PLAN_DEFAULT is supported (no OVERLAP, NATURAL, UNFUSED, INPUT_FROM_IN -- which is implied -- or ANY_LENGTH spectral-filter plans)'),
        ({'flags': 16}, -6, 'dfft_plan_create_conv_real_multi: only DFFT_PLAN_DEFAULT is supported (no OVERLAP, NATURAL, UNFUSED, INPUT_FROM_IN -- which is implied -- or ANY_LENGTH spectral-filter plans)'),
        ({'n': (8192, 64, 64)}, -6, 'dfft_plan_create_conv_real_multi: FFT length 8192 -- N0 and N1 must be single-pass lengths (products of 2, 3, 5, 7 up to 4096)'),
        ({'n': (64, 97, 64)}, -6, 'dfft_plan_create_conv_real_multi: FFT length 97 -- N0 and N1 must be single-pass lengths (products of 2, 3, 5, 7 up to 4096)'),
        ({'n': (64, 64, 9)}, -6, 'dfft_plan_create_conv_real_multi: N2 = 9 -- the real axis must be of dfft_real_form 1 (even, N2/2 a single-pass length)'),
        ({'n': (64, 64, 194)}, -6, 'dfft_plan_create_conv_real_multi: N2 = 194 -- the real axis must be of dfft_real_form 1 (even, N2/2 a single-pass length)'),
        ({'n': (64, 64, 1 << 30)}, -6, 'dfft_plan_create_conv_real_multi: N2 = 1073741824 -- the real axis must be of dfft_real_form 1 (even, N2/2 a single-pass length)'),
        ({'n': (64, 64, 2)}, -6, 'dfft_plan_create_conv_real_multi: N2 = 2 -- the real axis must be of dfft_real_form 1 (even, N2/2 a single-pass length)'),
        ({'n': (4096, 4096, 256)}, -6, 'dfft_plan_create_conv_real_multi: more than 2^31 complex elements per device'),
        ({'outs': None, 'nout': 9}, -1, 'dfft_plan_create_conv_real_multi: outs is NULL'),
        ({'nout': 0, 'inp': None}, -1, 'dfft_plan_create_conv_real_multi: noutputs must be 1 .. 8'),
        ({'inp': None, 'outs': (B, None)}, -1, 'dfft_plan_create_conv_real_multi: null plan/in'),
        ({'outs': (B, None, B)}, -1, 'dfft_plan_create_conv_real_multi: outs[1] is NULL'),
        ({'outs': (B, B, None)}, -1, 'dfft_plan_create_conv_real_multi: outs[0] and outs[1] are the same buffer'),
        ({'outs': (B, B), 'n': (0, 64, 64)}, -1, 'dfft_plan_create_conv_real_multi: outs[0] and outs[1] are the same buffer'),
        ({'inp': None, 'n': (0, 64, 64)}, -1, 'dfft_plan_create_conv_real_multi: null plan/in'),
        ({'n': (64, 0, 64), 'dtype': 2}, -1, 'dfft_plan_create_conv_real_multi: sizes must be positive'),
        ({'dtype': 2, 'g': 1}, -1, 'dfft_plan_create_conv_real_multi: dtype'),
        ({'P': 2, 'g': 2}, -1, 'dfft_plan_create_conv_real_multi: device index'),
        ({'P': 2, 'flags': 1}, -1, 'dfft_plan_create_conv_real_multi: a communicator is required for P > 1'),
        ({'flags': 2, 'n': (97, 64, 64)}, -6, 'dfft_plan_create_conv_real_multi: only DFFT_PLAN_DEFAULT is supported (no OVERLAP, NATURAL, UNFUSED, INPUT_FROM_IN -- which is implied -- or ANY_LENGTH spectral-filter plans)'),
        ({'n': (64, 97, 9)}, -6, 'dfft_plan_create_conv_real_multi: FFT length 97 -- N0 and N1 must be single-pass lengths (products of 2, 3, 5, 7 up to 4096)'),
        ({'n': (97, 8192, 64)}, -6, 'dfft_plan_create_conv_real_multi: FFT length 97 -- N0 and N1 must be single-pass lengths (products of 2, 3, 5, 7 up to 4096)'),
    ],
}

BATCH_TABLE = {
    "dfft_fft1d_rows": [
        ((None, B, 64, 1, 0, 1), -1, 'dfft_fft1d_rows: bad arguments'),
        ((A, None, 64, 1, 0, 1), -1, 'dfft_fft1d_rows: bad arguments'),
        ((A, B, 64, -1, 0, 1), -1, 'dfft_fft1d_rows: bad arguments'),
        ((A, B, 64, 1, 2, 1), -1, 'dfft_fft1d_rows: bad arguments'),
        ((A, B, 64, 1, 0, 0), -1, 'dfft_fft1d_rows: bad arguments'),
        ((A, B, 0, 1, 0, 1), -6, 'dfft_fft1d_rows: unsupported length'),
        ((A, B, 11, 1, 0, 1), -6, 'dfft_fft1d_rows: unsupported length'),
        ((A, B, 1 << 30, 1, 1, -1), -6, 'dfft_fft1d_rows: unsupported length'),
        ((A, A + 16, 64, 4, 0, 1), -1, 'dfft_fft1d_rows: in and out overlap partly (the transform runs out of place or exactly in place)'),
        ((A, A - 16, 64, 4, 1, -1), -1, 'dfft_fft1d_rows: in and out overlap partly (the transform runs out of place or exactly in place)'),
        ((A, A + 8, 64, 1, 1, 1), -1, 'dfft_fft1d_rows: in and out overlap partly (the transform runs out of place or exactly in place)'),
        ((A, B, 0, 1, 2, 1), -1, 'dfft_fft1d_rows: bad arguments'),
        ((A, B, 1 << 30, 1, 0, 0), -1, 'dfft_fft1d_rows: bad arguments'),
        ((A, A + 16, 1 << 30, 4, 0, 1), -6, 'dfft_fft1d_rows: unsupported length'),
    ],
    "dfft_rfft1d": [
        ((None, B, 64, 1, 0, 1), -1, 'dfft_rfft1d: bad arguments'),
        ((A, None, 64, 1, 0, 1), -1, 'dfft_rfft1d: bad arguments'),
        ((A, B, 64, -1, 0, 1), -1, 'dfft_rfft1d: bad arguments'),
        ((A, B, 64, 1, 2, 1), -1, 'dfft_rfft1d: bad arguments'),
        ((A, B, 64, 1, 0, 0), -1, 'dfft_rfft1d: bad arguments'),
        ((A, B, 0, 1, 0, 1), -6, 'dfft_rfft1d: length 0 has no real form (at most 2^23, or a four-step length)'),
        ((A, B, 1 << 30, 1, 0, 1), -6, 'dfft_rfft1d: length 1073741824 has no real form (at most 2^23, or a four-step length)'),
        ((A, B, 1 << 30, 1, 1, -1), -6, 'dfft_rfft1d: length 1073741824 has no real form (at most 2^23, or a four-step length)'),
        ((A, A + 16, 64, 4, 0, 1), -1, 'dfft_rfft1d: in and out overlap (the transform is out of place)'),
        ((A, A - 16, 64, 4, 1, -1), -1, 'dfft_rfft1d: in and out overlap (the transform is out of place)'),
        ((A, A, 64, 4, 0, 1), -1, 'dfft_rfft1d: in and out overlap (the transform is out of place)'),
        ((A, B, 0, 1, 2, 1), -1, 'dfft_rfft1d: bad arguments'),
        ((A, B, 1 << 30, 1, 0, 0), -1, 'dfft_rfft1d: bad arguments'),
        ((A, A + 16, 1 << 30, 4, 0, 1), -6, 'dfft_rfft1d: length 1073741824 has no real form (at most 2^23, or a four-step length)'),
    ],
    "dfft_fft1d_cols": [
        ((None, B, 64, 4, 1, 0, 1), -1, 'dfft_fft1d_cols: bad arguments'),
        ((A, None, 64, 4, 1, 0, 1), -1, 'dfft_fft1d_cols: bad arguments'),
        ((A, B, 64, 4, -1, 0, 1), -1, 'dfft_fft1d_cols: bad arguments'),
        ((A, B, 64, 0, 1, 0, 1), -1, 'dfft_fft1d_cols: bad arguments'),
        ((A, B, 64, 4, 1, 2, 1), -1, 'dfft_fft1d_cols: bad arguments'),
        ((A, B, 64, 4, 1, 0, 0), -1, 'dfft_fft1d_cols: bad arguments'),
        ((A, B, 0, 4, 1, 0, 1), -6, 'dfft_fft1d_cols: unsupported length'),
        ((A, B, 1 << 30, 4, 1, 0, 1), -6, 'dfft_fft1d_cols: unsupported length'),
        ((A, B, 11, 4, 1, 1, -1), -6, 'dfft_fft1d_cols: unsupported length'),
        ((A, A + 16, 64, 4, 4, 0, 1), -1, 'dfft_fft1d_cols: in and out overlap partly (the transform runs out of place or exactly in place)'),
        ((A, A - 16, 64, 4, 4, 1, -1), -1, 'dfft_fft1d_cols: in and out overlap partly (the transform runs out of place or exactly in place)'),
        ((A, A + 8, 64, 1, 1, 1, 1), -1, 'dfft_fft1d_cols: in and out overlap partly (the transform runs out of place or exactly in place)'),
        ((A, B, 0, 0, 1, 0, 1), -1, 'dfft_fft1d_cols: bad arguments'),
        ((A, B, 1 << 30, 4, 1, 0, 2), -1, 'dfft_fft1d_cols: bad arguments'),
        ((A, A + 16, 1 << 30, 4, 4, 0, 1), -6, 'dfft_fft1d_cols: unsupported length'),
        ((A, A, 8, 1 << 31, 0, 0, 1), -6, 'dfft_fft1d_cols: n = 8, width = 2147483648: a column pass would span 2^32 or more 16-byte (fp32, odd width or unaligned: 8-byte) units, or width > 2^31 - 64'),
        ((A, A, 8192, 1 << 26, 0, 1, 1), -6, 'dfft_fft1d_cols: n = 8192, width = 67108864: a column pass would span 2^32 or more 16-byte (fp32, odd width or unaligned: 8-byte) units, or width > 2^31 - 64'),
        ((A, A, 4099, 1 << 31, 0, 0, 1), -6, 'dfft_fft1d_cols: unsupported length'),
    ],
    "dfft_fft1d_any": [
        ((None, B, 64, 4, 1, 0, 1), -1, 'dfft_fft1d_any: bad arguments'),
        ((A, None, 64, 4, 1, 0, 1), -1, 'dfft_fft1d_any: bad arguments'),
        ((A, B, 64, 4, -1, 0, 1), -1, 'dfft_fft1d_any: bad arguments'),
        ((A, B, 64, 0, 1, 0, 1), -1, 'dfft_fft1d_any: bad arguments'),
        ((A, B, 64, 4, 1, 2, 1), -1, 'dfft_fft1d_any: bad arguments'),
        ((A, B, 64, 4, 1, 0, 0), -1, 'dfft_fft1d_any: bad arguments'),
        ((A, B, 0, 4, 1, 0, 1), -6, 'dfft_fft1d_any: length 0 is outside every form (at most 2^23, or a four-step length)'),
        ((A, B, 1 << 30, 4, 1, 0, 1), -6, 'dfft_fft1d_any: length 1073741824 is outside every form (at most 2^23, or a four-step length)'),
        ((A, B, -5, 4, 1, 1, -1), -6, 'dfft_fft1d_any: length -5 is outside every form (at most 2^23, or a four-step length)'),
        ((A, A + 16, 64, 4, 4, 0, 1), -1, 'dfft_fft1d_any: in and out overlap partly (the transform runs out of place or exactly in place)'),
        ((A, A - 16, 64, 4, 4, 1, -1), -1, 'dfft_fft1d_any: in and out overlap partly (the transform runs out of place or exactly in place)'),
        ((A, A + 8, 64, 1, 1, 1, 1), -1, 'dfft_fft1d_any: in and out overlap partly (the transform runs out of place or exactly in place)'),
        ((A, B, 0, 0, 1, 0, 1), -1, 'dfft_fft1d_any: bad arguments'),
        ((A, B, 1 << 30, 4, 1, 0, 2), -1, 'dfft_fft1d_any: bad arguments'),
        ((A, A + 16, 1 << 30, 4, 4, 0, 1), -6, 'dfft_fft1d_any: length 1073741824 is outside every form (at most 2^23, or a four-step length)'),
        ((A, A, 8, 1 << 31, 0, 0, 1), -6, 'dfft_fft1d_cols: n = 8, width = 2147483648: a column pass would span 2^32 or more 16-byte (fp32, odd width or unaligned: 8-byte) units, or width > 2^31 - 64'),
        ((A, A, 8192, 1 << 26, 0, 1, 1), -6, 'dfft_fft1d_cols: n = 8192, width = 67108864: a column pass would span 2^32 or more 16-byte (fp32, odd width or unaligned: 8-byte) units, or width > 2^31 - 64'),
        ((A, A, 4099, 1 << 31, 0, 0, 1), -6, 'dfft_fft1d_any: n = 4099, width = 2147483648: a column pass would span 2^32 or more 16-byte (fp32, odd width or unaligned: 8-byte) units, or width > 2^31 - 64'),
    ],
    "dfft_rfft1d_strided": [
        ((None, B, 64, 4, 1, 0, 1), -1, 'dfft_rfft1d_strided: bad arguments'),
        ((A, None, 64, 4, 1, 0, 1), -1, 'dfft_rfft1d_strided: bad arguments'),
        ((A, B, 64, 4, -1, 0, 1), -1, 'dfft_rfft1d_strided: bad arguments'),
        ((A, B, 64, 0, 1, 0, 1), -1, 'dfft_rfft1d_strided: bad arguments'),
        ((A, B, 64, 4, 1, 2, 1), -1, 'dfft_rfft1d_strided: bad arguments'),
        ((A, B, 64, 4, 1, 0, 0), -1, 'dfft_rfft1d_strided: bad arguments'),
        ((A, B, 0, 4, 1, 0, 1), -6, 'dfft_rfft1d_strided: length 0 has no real form (at most 2^23, or a four-step length)'),
        ((A, B, 1 << 30, 4, 1, 0, 1), -6, 'dfft_rfft1d_strided: length 1073741824 has no real form (at most 2^23, or a four-step length)'),
        ((A, B, -5, 4, 1, 1, -1), -6, 'dfft_rfft1d_strided: length -5 has no real form (at most 2^23, or a four-step length)'),
        ((A, A + 16, 64, 4, 4, 0, 1), -1, 'dfft_rfft1d_strided: in and out overlap (the transform is out of place)'),
        ((A, A - 16, 64, 4, 4, 1, -1), -1, 'dfft_rfft1d_strided: in and out overlap (the transform is out of place)'),
        ((A, A, 64, 4, 4, 0, 1), -1, 'dfft_rfft1d_strided: in and out overlap (the transform is out of place)'),
        ((A, B, 0, 0, 1, 0, 1), -1, 'dfft_rfft1d_strided: bad arguments'),
        ((A, B, 1 << 30, 4, 1, 0, 2), -1, 'dfft_rfft1d_strided: bad arguments'),
        ((A, A + 16, 1 << 30, 4, 4, 0, 1), -6, 'dfft_rfft1d_strided: length 1073741824 has no real form (at most 2^23, or a four-step length)'),
        ((A, A, 8, 1 << 31, 0, 0, 1), -1, 'dfft_rfft1d_strided: in and out overlap (the transform is out of place)'),
        ((A, A, 8192, 1 << 26, 0, 1, 1), -1, 'dfft_rfft1d_strided: in and out overlap (the transform is out of place)'),
        ((A, A, 4099, 1 << 31, 0, 0, 1), -1, 'dfft_rfft1d_strided: in and out overlap (the transform is out of place)'),
    ],
    "dfft_fft2d_batch": [
        ((None, B, 64, 64, 1, 0, 1), -1, 'dfft_fft2d_batch: bad arguments'),
        ((A, None, 64, 64, 1, 0, 1), -1, 'dfft_fft2d_batch: bad arguments'),
        ((A, B, 0, 64, 1, 0, 1), -1, 'dfft_fft2d_batch: bad arguments'),
        ((A, B, 64, 0, 1, 0, 1), -1, 'dfft_fft2d_batch: bad arguments'),
        ((A, B, 64, 64, -1, 0, 1), -1, 'dfft_fft2d_batch: bad arguments'),
        ((A, B, 64, 64, 1, 2, 1), -1, 'dfft_fft2d_batch: bad arguments'),
        ((A, B, 64, 64, 1, 0, 0), -1, 'dfft_fft2d_batch: bad arguments'),
        ((A, B, 11, 64, 1, 0, 1), -6, 'dfft_fft2d_batch: unsupported length'),
        ((A, B, 64, 11, 1, 0, 1), -6, 'dfft_fft2d_batch: unsupported length'),
        ((A, B, 1 << 30, 1 << 30, 1, 0, 1), -6, 'dfft_fft2d_batch: unsupported length'),
        ((A, A + 16, 64, 64, 2, 0, 1), -1, 'dfft_fft2d_batch: in and out overlap partly (the transform runs out of place or exactly in place)'),
        ((A, A - 16, 64, 64, 2, 1, -1), -1, 'dfft_fft2d_batch: in and out overlap partly (the transform runs out of place or exactly in place)'),
        ((A, A + 8, 8, 8, 1, 1, 1), -1, 'dfft_fft2d_batch: in and out overlap partly (the transform runs out of place or exactly in place)'),
        ((A, B, 0, 1 << 30, 1, 0, 1), -1, 'dfft_fft2d_batch: bad arguments'),
        ((A, B, 1 << 30, 64, 1, 0, 0), -1, 'dfft_fft2d_batch: bad arguments'),
        ((A, A + 16, 64, 1 << 30, 2, 0, 1), -6, 'dfft_fft2d_batch: unsupported length'),
    ],
    "dfft_rfft2d_batch": [
        ((None, B, 64, 64, 1, 0, 1), -1, 'dfft_rfft2d_batch: bad arguments'),
        ((A, None, 64, 64, 1, 0, 1), -1, 'dfft_rfft2d_batch: bad arguments'),
        ((A, B, 0, 64, 1, 0, 1), -1, 'dfft_rfft2d_batch: bad arguments'),
        ((A, B, 64, 0, 1, 0, 1), -1, 'dfft_rfft2d_batch: bad arguments'),
        ((A, B, 64, 64, -1, 0, 1), -1, 'dfft_rfft2d_batch: bad arguments'),
        ((A, B, 64, 64, 1, 2, 1), -1, 'dfft_rfft2d_batch: bad arguments'),
        ((A, B, 64, 64, 1, 0, 0), -1, 'dfft_rfft2d_batch: bad arguments'),
        ((A, B, 1 << 30, 64, 1, 0, 1), -6, 'dfft_rfft2d_batch: n1 = 1073741824 is outside every form'),
        ((A, B, 64, 1 << 30, 1, 0, 1), -6, 'dfft_rfft2d_batch: n2 = 1073741824 has no real form'),
        ((A, B, 1 << 30, 1 << 30, 1, 0, 1), -6, 'dfft_rfft2d_batch: n2 = 1073741824 has no real form'),
        ((A, A + 16, 64, 64, 2, 0, 1), -1, 'dfft_rfft2d_batch: in and out overlap (the transform is out of place)'),
        ((A, A - 16, 64, 64, 2, 1, -1), -1, 'dfft_rfft2d_batch: in and out overlap (the transform is out of place)'),
        ((A, A, 64, 64, 2, 0, 1), -1, 'dfft_rfft2d_batch: in and out overlap (the transform is out of place)'),
        ((A, B, 0, 1 << 30, 1, 0, 1), -1, 'dfft_rfft2d_batch: bad arguments'),
        ((A, B, 1 << 30, 64, 1, 0, 0), -1, 'dfft_rfft2d_batch: bad arguments'),
        ((A, A + 16, 64, 1 << 30, 2, 0, 1), -6, 'dfft_rfft2d_batch: n2 = 1073741824 has no real form'),
    ],
    "dfft_r2r1d_strided": [
        ((None, B, 64, 4, 1, 0, 0), -1, 'dfft_r2r1d_strided: bad arguments'),
        ((A, None, 64, 4, 1, 0, 0), -1, 'dfft_r2r1d_strided: bad arguments'),
        ((A, B, 0, 4, 1, 0, 0), -1, 'dfft_r2r1d_strided: bad arguments'),
        ((A, B, 64, 0, 1, 0, 0), -1, 'dfft_r2r1d_strided: bad arguments'),
        ((A, B, 64, 4, 0, 0, 0), -1, 'dfft_r2r1d_strided: bad arguments'),
        ((A, B, 64, 4, 1, 2, 0), -1, 'dfft_r2r1d_strided: bad arguments'),
        ((A, B, 64, 4, 1, 0, -1), -1, 'dfft_r2r1d_strided: bad arguments'),
        ((A, B, 64, 4, 1, 0, 4), -1, 'dfft_r2r1d_strided: bad arguments'),
        ((A, B, 1 << 30, 4, 1, 0, 1), -1, 'dfft_r2r1d_strided: length 1073741824 is outside every form (at most 2^23, or a four-step length)'),
        ((A, A + 8, 64, 4, 4, 0, 2), -1, 'dfft_r2r1d_strided: in and out overlap partly (the transform runs out of place or exactly in place)'),
        ((A, A - 8, 64, 4, 4, 1, 3), -1, 'dfft_r2r1d_strided: in and out overlap partly (the transform runs out of place or exactly in place)'),
        ((A, B, 1 << 30, 4, 1, 0, 4), -1, 'dfft_r2r1d_strided: bad arguments'),
        ((A, A + 8, 1 << 30, 4, 4, 0, 0), -1, 'dfft_r2r1d_strided: length 1073741824 is outside every form (at most 2^23, or a four-step length)'),
        ((A, A, 4099, 1 << 32, 1, 0, 0), -6, 'dfft_r2r1d_strided (packed pairs): n = 4099, width = 2147483648: a column pass would span 2^32 or more 16-byte (fp32, odd width or unaligned: 8-byte) units, or width > 2^31 - 64'),
    ],
    "dfft_scale": [
        ((None, 8, 0, 2.0), -1, 'dfft_scale: bad arguments'),
        ((A, -1, 0, 2.0), -1, 'dfft_scale: bad arguments'),
        ((A, 8, 2, 2.0), -1, 'dfft_scale: bad arguments'),
        ((None, -1, 5, 2.0), -1, 'dfft_scale: bad arguments'),
    ],
}
# ---- TABLE END


@pytest.mark.parametrize("entry", sorted(CREATE_TABLE))
def test_create_refusals_are_byte_identical(entry):
    for kw, rc, msg in CREATE_TABLE[entry]:
        assert _create(entry, **kw) == (rc, msg), (entry, kw)


@pytest.mark.parametrize("entry", sorted(BATCH_TABLE))
def test_plan_less_refusals_are_byte_identical(entry):
    for args, rc, msg in BATCH_TABLE[entry]:
        assert _call(entry, args) == (rc, msg), (entry, args)


def test_the_tables_cover_every_entry_point_and_no_row_reaches_the_device_query():
    from distributedfft_amd import _lib as L
    assert sorted(CREATE_TABLE) == sorted(n for n in L.SIGNATURES if n.startswith("dfft_plan_create"))
    assert sorted(BATCH_TABLE) == ["dfft_fft1d_any", "dfft_fft1d_cols", "dfft_fft1d_rows", "dfft_fft2d_batch", "dfft_r2r1d_strided", "dfft_rfft1d",
                                   "dfft_rfft1d_strided", "dfft_rfft2d_batch", "dfft_scale"]
    for table in (CREATE_TABLE, BATCH_TABLE):
        for entry, rows in table.items():
            assert len(rows) >= 4, entry
            for _, rc, msg in rows:
                assert rc in (L.EINVAL, L.EUNSUPPORTED) and msg and "no HIP device" not in msg, (entry, rc, msg)
