"""One sha256 over the answers of every query-only entry point of the fused 1-D real kernel families (scratch sizes, fused-route
predicates, slice counts, length and block choosers), over tuned and untuned lengths, both precisions, both filter kinds, auto / cross,
row counts on both sides of the 256 MiB chunk cap, both values of each *_FUSED switch and the two chunk overrides; and the scratch and
route queries of the any-length, strided real and real-to-real transforms, which take the same chunk arithmetic and switches.  Host arithmetic
only: no device is needed.  Run it on two builds (DFFT_LIB=<path to libdfft_mi355x_pt.so>) to show that a refactor of the host
scaffold answers the same.

  DFFT_LIB=/path/to/lib.so python tools/fused_host_digest.py"""
import ctypes
import hashlib
import itertools
import os
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from distributedfft_amd import _lib  # noqa: E402

SWITCHES = ("DFFT_RCONV_FUSED", "DFFT_RCONV_LONG_FUSED", "DFFT_RXSPEC_FUSED", "DFFT_RXSPEC_LONG_FUSED", "DFFT_STFT_FUSED", "DFFT_RCSD_FUSED")
CHUNKS = ("DFFT_STFT_CHUNK_BYTES", "DFFT_RCSD_CHUNK_BYTES")
COUNTS = (1, 3, 64, 4097)


def tuned_lengths():
    text = (ROOT / "distributedfft_amd" / "csrc" / "dfft_plans.h").read_text()
    return sorted({int(n) for n in re.findall(r"^\s*X\((\d+),", text, re.M)})


def main():
    lib = _lib.load()
    h = hashlib.sha256()
    answers = 0

    def put(*values):
        nonlocal answers
        answers += 1
        h.update((" ".join(str(int(v)) for v in values) + "\n").encode())

    # every tuned half-length and three untuned accepted ones (run-time-scheduled lengths: the default branches of the dispatch)
    tuned, untuned = tuned_lengths(), [18, 36, 72]
    for M in untuned:
        assert M not in tuned and lib.dfft_rconv1d_length(2 * M) == 2 * M, (M, "must be accepted and have no tuned plan")
        assert not lib.dfft_rconv1d_fused_applies(2 * M, 2 * M, 0, 0, 1), (M, "must run the composed route")
    halves = [M for M in tuned if lib.dfft_rconv1d_length(2 * M) == 2 * M] + untuned
    longs = sorted({lib.dfft_rconv1d_long_length(x) for x in (8193, 20000, 98304, 100000, 1 << 20, 3 * (1 << 20), 1 << 23)} - {0})
    for env in itertools.product(("1", "0"), repeat=len(SWITCHES)):
        if env.count("0") > 1:   # each switch off on its own, and all on
            continue
        for chunk in (None, "65536", "3000000"):
            for k, v in zip(SWITCHES, env):
                os.environ[k] = v
            for k in CHUNKS:
                os.environ.pop(k, None)
                if chunk:
                    os.environ[k] = chunk
            put(*(int(v) for v in env), int(chunk or 0))
            for dtype in (0, 1):
                for M in halves:
                    m = 2 * M
                    put(lib.dfft_rconv1d_length(m - 1), lib.dfft_rconv1d_os_fused_applies(m, dtype), lib.dfft_stft1d_fused_applies(m, dtype))
                    for fk, vec in itertools.product((0, 1), (0, 1)):
                        put(lib.dfft_rconv1d_fused_applies(m - 1 - vec, m, dtype, fk, vec))
                    for vec in (0, 1):
                        put(lib.dfft_rxspec1d_fused_applies(m - 1 - vec, m, dtype, vec))
                    for autos in (0, 1):
                        put(lib.dfft_rcsd1d_fused_applies(m, dtype, autos))
                    # rows / channels / batch from COUNTS, and a row count on the far side of the 256 MiB cap
                    big = (300 << 20) // (m * 4) + 1
                    for ch, b in itertools.product(COUNTS, COUNTS + (big,)):
                        put(lib.dfft_rconv1d_scratch_bytes(m - 1, m, ch, b, dtype), lib.dfft_rxspec1d_scratch_bytes(m - 1, m, ch, b, dtype),
                            lib.dfft_rxspec1d_slices(m, ch, b, dtype), lib.dfft_rconv1d_os_scratch_bytes(5 * m + 3, m, (m // 4) & ~1, ch, b, dtype),
                            lib.dfft_rcsd1d_slices(m, ch, b, dtype))
                        for kind in (0, 1):   # out_kind of the STFT, autos of the cross-spectral density
                            put(lib.dfft_stft1d_scratch_bytes(m, b, ch, dtype, kind), lib.dfft_rcsd1d_scratch_bytes(m, b, ch, dtype, kind))
                        put(lib.dfft_istft1d_scratch_bytes(m, b, ch, dtype))
                for m in longs:
                    put(m, lib.dfft_rconv1d_long_fused_applies(m, dtype), lib.dfft_rxspec1d_long_fused_applies(m, dtype))
                    for ch, b in itertools.product(COUNTS, COUNTS):
                        put(lib.dfft_rconv1d_long_scratch_bytes(m - 1, m, ch, b, dtype), lib.dfft_rxspec1d_long_scratch_bytes(m - 1, m, ch, b, dtype),
                            lib.dfft_rxspec1d_long_slices(m, ch, b, dtype))
                for taps, n_out in itertools.product((1, 2, 17, 256, 1000, 4097, 8191), (1, 100, 65536, 1 << 22)):
                    mm, dd = ctypes.c_longlong(0), ctypes.c_longlong(0)
                    ok = lib.dfft_rconv1d_os_block(taps, n_out, dtype, ctypes.byref(mm), ctypes.byref(dd))
                    put(ok, mm.value, dd.value)
    # the older families that take the scaffold's chunk arithmetic and switches: any-length, strided real and real-to-real transforms
    for r2r_on, bs_on in itertools.product(("1", "0"), repeat=2):
        os.environ["DFFT_R2R_FUSED"], os.environ["DFFT_BLUESTEIN_FUSED"] = r2r_on, bs_on
        for dtype, n, s in itertools.product((0, 1), (18, 97, 243, 512, 2053, 4096, 6000), (1, 3, 64)):
            for b in COUNTS + ((300 << 20) // (n * s * 8) + 1,):
                put(lib.dfft_fft1d_any_scratch_bytes(n, s, b, dtype), lib.dfft_rfft1d_strided_scratch_bytes(n, s, b, dtype),
                    lib.dfft_bluestein_fused_applies(n, s), lib.dfft_rfft_cols_fused_applies(n, s, dtype))
                for kind, vec in itertools.product((0, 1, 2, 3), (0, 1)):
                    put(lib.dfft_r2r1d_strided_scratch_bytes(n, s, b, dtype, kind, vec), lib.dfft_r2r_fused_applies(n, s, dtype, kind, vec))
    for x in (1, 2, 3, 100, 1000, 4097, 8191, 8192, 8193, 1 << 16, 1 << 22, (1 << 23) + 1):
        put(lib.dfft_rconv1d_length(x), lib.dfft_rconv1d_long_length(x))
    print(f"{answers} answers sha256 {h.hexdigest()}")


if __name__ == "__main__":
    main()
