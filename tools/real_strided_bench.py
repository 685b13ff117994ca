"""Real transforms along a strided axis against the same data widened to complex: dfft_rfft1d_strided (forward and backward) next to
dfft_fft1d_any on the complex copy [batch][n][s], and dfft_rfft2d_batch next to dfft_fft2d_batch on the widened planes.  About 256 MiB of
reals per case; the two variants alternate call by call, and each reports the median of `--reps` device-event timings.

  python tools/real_strided_bench.py [--reps 30] [--out results.jsonl]          one JSON line per case, ratio = real / complex"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

NS = [256, 512, 768, 1024, 2048, 125, 243]
# tuned lengths whose fused tiles have the narrowest row segments (32 bytes and less in fp32 or fp64)
NS_NARROW = [1000, 1280, 1536, 2187, 2401, 3125, 4096]
SS = [512, 1000]
PLANES = [(256, 256), (512, 512), (768, 512), (1024, 1024)]
TARGET = 256 << 20


def timed(torch, fns, reps):
    """Median milliseconds of each fn, the fns alternating call by call."""
    times = [[] for _ in fns]
    for f in fns:  # warm-up: tables, scratch, occupancy queries
        f()
    torch.cuda.synchronize()
    for _ in range(reps):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b))
    return [statistics.median(t) for t in times]


def check(lib, rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: {rc} {lib.dfft_last_error().decode()}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--prec", default="f64,f32")
    ap.add_argument("--ns", default=None, help="comma-separated lengths of the strided cases (default: all)")
    ap.add_argument("--no-2d", action="store_true")
    a = ap.parse_args()
    import torch
    from distributedfft_amd import _lib as L
    lib = L.load()
    dev = torch.device("cuda:0")
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for prec in a.prec.split(","):
        rdt, cdt, code = (torch.float64, torch.complex128, L.F64) if prec == "f64" else (torch.float32, torch.complex64, L.F32)
        rs = 8 if prec == "f64" else 4
        for s in SS:
            for n in ([int(v) for v in a.ns.split(",")] if a.ns else NS + NS_NARROW):
                batch = max(1, TARGET // (n * s * rs))
                nh = n // 2 + 1
                x = torch.randn((batch, n, s), dtype=rdt, device=dev)
                X = torch.empty((batch, nh, s), dtype=cdt, device=dev)
                y = torch.empty_like(x)
                xc = x.to(cdt)
                Xc = torch.empty_like(xc)
                P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
                fr = lambda: check(lib, lib.dfft_rfft1d_strided(P(x), P(X), n, s, batch, code, 1, None), "r2c")  # noqa: E731
                br = lambda: check(lib, lib.dfft_rfft1d_strided(P(X), P(y), n, s, batch, code, -1, None), "c2r")  # noqa: E731
                fc = lambda: check(lib, lib.dfft_fft1d_any(P(xc), P(Xc), n, s, batch, code, 1, None), "c2c fwd")  # noqa: E731
                bc = lambda: check(lib, lib.dfft_fft1d_any(P(Xc), P(xc), n, s, batch, code, -1, None), "c2c bwd")  # noqa: E731
                t_fr, t_fc = timed(torch, [fr, fc], a.reps)
                t_br, t_bc = timed(torch, [br, bc], a.reps)
                for d, tr, tc in (("forward", t_fr, t_fc), ("backward", t_br, t_bc)):
                    emit({"case": "strided", "prec": prec, "n": n, "s": s, "batch": batch, "dir": d, "real_ms": round(tr, 4),
                          "complex_ms": round(tc, 4), "ratio": round(tr / tc, 3),
                          "real_gbs": round(batch * s * (n * rs + nh * 2 * rs) / tr / 1e6, 1)})
                del x, X, y, xc, Xc
                torch.cuda.empty_cache()
        for n1, n2 in ([] if a.no_2d else PLANES):
            batch = max(1, TARGET // (n1 * n2 * rs))
            nh = n2 // 2 + 1
            x = torch.randn((batch, n1, n2), dtype=rdt, device=dev)
            X = torch.empty((batch, n1, nh), dtype=cdt, device=dev)
            xc = x.to(cdt)
            Xc = torch.empty_like(xc)
            P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
            fr = lambda: check(lib, lib.dfft_rfft2d_batch(P(x), P(X), n1, n2, batch, code, 1, None), "rfft2d")  # noqa: E731
            fc = lambda: check(lib, lib.dfft_fft2d_batch(P(xc), P(Xc), n1, n2, batch, code, 1, None), "fft2d")  # noqa: E731
            t_fr, t_fc = timed(torch, [fr, fc], a.reps)
            emit({"case": "2d", "prec": prec, "n1": n1, "n2": n2, "batch": batch, "dir": "forward", "real_ms": round(t_fr, 4),
                  "complex_ms": round(t_fc, 4), "ratio": round(t_fr / t_fc, 3)})
            del x, X, xc, Xc
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
