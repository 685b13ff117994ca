"""Long 1-D real FFT convolution (dfft_rconv1d_long) against what a caller composes without it.  Per case (precision, m, n, rows; 16
channels) four variants, one JSON line each:

  fused      dfft_rconv1d_long, the three-launch pipeline
  composed   dfft_rconv1d_long under DFFT_RCONV_LONG_FUSED=0: pad kernel, real rows of length m, multiply, inverse rows, truncate kernel
             on the library's scratch
  baseline   the calls that exist without the entry point: torch zero-pad, dfft_rfft1d forward, torch multiply (1 / m folded into H, so
             the separate divide is not charged), dfft_rfft1d backward, slice-copy into the result
  copy       a plain device copy of n * rows reals (2 * n * rows reals moved): the floor of anything that reads and writes the rows

Timing: HIP events on the stream the work runs on, around `--inner` back-to-back calls without host synchronisation; `--warmup` untimed
rounds, `--reps` timed rounds (>= 20) with the four variants ALTERNATING inside every round, median and spread (p10 .. p90) of the
per-call time.  fused_TBps = 2 * n * rows * sizeof(real) / time; fused_of_copy = copy time / fused time.

  python tools/lconv_bench.py [--cases f64:65536:32768:1024,...] [--reps 20] [--out results.jsonl] [--tag run1]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

DEFAULT_CASES = ("f64:65536:32768:1024,f32:65536:32768:1024,f64:2097152:1048576:64,f32:2097152:1048576:64,"
                 "f64:16384:16384:4096,f32:16384:16384:4096")
CHANNELS = 16


def stats(ms):
    s = sorted(ms)
    return {"median_ms": round(statistics.median(s), 5), "p10_ms": round(s[len(s) // 10], 5), "p90_ms": round(s[(9 * len(s)) // 10], 5), "samples": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="f64|f32:m:n:rows, comma-separated (rows a multiple of 16)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=3, help="calls per timed window")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    assert a.reps >= 20, "at least 20 timed rounds"
    import torch
    from distributedfft_amd import _lib as L
    from distributedfft_amd import api
    if not torch.cuda.is_available():
        sys.exit("lconv_bench: no HIP device (nothing is measured on a CPU)")
    lib = L.load()
    dev = torch.device("cuda:0")
    out = open(a.out, "a") if a.out else None

    for case in a.cases.split(","):
        prec, m, n, rows = case.split(":")
        m, n, rows = int(m), int(n), int(rows)
        assert rows % CHANNELS == 0
        batch = rows // CHANNELS
        rdt, cdt, code, rs = (torch.float64, torch.complex128, api.F64, 8) if prec == "f64" else (torch.float32, torch.complex64, api.F32, 4)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234)
        x = (torch.rand((batch, CHANNELS, n), generator=gen, device=dev, dtype=torch.float32) - 0.5).to(rdt)
        H = torch.complex(torch.rand((CHANNELS, m // 2 + 1), generator=gen, device=dev, dtype=torch.float32) + 0.5,
                          torch.rand((CHANNELS, m // 2 + 1), generator=gen, device=dev, dtype=torch.float32) - 0.5).to(cdt)
        Hp = api.rconv1d_long_filter(H)
        Hs = (H / m).contiguous()
        y = torch.empty_like(x)
        yb = torch.empty_like(x)
        bins = torch.empty((batch, CHANNELS, m // 2 + 1), dtype=cdt, device=dev)
        full = torch.empty((batch, CHANNELS, m), dtype=rdt, device=dev)
        vp = C.c_void_p
        n1, n2 = C.c_int(0), C.c_int(0)
        assert lib.dfft_rconv1d_long_split(m, C.byref(n1), C.byref(n2)) == 1, f"{case}: m is not accepted"

        def lconv(dst):
            L.check(lib.dfft_rconv1d_long(vp(x.data_ptr()), vp(dst.data_ptr()), vp(Hp.data_ptr()), n, m, CHANNELS, batch, code, api.FILTER_COMPLEX, None),
                    "dfft_rconv1d_long")

        def fused():
            lconv(y)

        def composed():
            os.environ["DFFT_RCONV_LONG_FUSED"] = "0"
            try:
                lconv(yb)
            finally:
                os.environ.pop("DFFT_RCONV_LONG_FUSED", None)

        def baseline():
            xp = torch.nn.functional.pad(x, (0, m - n)) if m > n else x
            L.check(lib.dfft_rfft1d(vp(xp.data_ptr()), vp(bins.data_ptr()), m, rows, code, api.FORWARD, None), "dfft_rfft1d")
            torch.mul(bins, Hs, out=bins)
            L.check(lib.dfft_rfft1d(vp(bins.data_ptr()), vp(full.data_ptr()), m, rows, code, api.BACKWARD, None), "dfft_rfft1d")
            yb.copy_(full[..., :n])

        def copy():
            yb.copy_(x)

        variants = [("fused", fused), ("composed", composed), ("baseline", baseline), ("copy", copy)]
        assert lib.dfft_rconv1d_long_fused_applies(m, code) == 1, f"{case}: not a fused length"
        # the three routes agree before anything is timed
        fused()
        baseline()
        torch.cuda.synchronize()
        dev_base = float((y - yb).abs().max() / yb.abs().max())
        composed()
        torch.cuda.synchronize()
        dev_comp = float((y - yb).abs().max() / yb.abs().max())
        assert max(dev_base, dev_comp) < (1e-11 if prec == "f64" else 5e-4), (case, dev_base, dev_comp)
        st = torch.cuda.current_stream()
        times = {name: [] for name, _ in variants}
        for r in range(a.warmup + a.reps):
            for name, fn in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(a.inner):
                    fn()
                e1.record(st)
                e1.synchronize()
                if r >= a.warmup:
                    times[name].append(e0.elapsed_time(e1) / a.inner)
        med = {k: statistics.median(v) for k, v in times.items()}
        moved = 2 * n * rows * rs
        for name, _ in variants:
            rec = {"case": case, "prec": prec, "m": m, "n": n, "n1": n1.value, "n2": n2.value, "rows": rows, "channels": CHANNELS, "variant": name,
                   "inner": a.inner, **stats(times[name]), "tag": a.tag}
            if name == "fused":
                rec.update(fused_TBps=round(moved / (med["fused"] * 1e-3) / 1e12, 3), fused_of_copy=round(med["copy"] / med["fused"], 3),
                           speedup_over_baseline=round(med["baseline"] / med["fused"], 2), speedup_over_composed=round(med["composed"] / med["fused"], 2),
                           max_rel_dev_from_baseline=dev_base, max_rel_dev_from_composed=dev_comp)
            if name == "copy":
                rec.update(copy_TBps=round(moved / (med["copy"] * 1e-3) / 1e12, 3))
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        del x, H, Hp, Hs, y, yb, bins, full
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
