"""Overlap-save 1-D real FFT convolution (dfft_rconv1d_os) against what a caller composes without it.  Per case (precision, n, taps,
rows on 16 channels; the block (m, discard) from dfft_rconv1d_os_block unless --m is given; n_out = n) four variants, one JSON line each:

  fused      dfft_rconv1d_os, the one-launch block kernel
  composed   dfft_rconv1d_os under DFFT_RCONV_FUSED=0: gather kernel, R2C rows, multiply, C2R rows, scatter kernel on the library's scratch
  baseline   what a caller writes without the entry point: torch zero-pad, unfold(...) into overlapping blocks made contiguous,
             dfft_rconv1d with n = m in place on the blocks, slice-copies of the valid parts into the result
  copy       a plain device copy of n * rows reals (2 * n * rows reals moved): the floor of anything that reads and writes the rows

With --blocks the tool measures the chooser's per-block table instead: for every power-of-two m from 256 to 8192 the fused route on
1024 rows of 131072 samples with discard = m / 4, reported as nanoseconds per block (time / (rows * blocks per row)).

Timing: HIP events on the stream the work runs on, around `--inner` back-to-back calls without host synchronisation; `--warmup` untimed
rounds, `--reps` timed rounds (>= 20) with the variants ALTERNATING inside every round, median and spread (p10 .. p90) of the per-call
time.  fused_TBps = 2 * n * rows * sizeof(real) / time; fused_of_copy = copy time / fused time.

  python tools/osconv_bench.py [--cases f64:65536:257:4096,...] [--blocks] [--reps 20] [--out results.jsonl] [--tag run1]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

DEFAULT_CASES = ("f64:65536:257:4096,f32:65536:257:4096,f64:65536:1025:4096,f32:65536:1025:4096,"
                 "f64:1048576:1025:256,f32:1048576:1025:256")
CHANNELS = 16
BLOCK_ROWS, BLOCK_N = 1024, 131072


def stats(ms):
    s = sorted(ms)
    return {"median_ms": round(statistics.median(s), 5), "p10_ms": round(s[len(s) // 10], 5), "p90_ms": round(s[(9 * len(s)) // 10], 5), "samples": len(s)}


def timed_rounds(torch, variants, warmup, reps, inner):
    st = torch.cuda.current_stream()
    times = {name: [] for name, _ in variants}
    for r in range(warmup + reps):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(inner):
                fn()
            e1.record(st)
            e1.synchronize()
            if r >= warmup:
                times[name].append(e0.elapsed_time(e1) / inner)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="f64|f32:n:taps:rows, comma-separated")
    ap.add_argument("--m", type=int, default=0, help="block length (default: the chooser's)")
    ap.add_argument("--blocks", action="store_true", help="measure the per-block table t(m) instead")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=3, help="calls per timed window")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    assert a.reps >= 20, "at least 20 timed rounds"
    import torch
    from distributedfft_amd import _lib as L
    from distributedfft_amd import api
    if not torch.cuda.is_available():
        sys.exit("osconv_bench: no HIP device (nothing is measured on a CPU)")
    lib = L.load()
    dev = torch.device("cuda:0")
    out = open(a.out, "a") if a.out else None
    vp = C.c_void_p

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def types(prec):
        return (torch.float64, torch.complex128, api.F64, 8) if prec == "f64" else (torch.float32, torch.complex64, api.F32, 4)

    def inputs(prec, rows, n, m):
        rdt, cdt, _, _ = types(prec)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234)
        x = (torch.rand((rows // CHANNELS, CHANNELS, n), generator=gen, device=dev, dtype=torch.float32) - 0.5).to(rdt)
        H = torch.complex(torch.rand((CHANNELS, m // 2 + 1), generator=gen, device=dev, dtype=torch.float32) + 0.5,
                          torch.rand((CHANNELS, m // 2 + 1), generator=gen, device=dev, dtype=torch.float32) - 0.5).to(cdt)
        return x, H

    if a.blocks:
        for prec in ("f64", "f32"):
            _, _, code, rs = types(prec)
            runs = []
            for m in (256, 512, 1024, 2048, 4096, 8192):
                d = m // 4
                x, H = inputs(prec, BLOCK_ROWS, BLOCK_N, m)
                y = torch.empty_like(x)
                assert lib.dfft_rconv1d_os_fused_applies(m, code) == 1, m

                def fused(x=x, y=y, H=H, m=m, d=d):
                    L.check(lib.dfft_rconv1d_os(vp(x.data_ptr()), vp(y.data_ptr()), vp(H.data_ptr()), BLOCK_N, BLOCK_N, m, d, CHANNELS, BLOCK_ROWS // CHANNELS,
                                                code, api.FILTER_COMPLEX, None), "dfft_rconv1d_os")
                runs.append((m, d, fused, (x, y, H)))
            x0, y0 = runs[0][3][0], runs[0][3][1]
            variants = [(f"m{m}", fn) for m, _, fn, _ in runs] + [("copy", lambda: y0.copy_(x0))]
            times = timed_rounds(torch, variants, a.warmup, a.reps, a.inner)
            for m, d, _, _ in runs:
                items = BLOCK_ROWS * -(-BLOCK_N // (m - d))
                t = times[f"m{m}"]
                emit({"table": "t(m)", "prec": prec, "m": m, "discard": d, "rows": BLOCK_ROWS, "n": BLOCK_N, "items": items, "inner": a.inner, **stats(t),
                      "ns_per_block": round(statistics.median(t) * 1e6 / items, 3), "fused_TBps": round(2 * BLOCK_N * BLOCK_ROWS * rs / (statistics.median(t) * 1e-3) / 1e12, 3),
                      "tag": a.tag})
            emit({"table": "t(m)", "prec": prec, "variant": "copy", **stats(times["copy"]),
                  "copy_TBps": round(2 * BLOCK_N * BLOCK_ROWS * rs / (statistics.median(times["copy"]) * 1e-3) / 1e12, 3), "tag": a.tag})
            del runs, variants, x0, y0
            torch.cuda.empty_cache()
        return

    for case in a.cases.split(","):
        prec, n, taps, rows = case.split(":")
        n, taps, rows = int(n), int(taps), int(rows)
        rdt, cdt, code, rs = types(prec)
        batch = rows // CHANNELS
        if a.m:
            m, d = a.m, taps - 1 + ((taps - 1) & 1)
        else:
            m, d = api.rconv1d_os_block(taps, n, code)
        S = m - d
        nb = -(-n // S)
        x, H = inputs(prec, rows, n, m)
        y = torch.empty_like(x)
        yb = torch.empty_like(x)

        def os_call(dst):
            L.check(lib.dfft_rconv1d_os(vp(x.data_ptr()), vp(dst.data_ptr()), vp(H.data_ptr()), n, n, m, d, CHANNELS, batch, code, api.FILTER_COMPLEX, None),
                    "dfft_rconv1d_os")

        def fused():
            os_call(y)

        def composed():
            os.environ["DFFT_RCONV_FUSED"] = "0"
            try:
                os_call(yb)
            finally:
                os.environ.pop("DFFT_RCONV_FUSED", None)

        nf = n // S  # whole blocks of results

        def baseline():
            xp = torch.nn.functional.pad(x, (d, nb * S - n))                      # [batch][channels][(nb - 1) S + m]
            blocks = xp.unfold(-1, m, S).permute(0, 2, 1, 3).contiguous()         # [batch][nb][channels][m]: rows r use filter r % channels
            L.check(lib.dfft_rconv1d(vp(blocks.data_ptr()), vp(blocks.data_ptr()), vp(H.data_ptr()), m, m, CHANNELS, batch * nb, code, api.FILTER_COMPLEX, None),
                    "dfft_rconv1d")
            valid = blocks[..., d:].permute(0, 2, 1, 3)                           # [batch][channels][nb][S]
            if nf:
                yb[..., :nf * S].unflatten(-1, (nf, S)).copy_(valid[:, :, :nf])
            if nf < nb:
                yb[..., nf * S:].copy_(valid[:, :, nf, :n - nf * S])

        def copy():
            yb.copy_(x)

        variants = [("fused", fused), ("composed", composed), ("baseline", baseline), ("copy", copy)]
        assert lib.dfft_rconv1d_os_fused_applies(m, code) == 1, f"{case}: m = {m} is not a fused length"
        # the three routes agree before anything is timed
        fused()
        baseline()
        torch.cuda.synchronize()
        dev_base = float((y - yb).abs().max() / yb.abs().max())
        composed()
        torch.cuda.synchronize()
        dev_comp = float((y - yb).abs().max() / yb.abs().max())
        assert max(dev_base, dev_comp) < (1e-12 if prec == "f64" else 1e-4), (case, dev_base, dev_comp)
        times = timed_rounds(torch, variants, a.warmup, a.reps, a.inner)
        med = {k: statistics.median(v) for k, v in times.items()}
        moved = 2 * n * rows * rs
        for name, _ in variants:
            rec = {"case": case, "prec": prec, "n": n, "taps": taps, "m": m, "discard": d, "blocks_per_row": nb, "rows": rows, "channels": CHANNELS,
                   "variant": name, "inner": a.inner, **stats(times[name]), "tag": a.tag}
            if name == "fused":
                rec.update(fused_TBps=round(moved / (med["fused"] * 1e-3) / 1e12, 3), fused_of_copy=round(med["copy"] / med["fused"], 3),
                           speedup_over_baseline=round(med["baseline"] / med["fused"], 2), speedup_over_composed=round(med["composed"] / med["fused"], 2),
                           ns_per_block=round(med["fused"] * 1e6 / (rows * nb), 3), max_rel_dev_from_baseline=dev_base, max_rel_dev_from_composed=dev_comp)
            if name == "copy":
                rec.update(copy_TBps=round(moved / (med["copy"] * 1e-3) / 1e12, 3))
            emit(rec)
        del x, H, y, yb
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
