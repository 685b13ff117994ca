"""Framed (Welch) 1-D real cross-spectrum (dfft_rcsd1d) against what a caller composes without it.  Per case (precision, rows, n, n_fft,
auto | cross; hop = n_fft / 2, periodic Hann window) one JSON line per variant:

  fused            dfft_rcsd1d as it is routed (its `route` field says which): the one-launch kernel (plus the slice reduction), or composed
  composed         dfft_rcsd1d under DFFT_RCSD_FUSED=0: the STFT frame kernel (or gather-and-window and R2C rows) on both fields into
                   chunked scratch, multiply-accumulate in frame order
  baseline_stft    the spectrogram route: api.stft(x, n_fft, hop, w, center=False, power=2).mean(-2) (auto),
                   (api.stft(x).conj() * api.stft(y)).mean(-2) (cross)
  baseline_unfold  api.rxspec1d on x.unfold(-1, n_fft, hop) * w made contiguous, frames as the batch
  read             a sum over every row of x (auto) or of x * y (cross): the floor of anything that reads the fields once

Timing: HIP events on the stream the work runs on, around `--inner` back-to-back calls; `--warmup` untimed rounds, `--reps` timed rounds
(>= 20) with the variants ALTERNATING inside every round, median and spread (p10 .. p90) of the per-call time.  TBps = fields * n * rows *
sizeof(real) / time: the model in which each row is read once and nothing else moves.

  python tools/rcsd_bench.py [--cases f64:4096:65536:1024:auto,...] [--reps 20] [--out results.jsonl] [--tag run1]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

DEFAULT_CASES = ",".join(f"{p}:4096:65536:{m}:{k}" for m in (256, 1024, 2048, 8192) for p in ("f64", "f32") for k in ("auto", "cross")) + "," + \
    ",".join(f"{p}:8:16777216:1024:{k}" for p in ("f64", "f32") for k in ("auto", "cross"))


def stats(ms):
    s = sorted(ms)
    return {"median_ms": round(statistics.median(s), 5), "p10_ms": round(s[len(s) // 10], 5), "p90_ms": round(s[(9 * len(s)) // 10], 5), "samples": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="f64|f32:rows:n:n_fft:auto|cross, comma-separated")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=2, help="calls per timed window")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    assert a.reps >= 20, "at least 20 timed rounds"
    import torch
    from distributedfft_amd import _lib as L
    from distributedfft_amd import api
    if not torch.cuda.is_available():
        sys.exit("rcsd_bench: no HIP device (nothing is measured on a CPU)")
    lib = L.load()
    dev = torch.device("cuda:0")
    out = open(a.out, "a") if a.out else None

    for case in a.cases.split(","):
        prec, rows, n, m, kind = case.split(":")
        rows, n, m = int(rows), int(n), int(m)
        hop, auto = m // 2, kind == "auto"
        rdt, cdt, code, rs = (torch.float64, torch.complex128, api.F64, 8) if prec == "f64" else (torch.float32, torch.complex64, api.F32, 4)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234)
        x = (torch.rand((rows, n), generator=gen, device=dev, dtype=torch.float32) - 0.5).to(rdt)
        y = x if auto else (torch.rand((rows, n), generator=gen, device=dev, dtype=torch.float32) - 0.5).to(rdt)
        w = torch.hann_window(m, periodic=True, dtype=rdt, device=dev)
        frames = api.stft_frames(n, m, hop, 0)
        nb = m // 2 + 1
        s_f = torch.empty((rows, nb), dtype=cdt, device=dev)
        s_c = torch.empty_like(s_f)
        vp = C.c_void_p
        keep = {}

        def rcsd(dst):
            L.check(lib.dfft_rcsd1d(vp(x.data_ptr()), vp(y.data_ptr()), vp(dst.data_ptr()), vp(w.data_ptr()), n, m, hop, frames, rows, 1.0 / frames, code,
                                    None), "dfft_rcsd1d")

        def fused():
            rcsd(s_f)

        def composed():
            os.environ["DFFT_RCSD_FUSED"] = "0"
            try:
                rcsd(s_c)
            finally:
                os.environ.pop("DFFT_RCSD_FUSED", None)

        def baseline_stft():
            if auto:
                keep["stft"] = api.stft(x, m, hop, w, center=False, power=2, frames_last=False).mean(-2)
            else:
                keep["stft"] = (api.stft(x, m, hop, w, center=False, frames_last=False).conj() * api.stft(y, m, hop, w, center=False, frames_last=False)).mean(-2)

        def baseline_unfold():
            xf = (x.unfold(-1, m, hop) * w).transpose(0, 1).contiguous()      # (frames, rows, m): frames as the batch of rxspec1d
            yf = xf if auto else (y.unfold(-1, m, hop) * w).transpose(0, 1).contiguous()
            keep["unfold"] = api.rxspec1d(xf, yf, m)

        def read():
            keep["read"] = (x if auto else x * y).sum(-1)

        variants = [("fused", fused), ("composed", composed), ("baseline_stft", baseline_stft), ("baseline_unfold", baseline_unfold), ("read", read)]
        is_fused = lib.dfft_rcsd1d_fused_applies(m, code, int(auto)) == 1
        # the routes agree before anything is timed
        for _, fn in variants:
            fn()
        torch.cuda.synchronize()
        scale = float(keep["stft"].abs().max())
        devs = {"stft": float((s_f - keep["stft"]).abs().max()) / scale, "unfold": float((s_f - keep["unfold"] / frames).abs().max()) / scale,
                "composed": float((s_f - s_c).abs().max()) / scale}
        assert max(devs.values()) < (1e-11 if prec == "f64" else 2e-3), (case, devs)
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
        med = {name: statistics.median(v) for name, v in times.items()}
        moved = (1 if auto else 2) * n * rows * rs
        for name, _ in variants:
            rec = {"case": case, "prec": prec, "rows": rows, "n": n, "n_fft": m, "hop": hop, "frames": frames, "kind": kind, "variant": name,
                   "inner": a.inner, **stats(times[name]), "TBps": round(moved / (med[name] * 1e-3) / 1e12, 3), "tag": a.tag}
            if name == "fused":
                rec.update(route="fused" if is_fused else "composed", slices=int(lib.dfft_rcsd1d_slices(m, rows, frames, code)),
                           of_read=round(med["read"] / med["fused"], 3), speedup_over_stft=round(med["baseline_stft"] / med["fused"], 2),
                           speedup_over_unfold=round(med["baseline_unfold"] / med["fused"], 2), speedup_over_composed=round(med["composed"] / med["fused"], 2),
                           max_rel_dev=devs)
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        keep.clear()
        del x, y, s_f, s_c
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
