"""Batched short-time Fourier transform (dfft_stft1d / dfft_istft1d) against what a caller composes without it and against torch.
Per case (precision, rows, n, m; hop = m / 4, pad = m / 2 mirrored, a Hann window) the variants, one JSON line each:

  fused        dfft_stft1d, the one-launch frame kernel, complex bins
  fused_power  the same with the power spectrogram as output (half the bytes)
  composed     dfft_stft1d under DFFT_STFT_FUSED=0: gather-and-window kernel, R2C rows on the library's scratch
  baseline     what a caller wrote before: torch reflect-pad, unfold(-1, m, hop) * window made contiguous, dfft_rfft1d on the frames
  torch        torch.stft on the device
  istft        dfft_istft1d on the bins (the envelope built once, outside the timing)
  torch_istft  torch.istft on the same bins
  copy         a plain device copy of the output bytes (read + write): the floor of anything that writes that much

Timing: HIP events on the stream the work runs on, around `--inner` back-to-back calls without host synchronisation; `--warmup` untimed
rounds, `--reps` timed rounds (>= 20) with the variants ALTERNATING inside every round, median and spread (p10 .. p90) of the per-call
time.  TBps counts the input once and the output once.

  python tools/stft_bench.py [--cases f64:4096:65536:256,...] [--reps 20] [--out results.jsonl] [--tag run1]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

DEFAULT_CASES = ",".join(f"{p}:4096:65536:{m}" for p in ("f64", "f32") for m in (256, 512, 1024, 2048)) + ",f32:64:4194304:1024"


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
    ap.add_argument("--cases", default=DEFAULT_CASES, help="f64|f32:rows:n:m, comma-separated")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=2, help="calls per timed window")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    assert a.reps >= 20, "at least 20 timed rounds"
    import torch
    from distributedfft_amd import _lib as L
    from distributedfft_amd import api
    if not torch.cuda.is_available():
        sys.exit("stft_bench: no HIP device (nothing is measured on a CPU)")
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

    for case in a.cases.split(","):
        prec, rows, n, m = case.split(":")
        rows, n, m = int(rows), int(n), int(m)
        rdt, cdt, code, rs = (torch.float64, torch.complex128, api.F64, 8) if prec == "f64" else (torch.float32, torch.complex64, api.F32, 4)
        hop, pad, bins = m // 4, m // 2, m // 2 + 1
        frames = api.stft_frames(n, m, hop, pad)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234)
        x = (torch.rand((rows, n), generator=gen, device=dev, dtype=torch.float32) - 0.5).to(rdt)
        w = torch.hann_window(m, dtype=rdt, device=dev)
        X = torch.empty((rows, frames, bins), dtype=cdt, device=dev)
        Xb = torch.empty_like(X)
        P = torch.empty((rows, frames, bins), dtype=rdt, device=dev)
        y = torch.empty((rows, n), dtype=rdt, device=dev)
        inv_env = (1.0 / api.istft_envelope(w, m, hop, frames)[pad:pad + n]).to(rdt).contiguous()

        def fwd(dst, kind):
            L.check(lib.dfft_stft1d(vp(x.data_ptr()), vp(dst.data_ptr()), vp(w.data_ptr()), n, m, hop, pad, frames, rows, code, api.STFT_PAD_REFLECT, kind, 1.0,
                                    None), "dfft_stft1d")

        def fused():
            fwd(X, api.STFT_OUT_COMPLEX)

        def fused_power():
            fwd(P, api.STFT_OUT_POWER)

        def composed():
            os.environ["DFFT_STFT_FUSED"] = "0"
            try:
                fwd(Xb, api.STFT_OUT_COMPLEX)
            finally:
                os.environ.pop("DFFT_STFT_FUSED", None)

        def baseline():
            xp = torch.nn.functional.pad(x[None], (pad, pad), mode="reflect")[0]
            fr = (xp.unfold(-1, m, hop)[:, :frames] * w).contiguous()
            L.check(lib.dfft_rfft1d(vp(fr.data_ptr()), vp(Xb.data_ptr()), m, rows * frames, code, api.FORWARD, None), "dfft_rfft1d")

        def torch_stft():
            return torch.stft(x, m, hop, window=w, center=True, pad_mode="reflect", onesided=True, return_complex=True)

        def inverse():
            L.check(lib.dfft_istft1d(vp(X.data_ptr()), vp(y.data_ptr()), vp(w.data_ptr()), vp(inv_env.data_ptr()), n, m, hop, pad, frames, rows, code, None),
                    "dfft_istft1d")

        Xt = X.transpose(1, 2)

        def torch_istft():
            return torch.istft(Xt, m, hop, window=w, center=True, length=n)

        def copy():
            Xb.copy_(X)

        assert lib.dfft_stft1d_fused_applies(m, code) == 1, f"{case}: m = {m} is not a fused length"
        # the routes agree before anything is timed
        fused()
        baseline()
        torch.cuda.synchronize()
        scale = float(torch.view_as_real(Xb).abs().max())
        dev_base = float(torch.view_as_real(X - Xb).abs().max()) / scale
        composed()
        torch.cuda.synchronize()
        dev_comp = float(torch.view_as_real(X - Xb).abs().max()) / scale
        dev_torch = float(torch.view_as_real(X - torch_stft().transpose(1, 2)).abs().max()) / scale
        inverse()
        torch.cuda.synchronize()
        dev_inv = float((y - x).abs().max())
        dev_tinv = float((y - torch_istft()).abs().max())
        tol = 1e-12 if prec == "f64" else 1e-4
        assert max(dev_base, dev_comp, dev_torch, dev_inv, dev_tinv) < tol, (case, dev_base, dev_comp, dev_torch, dev_inv, dev_tinv)
        variants = [("fused", fused), ("fused_power", fused_power), ("composed", composed), ("baseline", baseline), ("torch", torch_stft), ("istft", inverse),
                    ("torch_istft", torch_istft), ("copy", copy)]
        times = timed_rounds(torch, variants, a.warmup, a.reps, a.inner)
        med = {k: statistics.median(v) for k, v in times.items()}
        in_b, out_b = rows * n * rs, rows * frames * bins * 2 * rs
        moved = {"fused": in_b + out_b, "fused_power": in_b + out_b // 2, "composed": in_b + out_b, "baseline": in_b + out_b, "torch": in_b + out_b,
                 "istft": in_b + out_b, "torch_istft": in_b + out_b, "copy": 2 * out_b}
        for name, _ in variants:
            rec = {"case": case, "prec": prec, "rows": rows, "n": n, "m": m, "hop": hop, "frames": frames, "variant": name, "inner": a.inner,
                   **stats(times[name]), "TBps": round(moved[name] / (med[name] * 1e-3) / 1e12, 3), "tag": a.tag}
            if name == "fused":
                rec.update(speedup_over_baseline=round(med["baseline"] / med["fused"], 2), speedup_over_composed=round(med["composed"] / med["fused"], 2),
                           speedup_over_torch=round(med["torch"] / med["fused"], 2), power_over_complex=round(med["fused"] / med["fused_power"], 2),
                           max_rel_dev_from_baseline=dev_base, max_rel_dev_from_composed=dev_comp, max_rel_dev_from_torch=dev_torch)
            if name == "istft":
                rec.update(speedup_over_torch=round(med["torch_istft"] / med["istft"], 2), max_abs_dev_round_trip=dev_inv, max_abs_dev_from_torch=dev_tinv)
            emit(rec)
        del x, X, Xb, Xt, P, y, inv_env
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
