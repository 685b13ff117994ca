"""Long batched 1-D real cross-spectrum (dfft_rxspec1d_long) against what a caller composes without it, and a whole fftconv1d_long
training step against torch's own autograd.  Per case (precision, m, n, rows on 16 channels) one JSON line per variant:

  fused      dfft_rxspec1d_long: pass A on both fields, the accumulating Mid kernel, the slice reduction
  composed   dfft_rxspec1d_long under DFFT_RXSPEC_LONG_FUSED=0: pad kernel and real rows of length m on both fields, multiply-accumulate,
             on the library's scratch
  baseline   the calls that exist without the entry point: torch zero-pad of both fields, dfft_rfft1d forward twice, torch
             conjugate-multiply, sum over the batch
  step_dfft  api.fftconv1d_long forward + backward with x and the taps (m - n + 1 of them) requiring grad (cases with n < m)
  step_torch the same step as torch.fft.irfft(torch.fft.rfft(x, m) * torch.fft.rfft(k, m), m)[..., :n] under torch's autograd

Timing: HIP events on the stream the work runs on, around `--inner` back-to-back calls; `--warmup` untimed rounds, `--reps` timed rounds
(>= 20) with the variants ALTERNATING inside every round, median and spread (p10 .. p90) of the per-call time.  fused_TBps =
2 * n * rows * sizeof(real) / time: the model in which each row of either field is read once and nothing else moves.

  python tools/lxspec_bench.py [--cases f64:65536:32768:1024,...] [--reps 20] [--out results.jsonl] [--tag run1] [--no-step]"""
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
    ap.add_argument("--inner", type=int, default=2, help="calls per timed window")
    ap.add_argument("--no-step", action="store_true", help="leave the training step out")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    assert a.reps >= 20, "at least 20 timed rounds"
    import torch
    from distributedfft_amd import _lib as L
    from distributedfft_amd import api
    if not torch.cuda.is_available():
        sys.exit("lxspec_bench: no HIP device (nothing is measured on a CPU)")
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
        g = (torch.rand((batch, CHANNELS, n), generator=gen, device=dev, dtype=torch.float32) - 0.5).to(rdt)
        taps = m - n + 1
        step = not a.no_step and n < m and api.rconv1d_long_length(n + taps - 1) == m
        k = (torch.rand((CHANNELS, taps), generator=gen, device=dev, dtype=torch.float32) - 0.5).to(rdt) if step else None
        nb = m // 2 + 1
        s_f = torch.empty((CHANNELS, nb), dtype=cdt, device=dev)
        s_c = torch.empty_like(s_f)
        bx = torch.empty((batch, CHANNELS, nb), dtype=cdt, device=dev)
        bg = torch.empty_like(bx)
        vp = C.c_void_p
        keep = {}

        def rxspec(dst):
            L.check(lib.dfft_rxspec1d_long(vp(x.data_ptr()), vp(g.data_ptr()), vp(dst.data_ptr()), n, m, CHANNELS, batch, code, 0, None),
                    "dfft_rxspec1d_long")

        def fused():
            rxspec(s_f)

        def composed():
            os.environ["DFFT_RXSPEC_LONG_FUSED"] = "0"
            try:
                rxspec(s_c)
            finally:
                os.environ.pop("DFFT_RXSPEC_LONG_FUSED", None)

        def baseline():
            xp = torch.nn.functional.pad(x, (0, m - n))
            gp = torch.nn.functional.pad(g, (0, m - n))
            L.check(lib.dfft_rfft1d(vp(xp.data_ptr()), vp(bx.data_ptr()), m, rows, code, api.FORWARD, None), "dfft_rfft1d")
            L.check(lib.dfft_rfft1d(vp(gp.data_ptr()), vp(bg.data_ptr()), m, rows, code, api.FORWARD, None), "dfft_rfft1d")
            keep["base"] = (bx.conj() * bg).sum(0)

        def step_dfft():
            xa, ka = x.detach().requires_grad_(True), k.detach().requires_grad_(True)
            api.fftconv1d_long(xa, ka).backward(g)
            keep["dfft"] = (xa.grad, ka.grad)

        def step_torch():
            xa, ka = x.detach().requires_grad_(True), k.detach().requires_grad_(True)
            torch.fft.irfft(torch.fft.rfft(xa, m) * torch.fft.rfft(ka, m), m)[..., :n].backward(g)
            keep["torch"] = (xa.grad, ka.grad)

        variants = [("fused", fused), ("composed", composed), ("baseline", baseline)]
        if step:
            variants += [("step_dfft", step_dfft), ("step_torch", step_torch)]
        is_fused = lib.dfft_rxspec1d_long_fused_applies(m, code) == 1
        # the routes agree before anything is timed
        fused()
        baseline()
        composed()
        torch.cuda.synchronize()
        scale = float(keep["base"].abs().max())
        dev_base = float((s_f - keep["base"]).abs().max()) / scale
        dev_comp = float((s_f - s_c).abs().max()) / scale
        tol = 1e-11 if prec == "f64" else 2e-3
        assert max(dev_base, dev_comp) < tol, (case, dev_base, dev_comp)
        dev_step = None
        if step:
            step_dfft()
            step_torch()
            torch.cuda.synchronize()
            dev_step = max(float((keep["dfft"][i] - keep["torch"][i]).abs().max() / keep["torch"][i].abs().max()) for i in (0, 1))
            assert dev_step < tol, (case, dev_step)
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
        moved = 2 * n * rows * rs
        a1, a2 = C.c_int(0), C.c_int(0)
        lib.dfft_rconv1d_long_split(m, C.byref(a1), C.byref(a2))
        for name, _ in variants:
            rec = {"case": case, "prec": prec, "m": m, "n": n, "rows": rows, "channels": CHANNELS, "variant": name, "inner": a.inner, **stats(times[name]),
                   "tag": a.tag}
            if name == "fused":
                rec.update(route="fused" if is_fused else "composed", split=[a1.value, a2.value],
                           slices=int(lib.dfft_rxspec1d_long_slices(m, CHANNELS, batch, code)),
                           fused_TBps=round(moved / (med["fused"] * 1e-3) / 1e12, 3),
                           speedup_over_baseline=round(med["baseline"] / med["fused"], 2), speedup_over_composed=round(med["composed"] / med["fused"], 2),
                           max_rel_dev_from_baseline=dev_base, max_rel_dev_from_composed=dev_comp)
            if name == "step_dfft":
                rec.update(taps=taps, speedup_over_torch=round(med["step_torch"] / med["step_dfft"], 2), max_rel_dev_from_torch=dev_step)
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        keep.clear()
        del x, g, k, s_f, s_c, bx, bg
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
