"""Batched 1-D real cross-spectrum (dfft_rxspec1d) against what a caller composes without it, and a whole fftconv1d training step against
torch's own autograd.  Per case (precision, m; n = m / 2, 4096 batch entries on 16 channels) one JSON line per variant:

  fused      dfft_rxspec1d, the one-launch kernel (plus the slice reduction)
  composed   dfft_rxspec1d under DFFT_RXSPEC_FUSED=0: pad kernel and R2C rows on both fields, multiply-accumulate, on the library's scratch
  baseline   the calls that exist without the entry point: torch zero-pad of both fields, dfft_rfft1d forward twice, torch
             conjugate-multiply, sum over the batch
  read       sum over the batch of x * g (reads the 2 * n * rows reals the kernel reads, writes next to nothing): the floor of anything
             that reads both fields once
  step_dfft  api.fftconv1d forward + backward with x and the taps (n of them) requiring grad
  step_torch the same step as torch.fft.irfft(torch.fft.rfft(x, m) * torch.fft.rfft(k, m), m)[..., :n] under torch's autograd

Timing: HIP events on the stream the work runs on, around `--inner` back-to-back calls; `--warmup` untimed rounds, `--reps` timed rounds
(>= 20) with the variants ALTERNATING inside every round, median and spread (p10 .. p90) of the per-call time.  fused_TBps =
2 * n * rows * sizeof(real) / time: the model in which each row of either field is read once and nothing else moves.

  python tools/rxspec_bench.py [--cases f64:8192,...] [--reps 20] [--out results.jsonl] [--tag run1] [--no-step]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

DEFAULT_CASES = "f64:512,f32:512,f64:2048,f32:2048,f64:8192,f32:8192"
CHANNELS, BATCH = 16, 4096


def stats(ms):
    s = sorted(ms)
    return {"median_ms": round(statistics.median(s), 5), "p10_ms": round(s[len(s) // 10], 5), "p90_ms": round(s[(9 * len(s)) // 10], 5), "samples": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="f64|f32:m, comma-separated (n = m / 2)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=2, help="calls per timed window")
    ap.add_argument("--batch", type=int, default=BATCH)
    ap.add_argument("--no-step", action="store_true", help="leave the training step out")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    assert a.reps >= 20, "at least 20 timed rounds"
    import torch
    from distributedfft_amd import _lib as L
    from distributedfft_amd import api
    if not torch.cuda.is_available():
        sys.exit("rxspec_bench: no HIP device (nothing is measured on a CPU)")
    lib = L.load()
    dev = torch.device("cuda:0")
    out = open(a.out, "a") if a.out else None
    batch = a.batch
    rows = CHANNELS * batch

    for case in a.cases.split(","):
        prec, m = case.split(":")
        m = int(m)
        n = m // 2
        rdt, cdt, code, rs = (torch.float64, torch.complex128, api.F64, 8) if prec == "f64" else (torch.float32, torch.complex64, api.F32, 4)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234)
        x = (torch.rand((batch, CHANNELS, n), generator=gen, device=dev, dtype=torch.float32) - 0.5).to(rdt)
        g = (torch.rand((batch, CHANNELS, n), generator=gen, device=dev, dtype=torch.float32) - 0.5).to(rdt)
        k = (torch.rand((CHANNELS, n), generator=gen, device=dev, dtype=torch.float32) - 0.5).to(rdt)
        nb = m // 2 + 1
        s_f = torch.empty((CHANNELS, nb), dtype=cdt, device=dev)
        s_c = torch.empty_like(s_f)
        bx = torch.empty((batch, CHANNELS, nb), dtype=cdt, device=dev)
        bg = torch.empty_like(bx)
        vp = C.c_void_p
        keep = {}

        def rxspec(dst):
            L.check(lib.dfft_rxspec1d(vp(x.data_ptr()), vp(g.data_ptr()), vp(dst.data_ptr()), n, m, CHANNELS, batch, code, None), "dfft_rxspec1d")

        def fused():
            rxspec(s_f)

        def composed():
            os.environ["DFFT_RXSPEC_FUSED"] = "0"
            try:
                rxspec(s_c)
            finally:
                os.environ.pop("DFFT_RXSPEC_FUSED", None)

        def baseline():
            xp = torch.nn.functional.pad(x, (0, m - n))
            gp = torch.nn.functional.pad(g, (0, m - n))
            L.check(lib.dfft_rfft1d(vp(xp.data_ptr()), vp(bx.data_ptr()), m, rows, code, api.FORWARD, None), "dfft_rfft1d")
            L.check(lib.dfft_rfft1d(vp(gp.data_ptr()), vp(bg.data_ptr()), m, rows, code, api.FORWARD, None), "dfft_rfft1d")
            keep["base"] = (bx.conj() * bg).sum(0)

        def read():
            keep["read"] = (x * g).sum(0)

        def step_dfft():
            xa, ka = x.detach().requires_grad_(True), k.detach().requires_grad_(True)
            api.fftconv1d(xa, ka).backward(g)
            keep["dfft"] = (xa.grad, ka.grad)

        def step_torch():
            xa, ka = x.detach().requires_grad_(True), k.detach().requires_grad_(True)
            torch.fft.irfft(torch.fft.rfft(xa, m) * torch.fft.rfft(ka, m), m)[..., :n].backward(g)
            keep["torch"] = (xa.grad, ka.grad)

        variants = [("fused", fused), ("composed", composed), ("baseline", baseline), ("read", read)]
        if not a.no_step:
            variants += [("step_dfft", step_dfft), ("step_torch", step_torch)]
        is_fused = lib.dfft_rxspec1d_fused_applies(n, m, code, 1) == 1
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
        if not a.no_step:
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
        for name, _ in variants:
            rec = {"case": case, "prec": prec, "m": m, "n": n, "rows": rows, "channels": CHANNELS, "variant": name, "inner": a.inner, **stats(times[name]),
                   "tag": a.tag}
            if name == "fused":
                rec.update(route="fused" if is_fused else "composed", slices=int(lib.dfft_rxspec1d_slices(m, CHANNELS, batch, code)),
                           fused_TBps=round(moved / (med["fused"] * 1e-3) / 1e12, 3), fused_of_read=round(med["read"] / med["fused"], 3),
                           speedup_over_baseline=round(med["baseline"] / med["fused"], 2), speedup_over_composed=round(med["composed"] / med["fused"], 2),
                           max_rel_dev_from_baseline=dev_base, max_rel_dev_from_composed=dev_comp)
            if name == "read":
                rec.update(read_TBps=round(moved / (med["read"] * 1e-3) / 1e12, 3))
            if name == "step_dfft":
                rec.update(speedup_over_torch=round(med["step_torch"] / med["step_dfft"], 2), max_rel_dev_from_torch=dev_step)
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
