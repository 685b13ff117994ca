"""Timing of the any-length real transforms on one GPU, every variant of a case alternated execute by execute in ONE process (HIP events
around each call, median of --reps after --warmup), so drift of the device's clocks hits all variants alike.  One JSON line per case.

  python tools/real_any_bench.py [--reps 30] [--warmup 5] [--out profiles/r10/real_any_bench.jsonl] [--only 1d|3d]

1-D: dfft_rfft1d forward / backward on at least 256 MiB of reals against the same rows widened to complex through dfft_fft1d_rows
(single-pass and four-step n) or dfft_fft1d_any (Bluestein n), forward / backward, out of place; ratio = real / widened.
3D: api.PlanR2C(any_length=True) forward and backward (INPUT_FROM_IN) against the C2C plan of the same shape, forward."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

N1D = [125, 243, 375, 2187, 3125, 15625, 97, 1009]
N3D = [125, 243, 375]


def _time(fns, reps, warmup, stream):
    """fns: name -> callable enqueuing on `stream`.  Median / min ms per name, the names alternated call by call."""
    import torch
    ms = {k: [] for k in fns}
    for it in range(warmup + reps):
        for k, f in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(stream)
            f()
            e.record(stream)
            e.synchronize()
            if it >= warmup:
                ms[k].append(s.elapsed_time(e))
    return {k: statistics.median(v) for k, v in ms.items()}, {k: min(v) for k, v in ms.items()}


def bench_1d(n, prec, reps, warmup):
    import torch
    from distributedfft_amd import _lib, api
    lib = _lib.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)
    rdt, cdt = (torch.float64, torch.complex128) if prec == "f64" else (torch.float32, torch.complex64)
    rb = 8 if prec == "f64" else 4
    batch = -(-(256 << 20) // (rb * n))
    batch += batch % 2
    nh = n // 2 + 1
    code = api.F64 if prec == "f64" else api.F32
    x = torch.randn(batch, n, dtype=rdt, device=dev)
    X = torch.empty(batch, nh, dtype=cdt, device=dev)
    xb = torch.empty(batch, n, dtype=rdt, device=dev)
    xc = x.to(cdt)
    yc = torch.empty_like(xc)
    zc = torch.empty_like(xc)
    kind = api.length_kind(n)

    def widened(src, dst, d):
        if kind == 3:
            return lib.dfft_fft1d_any(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), n, 1, batch, code, d, sp)
        return lib.dfft_fft1d_rows(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), n, batch, code, d, sp)

    fns = {
        "rfft": lambda: lib.dfft_rfft1d(C.c_void_p(x.data_ptr()), C.c_void_p(X.data_ptr()), n, batch, code, api.FORWARD, sp),
        "c2c_fwd": lambda: widened(xc, yc, api.FORWARD),
        "irfft": lambda: lib.dfft_rfft1d(C.c_void_p(X.data_ptr()), C.c_void_p(xb.data_ptr()), n, batch, code, api.BACKWARD, sp),
        "c2c_bwd": lambda: widened(yc, zc, api.BACKWARD),
    }
    for f in fns.values():  # first calls build tables / scratch outside the timing
        assert f() == 0, _lib.load().dfft_last_error()
    torch.cuda.synchronize()
    med, mn = _time(fns, reps, warmup, stream)
    return {"case": "1d", "n": n, "dtype": prec, "real_form": api.real_form(n), "complex_kind": kind, "batch": batch,
            "real_bytes": batch * n * rb, "reps": reps, "ms": {k: round(v, 4) for k, v in med.items()},
            "ms_min": {k: round(v, 4) for k, v in mn.items()},
            "ratio_rfft_over_c2c": round(med["rfft"] / med["c2c_fwd"], 3), "ratio_irfft_over_c2c": round(med["irfft"] / med["c2c_bwd"], 3)}


def bench_3d(n, prec, reps, warmup):
    import torch
    from distributedfft_amd import api
    dev = torch.device("cuda:0")
    N = (n, n, n)
    rdt, cdt = (torch.float64, torch.complex128) if prec == "f64" else (torch.float32, torch.complex64)
    rc, cc = api.r2c_counts(*N, 1, 0)
    mc = api.get_max_data_count(*N, 1, True)
    xr = torch.randn(rc, dtype=rdt, device=dev)
    bins = torch.zeros(cc, dtype=cdt, device=dev)
    xr_back = torch.zeros(rc, dtype=rdt, device=dev)
    xc = torch.randn(mc, dtype=cdt, device=dev)
    yc = torch.zeros(mc, dtype=cdt, device=dev)
    torch.cuda.synchronize()
    plans = {
        "r2c_fwd": api.PlanR2C(*N, xr, bins, None, 0, 1, api.FORWARD, api.PLAN_INPUT_FROM_IN, any_length=True),
        "c2r_bwd": api.PlanR2C(*N, bins, xr_back, None, 0, 1, api.BACKWARD, api.PLAN_INPUT_FROM_IN, any_length=True),
        "c2c_fwd": api.Plan(*N, xc, yc, None, 0, 1, api.FORWARD, api.PLAN_INPUT_FROM_IN),
    }
    plans["c2c_fwd"].tune()
    ms = {k: [] for k in plans}
    stream = {k: torch.cuda.ExternalStream(p.stream) for k, p in plans.items()}
    for it in range(warmup + reps):
        for k, p in plans.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(stream[k])
            p.execute(api.EXEC_NO_TIMING)
            e.record(stream[k])
            e.synchronize()
            if it >= warmup:
                ms[k].append(s.elapsed_time(e))
    desc = {k: p.describe() for k, p in plans.items()}
    for p in plans.values():
        p.destroy()
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"case": "3d", "shape": f"{n}x{n}x{n}", "dtype": prec, "reps": reps, "ms": {k: round(v, 4) for k, v in med.items()},
            "ms_min": {k: round(min(v), 4) for k, v in ms.items()},
            "ratio_r2c_over_c2c": round(med["r2c_fwd"] / med["c2c_fwd"], 3), "ratio_c2r_over_c2c": round(med["c2r_bwd"] / med["c2c_fwd"], 3),
            "describe": desc}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["1d", "3d"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    rows = []
    if a.only in (None, "1d"):
        for prec in ("f64", "f32"):
            for n in N1D:
                rows.append(bench_1d(n, prec, a.reps, a.warmup))
                print(json.dumps(rows[-1]), flush=True)
                torch.cuda.empty_cache()
    if a.only in (None, "3d"):
        for n in N3D:
            rows.append(bench_3d(n, "f64", a.reps, a.warmup))
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
