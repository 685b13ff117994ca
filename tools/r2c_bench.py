"""R2C forward, C2R backward and the C2C forward of the same shape, timed in ONE process on one GPU: warm-up, then the three plans
alternate execute by execute (HIP events around each execute, median of the repetitions), so drift of the device's clocks hits all three
alike.  One JSON line per shape; --out writes them all to a file.

  python tools/r2c_bench.py [--reps 30] [--warmup 5] [--shapes 256x256x256:f64,512x512x512:f64,...] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

DEFAULT = "256x256x256:f64,512x512x512:f64,512x512x512:f32,1024x768x512:f64"


def bench_shape(N, prec, reps, warmup):
    import torch
    from distributedfft_amd import api
    dev = torch.device("cuda:0")
    n0, n1, n2 = N
    rdt, cdt = (torch.float64, torch.complex128) if prec == "f64" else (torch.float32, torch.complex64)
    rc, cc = api.r2c_counts(n0, n1, n2, 1, 0)
    mc = api.get_max_data_count(n0, n1, n2, 1, True)
    g = torch.Generator(device=dev).manual_seed(1)
    xr = torch.randn(rc, dtype=rdt, device=dev, generator=g)
    bins = torch.zeros(cc, dtype=cdt, device=dev)
    xr_back = torch.zeros(rc, dtype=rdt, device=dev)
    xc = torch.randn(mc, dtype=cdt, device=dev, generator=g)
    yc = torch.zeros(mc, dtype=cdt, device=dev)
    torch.cuda.synchronize()
    plans = {
        "r2c_fwd": api.PlanR2C(n0, n1, n2, xr, bins, None, 0, 1, api.FORWARD, api.PLAN_INPUT_FROM_IN),
        "c2r_bwd": api.PlanR2C(n0, n1, n2, bins, xr_back, None, 0, 1, api.BACKWARD, api.PLAN_INPUT_FROM_IN),
        "c2c_fwd": api.Plan(n0, n1, n2, xc, yc, None, 0, 1, api.FORWARD, api.PLAN_INPUT_FROM_IN),
    }
    plans["c2c_fwd"].tune()  # as bench.py does for out-of-place C2C plans
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
    eb = 16 if prec == "f64" else 8
    nh = n2 // 2 + 1
    # algorithmic HBM bytes: R2C = read the reals, Z->Y hand-over crosses the cache, X pass reads + writes the bins (single GPU)
    return {"shape": "x".join(map(str, N)), "dtype": prec, "reps": reps, "ms": {k: round(v, 4) for k, v in med.items()},
            "ms_min": {k: round(min(v), 4) for k, v in ms.items()},
            "ratio_r2c_over_c2c": round(med["r2c_fwd"] / med["c2c_fwd"], 3),
            "ratio_c2r_over_c2c": round(med["c2r_bwd"] / med["c2c_fwd"], 3),
            "bins_bytes": n0 * n1 * nh * eb, "c2c_bytes": n0 * n1 * n2 * eb, "describe": desc}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default=DEFAULT)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for item in a.shapes.split(","):
        shp, prec = item.split(":")
        r = bench_shape(tuple(int(v) for v in shp.split("x")), prec, a.reps, a.warmup)
        print(json.dumps(r), flush=True)
        rows.append(r)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
