"""Timing of the any-length (Bluestein) transforms on one GPU: every form in one process, alternated round by round, median of
--reps device-event timings per form.  One JSON line per form.

  python tools/bluestein_bench.py [--reps 30] [--out profiles/r09/bluestein_bench.jsonl]

Forms: fused rows at n = 1009 and 2039 (fp64, fp32, about 1 GiB per buffer), the same n under DFFT_BLUESTEIN_FUSED=0 (multi-pass form),
the 7-smooth neighbours 1000 and 2048 through dfft_fft1d_rows, fused columns at n = 97 with s = 1024, and 3D plans 97 x 256 x 256 and
251^3 (fp64, DFFT_PLAN_ANY_LENGTH, P = 1).  Per form: median time, algorithmic bytes (2 n batch s elem: one read and one write), flops
(Bluestein: 2 (5 M log2 M) + 12 M per transform; a 7-smooth length: 5 n log2 n) and the share of the larger of the two bounds -- HBM
8 TB/s (MI355X_MICROARCH.md), vector peak 78.6 TFLOPS fp64 (AMD's published MI355X specification; the microarchitecture guide gives no
fp64 figure) and 157.3 TFLOPS fp32."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM = 8e12
PEAK = {"f64": 78.6e12, "f32": 157.3e12}
GIB = 1 << 30


def bluestein_flops(M):
    return 2 * 5 * M * math.log2(M) + 12 * M


def smooth_flops(n):
    return 5 * n * math.log2(n)


def main():
    import torch
    from distributedfft_amd import _lib, api
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)
    cases = []  # dicts: name, run (callable), bytes, flops, prec, env

    def rows_case(name, n, prec, fn, flops_per, env=None, s=1, target=GIB):
        eb = 16 if prec == "f64" else 8
        batch = max(1, target // (n * s * eb))
        dt = torch.complex128 if prec == "f64" else torch.complex64
        x = torch.randn(batch * n * s, dtype=dt, device=dev)
        y = torch.empty_like(x)
        code = api.F64 if prec == "f64" else api.F32

        def run():
            if fn == "any":
                rc = lib.dfft_fft1d_any(x.data_ptr(), y.data_ptr(), n, s, batch, code, api.FORWARD, sp)
            else:
                rc = lib.dfft_fft1d_rows(x.data_ptr(), y.data_ptr(), n, batch, code, api.FORWARD, sp)
            _lib.check(rc, name)
        cases.append(dict(name=name, n=n, s=s, batch=batch, prec=prec, run=run, env=env or {},
                          bytes=2 * n * batch * s * eb, flops=flops_per * batch * s, M=api.bluestein_length(n)))

    for n in (1009, 2039):
        M = api.bluestein_length(n)
        for prec in ("f64", "f32"):
            rows_case(f"fused_rows_n{n}_{prec}", n, prec, "any", bluestein_flops(M))
            rows_case(f"multipass_rows_n{n}_{prec}", n, prec, "any", bluestein_flops(M), env={"DFFT_BLUESTEIN_FUSED": "0"})
    for n in (1000, 2048):
        for prec in ("f64", "f32"):
            rows_case(f"smooth_rows_n{n}_{prec}", n, prec, "rows", smooth_flops(n))
    for prec in ("f64", "f32"):
        rows_case(f"fused_cols_n97_s1024_{prec}", 97, prec, "any", bluestein_flops(api.bluestein_length(97)), s=1024)

    plans = []
    for N in ((97, 256, 256), (251, 251, 251)):
        total = N[0] * N[1] * N[2]
        x = torch.randn(total, dtype=torch.complex128, device=dev)
        y = torch.empty_like(x)
        torch.cuda.synchronize()
        p = api.Plan(*N, x, y, None, 0, 1, api.FORWARD, api.PLAN_ANY_LENGTH)
        plans.append(p)
        fl = 0.0
        for ax, n in enumerate(N):
            per = bluestein_flops(api.bluestein_length(n)) if api.length_kind(n) == 3 else smooth_flops(n)
            fl += per * total / n

        def run(p=p):
            p.execute(api.EXEC_NO_TIMING)
        cases.append(dict(name=f"plan3d_{N[0]}x{N[1]}x{N[2]}_f64", n=N, s=1, batch=1, prec="f64", run=run, env={}, plan=p,
                          bytes=2 * total * 16, flops=fl, M=[api.bluestein_length(n) for n in N], describe=p.describe()))

    def timed(c):
        old = {k: os.environ.get(k) for k in c["env"]}
        os.environ.update(c["env"])
        try:
            if "plan" in c:
                c["plan"].execute(api.EXEC_ASYNC)  # the plan's own stream; its stage events give the device time
                return sum(c["plan"].stage_times())
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            c["run"]()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v

    for c in cases:  # warm-up (tables, scratch, occupancy queries)
        for _ in range(3):
            timed(c)
    times = {c["name"]: [] for c in cases}
    for _ in range(a.reps):
        for c in cases:
            times[c["name"]].append(timed(c))
    lines = []
    for c in cases:
        t = statistics.median(times[c["name"]])
        bound = max(c["bytes"] / HBM, c["flops"] / PEAK[c["prec"]])
        rec = {"form": c["name"], "n": c["n"], "s": c["s"], "batch": c["batch"], "M": c["M"], "median_ms": round(t * 1e3, 4),
               "min_ms": round(min(times[c["name"]]) * 1e3, 4), "bytes": c["bytes"], "flops": round(c["flops"]),
               "TB_per_s": round(c["bytes"] / t / 1e12, 3), "TFLOPS": round(c["flops"] / t / 1e12, 3),
               "bound": "hbm" if c["bytes"] / HBM >= c["flops"] / PEAK[c["prec"]] else "flops",
               "share_of_bound": round(bound / t, 3), "reps": a.reps}
        if "describe" in c:
            rec["describe"] = c["describe"]
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    for p in plans:
        p.destroy()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
