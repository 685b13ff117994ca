"""Spectral-filter plans (api.PlanConv) against the composed route of the C2C API: forward Plan (placed with dfft_plan_tune as bench.py
does) -> torch.mul by H in the result layout -> backward Plan with the scale folded.  One JSON line per (shape, precision, P, variant).

Timing: HIP events on the stream the work runs on (the plan's own stream through torch.cuda.ExternalStream; torch's for torch.mul),
`--warmup` untimed rounds, `--reps` timed ones (>= 20), median and spread (p10 .. p90).  The composed route is charged the SUM of its three
pieces' device times -- none of the host synchronisation a caller needs between them -- so the baseline is a lower bound of what it costs.
P > 1 (virtual devices on one GPU, LOCAL communicator, one thread per device): wall-clock time of execute + sync between two thread
barriers; the exchange is host-synchronising there and has no device time line of its own.
Placement moves these kernels by 5-8 % from one process to the next: run the tool several times (the records carry `--tag`).

  python tools/conv_bench.py [--cases 256x256x256:f64:1,...] [--reps 20] [--out results.jsonl] [--tag run1]
  DFFT_LIB=<build of the parent commit> python tools/conv_bench.py --composed-only ...       the yardstick on the code before this feature"""
import argparse
import json
import os
import statistics
import sys
import threading
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

DEFAULT_CASES = "256x256x256:f64:1,512x512x512:f64:1,512x512x512:f32:1,1024x768x512:f64:1,512x512x512:f64:4"


def stats(ms):
    s = sorted(ms)
    return {"median_ms": round(statistics.median(s), 4), "p10_ms": round(s[len(s) // 10], 4), "p90_ms": round(s[(9 * len(s)) // 10], 4), "n": len(s)}


def time_on_stream(torch, stream, fn, warmup, reps):
    ext = torch.cuda.ExternalStream(stream) if stream else torch.cuda.current_stream()
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(ext)
        fn()
        b.record(ext)
        b.synchronize()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def slab(n, P, g):
    blk = -(-n // P)
    return g * blk, (blk if g < P - 1 else n - (P - 1) * blk)


def run_threads(P, work):
    errs = []

    def wrap(g):
        try:
            work(g)
        except Exception as e:  # pragma: no cover
            errs.append(e)
    th = [threading.Thread(target=wrap, args=(g,)) for g in range(P)]
    [t.start() for t in th]
    [t.join() for t in th]
    if errs:
        raise errs[0]


def wall_rounds(P, step, warmup, reps):
    """Every device thread runs step(g) per round between two barriers; returns the rounds' wall-clock times in ms (thread 0's clock)."""
    bar = threading.Barrier(P)
    out = []

    def work(g):
        for r in range(warmup + reps):
            bar.wait()
            t0 = time.perf_counter()
            step(g)
            bar.wait()
            if g == 0 and r >= warmup:
                out.append((time.perf_counter() - t0) * 1e3)
    run_threads(P, work)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="n0xn1xn2:f64|f32:P, comma-separated")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="")
    ap.add_argument("--composed-only", action="store_true", help="only the composed route (runs on a library without the conv entry points)")
    ap.add_argument("--conv-only", action="store_true")
    a = ap.parse_args()
    assert a.reps >= 20, "at least 20 timed executes"
    import torch
    from distributedfft_amd import api
    dev = torch.device("cuda:0")
    out = open(a.out, "a") if a.out else None
    libname = os.environ.get("DFFT_LIB", "tree")

    def emit(rec):
        rec.update(tag=a.tag, lib=libname)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for case in a.cases.split(","):
        shape, prec, P = case.split(":")
        N = tuple(int(v) for v in shape.split("x"))
        P = int(P)
        n0, n1, n2 = N
        cdt, rdt, S = (torch.complex128, torch.float64, 16) if prec == "f64" else (torch.complex64, torch.float32, 8)
        vol = n0 * n1 * n2
        base = {"case": case, "N": list(N), "prec": prec, "P": P, "volume_GiB": round(vol * S / 2 ** 30, 3)}
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234)
        comm = api.Comm.local(P) if P > 1 else None
        xs = [slab(n0, P, g)[1] for g in range(P)]
        ys = [slab(n1, P, g)[1] for g in range(P)]
        mc = [api.get_max_data_count(n0, n1, n2, P, g == P - 1) for g in range(P)]
        ins = [(torch.rand(mc[g], generator=gen, device=dev, dtype=torch.float32) - 0.5).to(cdt) for g in range(P)]
        hc = [(torch.rand(ys[g] * n2 * n0, generator=gen, device=dev, dtype=torch.float32) - 0.5).to(cdt) for g in range(P)]
        hr = [torch.rand(ys[g] * n2 * n0, generator=gen, device=dev, dtype=torch.float32).to(rdt) for g in range(P)]
        torch.cuda.synchronize()

        if not a.conv_only:
            # ---- composed route: forward plan, torch.mul, backward plan (scale folded)
            mids = [torch.zeros(mc[g], dtype=cdt, device=dev) for g in range(P)]
            outs = [torch.zeros(mc[g], dtype=cdt, device=dev) for g in range(P)]
            fw = [api.Plan(n0, n1, n2, ins[g], mids[g], comm, g, P, api.FORWARD, api.PLAN_INPUT_FROM_IN) for g in range(P)]
            bw = [api.Plan(n0, n1, n2, mids[g], outs[g], comm, g, P, api.BACKWARD, api.PLAN_INPUT_FROM_IN) for g in range(P)]
            for p in bw:
                p.set_scale(1.0 / vol)
            for p in fw + bw:
                p.tune()
            mul = [(lambda g=g: torch.mul(mids[g][:hc[g].numel()], hc[g], out=mids[g][:hc[g].numel()])) for g in range(P)]
            if P == 1:
                tf = time_on_stream(torch, fw[0].stream, lambda: fw[0].execute(api.EXEC_NO_TIMING), a.warmup, a.reps)
                tm = time_on_stream(torch, None, mul[0], a.warmup, a.reps)
                tb = time_on_stream(torch, bw[0].stream, lambda: bw[0].execute(api.EXEC_NO_TIMING), a.warmup, a.reps)
                tot = [x + y + z for x, y, z in zip(tf, tm, tb)]
                fw[0].execute()
                fw[0].sync()
                stf = fw[0].stage_times()
                bw[0].execute()
                bw[0].sync()
                stb = bw[0].stage_times()
                emit(dict(base, variant="composed", **stats(tot), forward=stats(tf), mul=stats(tm), backward=stats(tb),
                          forward_stage_ms=[round(v * 1e3, 4) for v in stf], backward_stage_ms=[round(v * 1e3, 4) for v in stb], describe=fw[0].describe()))
            else:
                def step(g):
                    fw[g].execute(api.EXEC_NO_TIMING)
                    fw[g].sync()
                    mul[g]()
                    torch.cuda.synchronize()
                    bw[g].execute(api.EXEC_NO_TIMING)
                    bw[g].sync()
                emit(dict(base, variant="composed", timing="wall", **stats(wall_rounds(P, step, a.warmup, a.reps)), describe=fw[0].describe()))
            for p in fw + bw:
                p.destroy()
            del mids, outs, fw, bw
            torch.cuda.empty_cache()

        if not a.composed_only:
            for variant, env, filt in (("conv-fused-complex", {}, hc), ("conv-fused-real", {}, hr), ("conv-multi-complex", {"DFFT_CONV_FUSED": "0"}, hc)):
                os.environ.update(env)
                outs = [torch.zeros(mc[g], dtype=cdt, device=dev) for g in range(P)]
                try:
                    cv = [api.PlanConv(n0, n1, n2, ins[g][:xs[g] * n1 * n2], outs[g][:xs[g] * n1 * n2], comm, g, P) for g in range(P)]
                finally:
                    for k in env:
                        os.environ.pop(k, None)
                for g in range(P):
                    cv[g].set_filter(filt[g])
                if P == 1:
                    t = time_on_stream(torch, cv[0].stream, lambda: cv[0].execute(api.EXEC_NO_TIMING), a.warmup, a.reps)
                    st = []
                    for _ in range(5):
                        cv[0].execute()
                        cv[0].sync()
                        st.append(cv[0].stage_times())
                    stm = [statistics.median(s[i] for s in st) for i in range(4)]
                    streams = 2.5 if variant.endswith("real") else 3.0  # data in, filter (half for a real one), data out
                    rec = dict(base, variant=variant, **stats(t), stage_ms=[round(v * 1e3, 4) for v in stm], describe=cv[0].describe())
                    if "xconv=fused" in rec["describe"]:
                        rec["x_stage_TBps"] = round(streams * vol * S / stm[2] / 1e12, 3)
                    emit(rec)
                else:
                    def step(g):
                        cv[g].execute(api.EXEC_NO_TIMING)
                        cv[g].sync()
                    emit(dict(base, variant=variant, timing="wall", **stats(wall_rounds(P, step, a.warmup, a.reps)), describe=cv[0].describe()))
                for p in cv:
                    p.destroy()
                del outs, cv
                torch.cuda.empty_cache()
        if comm:
            comm.destroy()
        del ins, hc, hr
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
