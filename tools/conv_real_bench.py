"""Real-field spectral-filter plans (api.PlanConvReal) against api.PlanConv on the same field widened to complex: the yardstick is the
C2C plan of the same build, whose code the real plans do not touch.  One process; the two plans are executed ALTERNATELY, call by call
(real, complex, real, ...), each timed by HIP events on its own stream, `--warmup` untimed rounds, then `--reps` timed ones (30 by
default); medians and the p10 .. p90 spread.  Per-stage times (forward YZ stage, exchanges, X stage, inverse YZ stage) are medians of
dfft_stage_times over five further timed executes of each plan.  One JSON line per (shape, precision, filter kind), and a Markdown table
at the end (profiles/r13/README.md quotes it).

The widening (real -> complex) and narrowing passes a caller of PlanConv pays for a real field are NOT charged to the complex plan: the
ratio is plan against plan.

  python tools/conv_real_bench.py [--cases 256x256x256:f64,...] [--reps 30] [--out results.jsonl] [--table table.md]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

DEFAULT_CASES = "256x256x256:f64,256x256x256:f32,512x512x512:f64,512x512x512:f32"


def stats(ms):
    s = sorted(ms)
    return {"median_ms": round(statistics.median(s), 4), "p10_ms": round(s[len(s) // 10], 4), "p90_ms": round(s[(9 * len(s)) // 10], 4), "n": len(s)}


def timed(torch, plan, flags):
    """One execute between two events on the plan's stream; the elapsed time is read after both plans of a round have been queued."""
    ext = torch.cuda.ExternalStream(plan.stream)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(ext)
    plan.execute(flags)
    b.record(ext)
    b.synchronize()
    return a.elapsed_time(b)


def stage_medians(plan, n=5):
    st = []
    for _ in range(n):
        plan.execute()
        plan.sync()
        st.append(plan.stage_times())
    return [round(statistics.median(s[i] for s in st) * 1e3, 4) for i in range(4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="n0xn1xn2:f64|f32, comma-separated")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--table", default=None)
    a = ap.parse_args()
    import torch
    from distributedfft_amd import api
    dev = torch.device("cuda:0")
    out = open(a.out, "a") if a.out else None
    rows = []
    for case in a.cases.split(","):
        shape, prec = case.split(":")
        n0, n1, n2 = (int(v) for v in shape.split("x"))
        nh = n2 // 2 + 1
        cdt, rdt = (torch.complex128, torch.float64) if prec == "f64" else (torch.complex64, torch.float32)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234)
        x = torch.randn(n0 * n1 * n2, generator=gen, device=dev, dtype=torch.float32).to(rdt)
        xc = x.to(cdt)
        yr, yc = torch.zeros_like(x), torch.zeros_like(xc)
        # an even real filter on the full spectrum [n1][n2][n0] and its half [n1][nh][n0]; the complex one is random (timing only)
        hfull = torch.rand(n1, n2, n0, generator=gen, device=dev, dtype=torch.float32).to(rdt)
        filters = {"real": (hfull[:, :nh, :].contiguous().reshape(-1), hfull.reshape(-1))}
        filters["complex"] = (filters["real"][0].to(cdt) * (0.6 + 0.8j), filters["real"][1].to(cdt) * (0.6 + 0.8j))
        del hfull
        torch.cuda.synchronize()
        pr = api.PlanConvReal(n0, n1, n2, x, yr, None, 0, 1)
        pc = api.PlanConv(n0, n1, n2, xc, yc, None, 0, 1)
        for kind in ("complex", "real"):
            pr.set_filter(filters[kind][0])
            pc.set_filter(filters[kind][1])
            for _ in range(a.warmup):
                timed(torch, pr, api.EXEC_NO_TIMING)
                timed(torch, pc, api.EXEC_NO_TIMING)
            tr, tc = [], []
            for _ in range(a.reps):
                tr.append(timed(torch, pr, api.EXEC_NO_TIMING))
                tc.append(timed(torch, pc, api.EXEC_NO_TIMING))
            sr, sc = stats(tr), stats(tc)
            rec = {"case": case, "filter": kind, "real": sr, "complex": sc, "ratio": round(sr["median_ms"] / sc["median_ms"], 3),
                   "real_stage_ms": stage_medians(pr), "complex_stage_ms": stage_medians(pc), "real_describe": pr.describe(),
                   "complex_describe": pc.describe()}
            rows.append(rec)
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        pr.destroy()
        pc.destroy()
        del x, xc, yr, yc, filters
        torch.cuda.empty_cache()
    head = ["| shape | filter | PlanConvReal ms (p10 .. p90) | PlanConv ms (p10 .. p90) | ratio | real stages ms (YZ, exch, X, YZ^-1) | complex stages ms |",
            "|---|---|---|---|---|---|---|"]
    for r in rows:
        head.append(f"| {r['case']} | {r['filter']} | {r['real']['median_ms']:.3f} ({r['real']['p10_ms']:.3f} .. {r['real']['p90_ms']:.3f}) | "
                    f"{r['complex']['median_ms']:.3f} ({r['complex']['p10_ms']:.3f} .. {r['complex']['p90_ms']:.3f}) | {r['ratio']:.3f} | "
                    f"{' / '.join(f'{v:.3f}' for v in r['real_stage_ms'])} | {' / '.join(f'{v:.3f}' for v in r['complex_stage_ms'])} |")
    table = "\n".join(head) + "\n"
    print(table, end="")
    if a.table:
        Path(a.table).parent.mkdir(parents=True, exist_ok=True)
        Path(a.table).write_text(table)


if __name__ == "__main__":
    main()
