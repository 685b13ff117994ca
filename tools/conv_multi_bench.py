"""Multi-output real-field spectral-filter plans (api.PlanConvRealMulti) against K api.PlanConvReal plans executed back to back, each with
its own filter H . a_k (x) b_k (x) c_k: the yardstick is the single-output plan of the same build, whose code the multi plan does not
touch.  One process; the two sides are executed ALTERNATELY, call by call (multi, K singles, multi, ...), each execute timed by HIP events
on its plan's stream; a round of singles is the sum of its K executes, each queued when the one before has finished.  `--warmup` untimed
rounds, then `--reps` timed ones (30 by default); medians and the p10 .. p90 spread.  Per-stage times (forward YZ stage, exchanges, X
stage, inverse YZ stages) are medians of dfft_stage_times over five further timed executes.  One JSON line per (shape, precision, filter
kind, K), and a Markdown table at the end (profiles/r14/README.md quotes it).

  python tools/conv_multi_bench.py [--cases 256x256x256:f64,...] [--outputs 3,4] [--reps 30] [--out results.jsonl] [--table table.md]"""
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


def timed_multi(torch, plan, flags):
    ext = torch.cuda.ExternalStream(plan.stream)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(ext)
    plan.execute(flags)
    b.record(ext)
    b.synchronize()
    return a.elapsed_time(b)


def timed_singles(torch, plans, flags):
    """K single-output executes back to back: the sum of their device times (each plan has its own stream; the next is queued when the
    one before has finished, so nothing overlaps and nothing waits on the host inside a measured interval)."""
    total = 0.0
    for p in plans:
        total += timed_multi(torch, p, flags)
    return total


def stage_medians(plans, n=5):
    st = []
    for _ in range(n):
        t = [0.0] * 4
        for p in plans:
            p.execute()
            p.sync()
            t = [u + v for u, v in zip(t, p.stage_times())]
        st.append(t)
    return [round(statistics.median(s[i] for s in st) * 1e3, 4) for i in range(4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="n0xn1xn2:f64|f32, comma-separated")
    ap.add_argument("--outputs", default="3,4", help="numbers of outputs K, comma-separated")
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
        for K in (int(v) for v in a.outputs.split(",")):
            # unit-modulus factors (timing only), the base filter [n1][nh][n0] real, and complex as a rotation of it
            fac = [[torch.polar(torch.ones(n, device=dev, dtype=rdt), torch.rand(n, generator=gen, device=dev, dtype=torch.float32).to(rdt) * 6.28)
                    for n in (n0, n1, nh)] for _ in range(K)]
            hreal = torch.rand(n1, nh, n0, generator=gen, device=dev, dtype=torch.float32).to(rdt)
            ym = [torch.zeros_like(x) for _ in range(K)]
            ys = [torch.zeros_like(x) for _ in range(K)]
            torch.cuda.synchronize()
            pm = api.PlanConvRealMulti(n0, n1, n2, x, ym, None, 0, 1)
            ps = [api.PlanConvReal(n0, n1, n2, x, ys[k], None, 0, 1) for k in range(K)]
            for k in range(K):
                pm.set_factors(k, *fac[k])
            for kind in ("complex", "real"):
                base = hreal if kind == "real" else hreal.to(cdt) * (0.6 + 0.8j)
                pm.set_filter(base.reshape(-1))
                for k in range(K):  # the single plans' filters: H . a_k (x) b_k (x) c_k, complex whatever the base is
                    hk = base.to(cdt) * fac[k][1][:, None, None] * fac[k][2][None, :, None] * fac[k][0][None, None, :]
                    ps[k].set_filter(hk.contiguous().reshape(-1))
                    del hk
                for _ in range(a.warmup):
                    timed_multi(torch, pm, api.EXEC_NO_TIMING)
                    timed_singles(torch, ps, api.EXEC_NO_TIMING)
                tm, ts = [], []
                for _ in range(a.reps):
                    tm.append(timed_multi(torch, pm, api.EXEC_NO_TIMING))
                    ts.append(timed_singles(torch, ps, api.EXEC_NO_TIMING))
                sm, ss = stats(tm), stats(ts)
                rec = {"case": case, "filter": kind, "K": K, "multi": sm, "singles": ss, "ratio": round(sm["median_ms"] / ss["median_ms"], 3),
                       "multi_stage_ms": stage_medians([pm]), "singles_stage_ms": stage_medians(ps), "multi_describe": pm.describe(),
                       "single_describe": ps[0].describe()}
                rows.append(rec)
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
                del base
            pm.destroy()
            for p in ps:
                p.destroy()
            del ym, ys, fac, hreal
            torch.cuda.empty_cache()
        del x
        torch.cuda.empty_cache()
    head = ["| shape | filter | K | PlanConvRealMulti ms (p10 .. p90) | K x PlanConvReal ms (p10 .. p90) | ratio | multi stages ms (YZ, exch, X, sum YZ^-1) | "
            "singles' stages ms (sums) |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        head.append(f"| {r['case']} | {r['filter']} | {r['K']} | {r['multi']['median_ms']:.3f} ({r['multi']['p10_ms']:.3f} .. {r['multi']['p90_ms']:.3f}) | "
                    f"{r['singles']['median_ms']:.3f} ({r['singles']['p10_ms']:.3f} .. {r['singles']['p90_ms']:.3f}) | {r['ratio']:.3f} | "
                    f"{' / '.join(f'{v:.3f}' for v in r['multi_stage_ms'])} | {' / '.join(f'{v:.3f}' for v in r['singles_stage_ms'])} |")
    table = "\n".join(head) + "\n"
    print(table, end="")
    if a.table:
        Path(a.table).parent.mkdir(parents=True, exist_ok=True)
        Path(a.table).write_text(table)


if __name__ == "__main__":
    main()
